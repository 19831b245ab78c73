// rtx_shade.hip — path building blocks: the other two public calls under Render, for a batch (rtx_camera_rays* and
// rtx_shade* of include/rtx.h).
//
//   camera_rays   Camera.GetRay (camera.go:265-299): one ray per lane, sample-major, with the Philox draws of event 0.
//   shade_hits    Material.Emit + Material.Scatter (ray.go:41-42, materials.go:23-113, 297-313): one record per lane,
//                 the hit taken from the caller's rtx_hit instead of a walk entry.
//
// Both are built from the megakernel's own pieces (rtx_device.h), so every float operation is the one a render
// performs: GetRay -> Hit -> Scatter in a loop is Ray.GetColor, and that loop reproduces a render bit for bit.
//
// Work distribution: no cross-wave state and no LDS.  Wave w of a launch owns records [64 w, 64 w + 64); a lane past
// the end computes on the last record and stores nothing, so every lane of every wave reaches the loads, the first
// Philox block, unit(dir) and the counting instantiation's reduce.  The only atomics are that reduce's: one per wave
// and counter.
//
// Wave votes under a partial EXEC.  unit() (one vote on the squared length for both of its fast forms) and the
// checker's parity choose between a short form and the general one by a ballot of the lanes that are there; both forms
// return the same bits for every lane the short form admits, and the ballot only sees active lanes, so a vote taken by
// a part of the wave (the lanes of one material, the lanes still rejecting in rand_unit_on_sphere) picks a form that
// is right for each of them.  The render's shade() takes the same votes inside the same branches.  Unit(r.dir) of
// Metal and Dielectric is computed by the whole wave and selected per lane, as hit_record does (rtx_walk.h).
#include "rtx_shade.h"

#include "rtx_device.h"
#include "rtx_launch_name.h"

namespace rtxd {
namespace {

constexpr uint32_t SHADE_BLOCK = 256;  // four waves; no LDS, so the size only sets the grid

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

}  // namespace

// COUNT: the counting instantiation (hits, scattered, rng_draws, texel_fetches).  NOISE: the scene has a Perlin
// texture.  The body is shade()'s material section (rtx_device.h), per lane.
// (This kernel and camera_rays: in rtxd itself, not in the unit's anonymous namespace; rtx_trace.hip, trace_rays.)
template <bool COUNT, bool NOISE>
__global__ __launch_bounds__(SHADE_BLOCK) void shade_hits(ShadeParams p) {
    const uint32_t i = blockIdx.x * SHADE_BLOCK + threadIdx.x;  // (n <= SHADE_LAUNCH_MAX: no wrap)
    const bool live = i < p.n;
    const uint32_t j = live ? i : p.n - 1u;
    // 32 + 48 + 16 B in: 2 + 3 + 1 dwordx4 loads
    const float4* rp = reinterpret_cast<const float4*>(p.rays + j);
    const float4 ra = rp[0], rb = rp[1];
    const float4* hp = reinterpret_cast<const float4*>(p.hits + j);
    const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
    const uint4 key = *reinterpret_cast<const uint4*>(p.keys + j);

    const uint32_t mi = __float_as_uint(h0.z);
    // (a material index outside the table is no hit: the record comes from the caller)
    const bool hit = live && __float_as_uint(h0.y) != RTX_HIT_NONE && mi < p.n_materials;
    const float4* mp = reinterpret_cast<const float4*>(p.materials + (hit ? mi : 0u));
    const float4 m0 = mp[0], m1 = mp[1];
    const uint32_t type = hit ? __float_as_uint(m0.x) : 0xFFFFFFFFu, tex = __float_as_uint(m0.y);
    const float fuzz = m0.z, ior = m0.w;
    const V3 albedo = v3(m1.x, m1.y, m1.z);

    const V3 rd = v3(rb.x, rb.y, rb.z);
    const V3 pt = v3(h1.x, h1.y, h1.z);  // HitInfo.point
    const V3 n = v3(h2.x, h2.y, h2.z);   // HitInfo.normal: unit, against the ray
    const float u = h1.w, v = h2.w;
    const bool front = __float_as_uint(h0.w) != 0u;
    (void)ra;  // the origin is not read: the bounce starts at the hit point

    const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), key.x, key.y};
    const uint32_t e = key.z;
    const U4 b0 = rng.block(e, 0);  // lockstep: every lane evaluates its block (e, 0) here

    // Metal and Dielectric both start from Unit(dir) and its mirror direction (the whole wave: unit's votes)
    const V3 ud = unit(rd);                                     // materials.go:61, 96
    const V3 mirror = reflect(ud, n);                           // materials.go:62, 108

    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    const bool inl = tex == RTX_DEV_TEX_INLINE;  // SolidColor, colour in albedo
    // the texture of a Lambertian (its attenuation) or a DiffuseLight (what it emits)
    V3 colour = albedo;
    if ((type == RTX_MAT_LAMBERTIAN || type == RTX_MAT_DIFFUSE_LIGHT) && !inl)
        colour = texture_value<COUNT, NOISE>(p.textures, p.texels, tex, u, v, pt, cnt);

    uint32_t draws = 0, flags = 0;
    bool scattered = false;
    V3 att = v3(0.0f, 0.0f, 0.0f), em = att, dir = att;
    if (type == RTX_MAT_LAMBERTIAN || type == RTX_MAT_METAL) {
        const V3 s = rand_unit_on_sphere(rng, e, b0, draws);    // the per-lane rejection loop
        if (type == RTX_MAT_LAMBERTIAN) {                       // materials.go:33-42
            dir = add(n, s);
            if (near_zero(dir)) dir = n;
            att = colour;
            scattered = true;
        } else {                                                // materials.go:60-75
            const V3 sc = add(mirror, scale(s, fuzz));
            if (dot(sc, n) > 0.0f) {                            // else absorbed: Emit() = 0
                dir = sc;
                att = albedo;
                scattered = true;
            }
        }
    } else if (type == RTX_MAT_DIELECTRIC) {                    // materials.go:91-113
        // 1/ior and both r0 values precomputed per material (upload_copy, rtx_render.hip)
        const float eta = front ? albedo.x : ior;
        const float d = dot(scale(ud, -1.0f), n);
        const float cos_t = d < 1.0f ? d : (d != d ? d : 1.0f); // float32(math.Min(float64(d), 1))
        const float sin_t = (float)__builtin_sqrt(1.0 - (double)(cos_t * cos_t));
        bool refl = sin_t * eta > 1.0f;
        if (!refl) {                                            // short-circuit: draw only here
            const float r0 = front ? albedo.y : albedo.z;       // ((1-eta)/(1+eta))^2, materials.go:116-118
            const float rf = r0 + (1.0f - r0) * (float)go_pow5(1.0 - (double)cos_t);
            refl = rf > unit_f32(b0.x);
            draws = 1;
        }
        dir = refl ? mirror : refract(ud, n, eta);
        att = v3(1.0f, 1.0f, 1.0f);
        scattered = true;
    } else if (type == RTX_MAT_DIFFUSE_LIGHT) {                 // emits, never scatters (materials.go:303-313)
        em = colour;
        flags = RTX_BOUNCE_EMITS;
    }
    if (scattered) flags |= RTX_BOUNCE_SCATTERED;

    if (live) {  // 64 B out: four dwordx4 stores
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4* o = reinterpret_cast<float4*>(p.out + i);
        o[0] = make_float4(att.x, att.y, att.z, __uint_as_float(flags));
        o[1] = make_float4(em.x, em.y, em.z, __uint_as_float(draws));
        o[2] = scattered ? make_float4(pt.x, pt.y, pt.z, 0.001f) : zero;           // GetColor's interval, ray.go:36
        o[3] = scattered ? make_float4(dir.x, dir.y, dir.z, __builtin_inff()) : zero;
    }
    if (COUNT) {  // reduced in the wave (every lane is here): one atomic per wave and counter
        const uint32_t nh = (uint32_t)__popcll(ballot(hit)), ns = (uint32_t)__popcll(ballot(scattered));
        const uint32_t nd = wave_sum(draws), nt = wave_sum(cnt.texel_fetches);
        if ((threadIdx.x & 63u) == 0u) {
            if (nh) atomicAdd(&p.counters[SHADE_HITS], (unsigned long long)nh);
            if (ns) atomicAdd(&p.counters[SHADE_SCATTERED], (unsigned long long)ns);
            if (nd) atomicAdd(&p.counters[SHADE_RNG_DRAWS], (unsigned long long)nd);
            if (nt) atomicAdd(&p.counters[SHADE_TEXEL_FETCHES], (unsigned long long)nt);
        }
    }
}

// GetRay for pixel blockIdx.x * SHADE_BLOCK + lane of the region's shard and sample k0 + blockIdx.y.
__global__ __launch_bounds__(SHADE_BLOCK) void camera_rays(CameraRayParams p) {
    const Shard& sh = p.shard;
    const uint64_t P = (uint64_t)sh.width * sh.rows;  // at most 2^32 - 1 (check_camera)
    const uint64_t i = (uint64_t)blockIdx.x * SHADE_BLOCK + threadIdx.x;
    const bool live = i < P;
    const uint32_t j = (uint32_t)(live ? i : P - 1u);
    const uint32_t lr = j / sh.width, xx = j - lr * sh.width;
    const uint32_t x = sh.x0 + xx, y = sh.y0 + region_row(lr, sh.rank, sh.world, sh.stripe_log2);
    const uint32_t k = sh.k0 + blockIdx.y;
    const uint32_t pixel = y * sh.cam.image_width + x;  // the GLOBAL pixel index: the RNG's counter word
    const PathRng rng{(uint32_t)sh.seed, (uint32_t)(sh.seed >> 32), pixel, k};
    uint32_t draws = 0;
    // event 0: block (0, 0) gives dx, dy and the first disk pair; the disk's rejection loop always runs
    const Ray r = camera_ray<false>(sh.cam, pixel_base(sh.cam, x, y), rng, rng.block(0, 0), draws);
    if (live) {  // 32 B (+ 16 B): two (+ one) dwordx4 stores
        const uint64_t rec = (uint64_t)blockIdx.y * P + i;
        float4* o = reinterpret_cast<float4*>(p.rays + rec);
        o[0] = make_float4(r.o.x, r.o.y, r.o.z, 0.001f);
        o[1] = make_float4(r.d.x, r.d.y, r.d.z, __builtin_inff());
        if (p.keys) *reinterpret_cast<uint4*>(p.keys + rec) = make_uint4(pixel, k, 1u, draws);
    }
}

namespace {

template <bool COUNT>
hipError_t launch_noise(const ShadeParams& p, bool noise, hipStream_t stream) {
    const dim3 grid((p.n + SHADE_BLOCK - 1) / SHADE_BLOCK), block(SHADE_BLOCK);
    const auto kern = noise ? &shade_hits<COUNT, true> : &shade_hits<COUNT, false>;
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_shade(const ShadeParams& p, bool count, bool noise, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > SHADE_LAUNCH_MAX || !p.rays || !p.hits || !p.keys || !p.out || !p.materials || !p.textures || !p.texels ||
        (count && !p.counters))
        return hipErrorInvalidValue;
    return count ? launch_noise<true>(p, noise, stream) : launch_noise<false>(p, noise, stream);
}

hipError_t launch_camera_rays(const CameraRayParams& p, hipStream_t stream) {
    const Shard& sh = p.shard;
    const uint64_t P = (uint64_t)sh.width * sh.rows;
    if (P == 0 || sh.kn == 0) return hipSuccess;
    if (P > 0xFFFFFFFFull || sh.kn > CAMERA_LAUNCH_SAMPLES || !p.rays || sh.world == 0 || sh.rank >= sh.world)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((P + SHADE_BLOCK - 1) / SHADE_BLOCK), sh.kn), block(SHADE_BLOCK);
    name_launch(&camera_rays);
    hipLaunchKernelGGL(camera_rays, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtxd
