// rtx_guides.hip — first-hit guide images (rtx_guides_device): per pixel, the mean over a range of
// samples of the albedo, normal and depth at the first hit of the render's own camera ray.
//
// The kernel is trace_rays' loop (rtx_trace.hip) with the hand-off turned inward.  One lane owns one pixel and
// produces its own rays: sample k's camera ray is camera_ray<false> of the render (event 0 of DESIGN.md §3), walked
// over the trace layout by the batched step.  A lane whose walk has ended is parked on the end sentinel.  Once
// `refill` lanes are parked with a sample to fold (or no lane walks) the whole wave forms the hit record of its
// current walks, the parked lanes fold theirs (A += a, N += n, Z += t, c += 1, in k order: a lane's samples follow
// one another) and begin their own next sample, and the other lanes keep walking.  When every lane is out of samples
// the wave stores its 64 records, two float4 each.  No ray, hit or bounce record goes through memory.
//
// Work distribution: no atomics, no cross-wave state.  Wave w owns tile w of the shard: 64 neighbouring pixels,
// 2^tile_w_log2 wide.  A lane past the shard's edge computes on the nearest pixel of the shard and stores nothing.
// Samples and walk positions only move forward, so the loop ends; nothing spins.  Every wave vote (the ballots here
// and those inside trav_begin, unit and the batched step) sits where the whole wave arrives: camera rays, walks'
// starts and hit records are computed on all 64 lanes and selected per lane, as rtx_trace.hip does.  The one vote
// under a lane's own branch is the checker's parity inside texture_value, as in shade_hits (rtx_shade.hip): both of
// its forms return the same bits for every lane that takes the short one.
#include "rtx_guides.h"

#include "rtx_device.h"
#include "rtx_trace.h"

namespace rtxd {
namespace {

constexpr int GUIDE_WAVES = 8;       // waves per workgroup (one LDS copy of the scene each)
constexpr uint32_t GUIDE_STEPS = 4;  // walk steps between two votes on the parked lanes

struct FirstHit {
    V3 a, n;
    float t;
    bool hit;
};

// What sample k adds for a lane's finished walk, computed by every lane (unit's votes): NewHitInfo (hittables.go:22-37)
// as write_hit forms it (rtx_trace.hip), then the material's colour as shade_hits reads it (rtx_shade.hip).
template <bool QUADS, bool NOISE>
__device__ __forceinline__ FirstHit first_hit(const GuideParams& p, const SceneRef E, const Trav& t, const Ray& r) {
    const bool hit = t.hit >= 0;
    const uint32_t e = hit ? (uint32_t)t.hit : 0u;  // (a miss reads entry 0 and drops it)
    const float4 sa = E.a[e];
    const float4 sb = E.b[e];
    const bool quad = QUADS && hit && __float_as_int(sb.w) == RTX_E_QUAD;
    const V3 pt = add(scale(r.d, t.closest), r.o);                                // ray.go:25-30
    const V3 ns = unit(scale(sub(pt, v3(sa.x, sa.y, sa.z)), sa.w));               // hittables.go:119-120
    V3 n = ns;
    uint32_t mi = 0u;
    float u = 0.0f, v = 0.0f;
    if (quad) {
        const uint32_t qi = 4u * (uint32_t)__float_as_int(sb.x);
        const float4 q0 = E.q[qi];
        mi = (uint32_t)__float_as_int(q0.w);
        n = v3(sa.x, sa.y, sa.z);                                                 // q.normal
        if (p.want_uv) {  // (alpha, beta) as quad_test formed them (hittables.go:181-183)
            const float4 q1 = E.q[qi + 1], q2 = E.q[qi + 2], q3 = E.q[qi + 3];
            const V3 php = sub(pt, v3(q0.x, q0.y, q0.z));
            const V3 w = v3(q3.x, q3.y, q3.z);
            u = dot(w, cross(php, v3(q2.x, q2.y, q2.z)));
            v = dot(w, cross(v3(q1.x, q1.y, q1.z), php));
        }
    } else if (hit) {
        mi = RTX_DEV_SPHERE_MATERIAL(__float_as_int(sb.w));
        if (p.want_uv) {                                                          // hittables.go:122-126
            const UV uv = sphere_uv(n.x, n.y, n.z);
            u = uv.u;
            v = uv.v;
        }
    }
    if (!(dot(r.d, n) < 0.0f)) n = scale(n, -1.0f);                               // hittables.go:23-26
    V3 a = v3(1.0f, 1.0f, 1.0f);  // a miss, a Dielectric, a DiffuseLight
    if (hit) {
        const float4* mp = reinterpret_cast<const float4*>(p.materials + mi);
        const float4 m0 = mp[0], m1 = mp[1];
        const uint32_t type = __float_as_uint(m0.x), tex = __float_as_uint(m0.y);
        const V3 albedo = v3(m1.x, m1.y, m1.z);
        Counters cnt{0, 0, 0, 0, 0, 0, 0};
        if (type == RTX_MAT_METAL) a = albedo;
        else if (type == RTX_MAT_LAMBERTIAN)  // (RTX_DEV_TEX_INLINE: a SolidColor, the colour in albedo)
            a = tex == RTX_DEV_TEX_INLINE ? albedo : texture_value<false, NOISE>(p.textures, p.texels, tex, u, v, pt, cnt);
    }
    return FirstHit{a, hit ? n : v3(0.0f, 0.0f, 0.0f), t.closest, hit};
}

// QUADS: the scene holds quads.  FIXED: the scene in the workgroup's LDS copy (scene_ref_fixed), else read from
// HBM.  NOISE: the scene has a Perlin texture.
template <bool QUADS, bool FIXED, bool NOISE>
__global__ __launch_bounds__(64 * GUIDE_WAVES) void guide_images(GuideParams p) {
    extern __shared__ float4 lds_entries[];
    SceneRef E;
    if constexpr (FIXED) {
        // scene_ref_fixed: the walk addresses LDS directly, so the copy must start at 0
        if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)lds_entries != 0u) __builtin_trap();
        const uint32_t m = p.n_entries + 1, nq4 = 4 * p.n_quads;
        for (uint32_t i = threadIdx.x; i < m; i += 64 * GUIDE_WAVES) {
            lds_entries[i] = p.entries[i];
            lds_entries[LDS_B / 16 + i] = p.entries[m + i];
        }
        for (uint32_t i = threadIdx.x; i < nq4; i += 64 * GUIDE_WAVES) lds_entries[LDS_B / 16 + m + i] = p.entries[2 * m + i];
        __syncthreads();
        E = scene_ref_fixed(lds_entries, p.n_entries, p.n_quads, 0u, 0u);
        E.prim_end = p.prim_end;
    } else {
        E = scene_ref(p.entries, p.n_entries, nullptr);
    }
    const uint32_t end = 16 * p.n_entries;  // the sentinel's position
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t twl = p.tile_w_log2, tw = 1u << twl, th = 64u >> twl;
    const uint32_t tiles_x = tiles_x_of(p.width, twl);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * GUIDE_WAVES + (threadIdx.x >> 6));
    if (wave >= tiles_x * tiles_y_of(p.rows, twl)) return;  // (the whole wave)
    const uint32_t tile_y = wave / tiles_x, tile_x = wave - tile_y * tiles_x;
    const uint32_t px = tile_x * tw + (lane & (tw - 1u)), py = tile_y * th + (lane >> twl);
    const bool live = px < p.width && py < p.rows;
    const uint32_t xx = px < p.width ? px : p.width - 1u, lr = py < p.rows ? py : p.rows - 1u;
    const uint32_t x = p.x0 + xx, y = p.y0 + region_row(lr, p.rank, p.world, p.stripe_log2);
    const uint32_t pixel = y * p.cam.image_width + x;  // the GLOBAL pixel index: the RNG's counter word
    const V3 base = pixel_base(p.cam, x, y);
    const uint32_t s0 = (uint32_t)p.seed, s1 = (uint32_t)(p.seed >> 32);

    uint32_t k = p.k0;                   // the lane's sample: walking it, or parked on its end
    const uint32_t kend = p.k0 + p.kn;   // (at most 2^32 - 1: the entry's check)
    uint32_t draws = 0;
    Ray r;
    {
        const PathRng rng{s0, s1, pixel, k};
        r = camera_ray<false>(p.cam, base, rng, rng.block(0, 0), draws);
    }
    Trav t{};
    trav_begin(t, r, p.start);
    V3 A = v3(0.0f, 0.0f, 0.0f), N = A;
    float Z = 0.0f;
    uint32_t c = 0;
    Counters cnt{0, 0, 0, 0, 0, 0, 0};

    for (;;) {
        const bool parked = t.i >= end;
        const bool pend = parked && k < kend;  // a finished walk, not folded yet
        const uint32_t np = (uint32_t)__popcll(ballot(pend));
        if (np >= p.refill || ballot(!parked) == 0) {
            if (np == 0u) break;  // every lane parked and out of samples
            const FirstHit h = first_hit<QUADS, NOISE>(p, E, t, r);
            if (pend) {
                A = add(A, h.a);
                N = add(N, h.n);
                if (h.hit) {
                    Z += h.t;
                    ++c;
                }
                ++k;
            }
            // the parked lanes' own next samples (the whole wave: trav_begin's votes)
            const PathRng rng{s0, s1, pixel, k};
            const Ray nr = camera_ray<false>(p.cam, base, rng, rng.block(0, 0), draws);
            Trav nt;
            trav_begin(nt, nr, p.start);
            if (pend && k < kend) {
                r = nr;
                t = nt;
            }  // (else walking on, or out of samples: it stays on the sentinel)
        }
        // GUIDE_STEPS walk steps: the med3 / div_by forms when every walking lane's ray is safe (traverse_phase)
        uint32_t idle = 0;
        if (ballot(!t.safe && t.i < end) == 0) {
#pragma unroll
            for (uint32_t s = 0; s < GUIDE_STEPS; ++s)
                trav_step_batched<false, QUADS, FIXED, false, true>(t, r, E, cnt, end, p.prim_batch, idle);
        } else {
#pragma unroll
            for (uint32_t s = 0; s < GUIDE_STEPS; ++s)
                trav_step_batched<false, QUADS, FIXED, false, false>(t, r, E, cnt, end, p.prim_batch, idle);
        }
    }
    if (live) {  // 32 B: two dwordx4 stores
        const float inv = 1.0f / (float)p.kn;
        float4* o = reinterpret_cast<float4*>(p.out + ((uint64_t)lr * p.width + xx));
        o[0] = make_float4(A.x * inv, A.y * inv, A.z * inv, (float)c * inv);
        o[1] = make_float4(N.x * inv, N.y * inv, N.z * inv, c ? Z / (float)c : 0.0f);
    }
}

template <bool QUADS, bool FIXED>
hipError_t launch_noise(const GuideParams& p, bool noise, hipStream_t stream) {
    const size_t shmem = FIXED ? LDS_B + (p.n_entries + 1) * 16 + p.n_quads * 64 : 0;  // trace_lds_bytes (rtx_trace.hip)
    const uint64_t tiles = (uint64_t)tiles_x_of(p.width, p.tile_w_log2) * tiles_y_of(p.rows, p.tile_w_log2);
    const dim3 grid((uint32_t)((tiles + GUIDE_WAVES - 1) / GUIDE_WAVES)), block(64 * GUIDE_WAVES);
    if (noise) hipLaunchKernelGGL((guide_images<QUADS, FIXED, true>), grid, block, shmem, stream, p);
    else hipLaunchKernelGGL((guide_images<QUADS, FIXED, false>), grid, block, shmem, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_guides(const GuideParams& p, bool noise, hipStream_t stream) {
    const uint64_t P = (uint64_t)p.width * p.rows;
    if (P == 0) return hipSuccess;
    if (P > 0xFFFFFFFFull || p.kn == 0 || (uint64_t)p.k0 + p.kn > 0xFFFFFFFFull || p.tile_w_log2 > 6u || p.refill == 0 ||
        p.refill > 64u || p.world == 0 || p.rank >= p.world || !p.entries || !p.materials || !p.textures || !p.texels ||
        !p.out)
        return hipErrorInvalidValue;
    const bool fixed = trace_placement(p.n_entries, p.n_quads) == RTX_SCENE_IN_LDS;
    if (p.n_quads) return fixed ? launch_noise<true, true>(p, noise, stream) : launch_noise<true, false>(p, noise, stream);
    return fixed ? launch_noise<false, true>(p, noise, stream) : launch_noise<false, false>(p, noise, stream);
}

}  // namespace rtxd
