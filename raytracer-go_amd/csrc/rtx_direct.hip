// rtx_direct.hip — direct light sampling for a batch of hits (rtx_direct_device): one light sample per
// record and the answer of its shadow ray, in one kernel.
//
//   sample   the contract of include/rtx.h ("direct light sampling"), computed with the render's own device functions
//            (rtx_device.h: the Philox block, texture_value, sphere_uv, unit, and the unit-sphere loop of
//            rand_unit_on_sphere with its attempts on blocks 1, 2, ..): float32, each operation rounded, no contraction.
//   shadow   trace_rays' any-hit walk (rtx_trace.hip) over the same trace layout: trav_begin, then walk_steps
//            (rtx_walk.h) with the ray's own tmin and the bound starting at tmax = 0.999, a lane parking at its first
//            accepted primitive.
//
// Work distribution: no cross-wave state.  Wave w owns records [w * range, (w + 1) * range) and takes them 64 at a
// time, the plain form of trace_rays (refill = 64): the block's samples are computed, its shadow rays are walked
// until every lane is parked on the end sentinel, the 64 records are stored.  A lane past the end of the range
// computes on the range's last record and stores nothing; a lane without a shadow ray starts parked.  Walk positions
// only move forward and the range is finite, so both loops end; nothing spins.  The only atomics are the counting
// instantiation's: one per wave and counter, after the wave's last block.
//
// Wave votes.  The ballots here, in trav_begin and in the batched step sit where the whole wave arrives.  unit()'s
// one vote on the squared length and the checker's parity (texture_value) are reached under a lane's own branch, as
// in shade_hits (rtx_shade.hip): both of their forms return the same bits for every lane the short form admits, and
// a ballot only sees the lanes that are there.
#include "rtx_direct.h"

#include "rtx_launch_name.h"
#include "rtx_trace.h"
#include "rtx_walk.h"

namespace rtxd {
namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// What a light sample reads of the scene copy.
struct LightTables {
    const rtx_material* materials;
    const rtx_texture* textures;
    const uint32_t* texels;
    const float4* lights;
    uint32_t n_lights;
};

// The texture of a Lambertian or a DiffuseLight (device material m0, m1) at (u, v, pt).
template <bool NOISE>
__device__ __forceinline__ V3 material_colour(const LightTables& p, const float4 m0, const float4 m1, float u, float v,
                                              V3 pt) {
    const uint32_t tex = __float_as_uint(m0.y);
    if (tex == RTX_DEV_TEX_INLINE) return v3(m1.x, m1.y, m1.z);  // a SolidColor, the colour in albedo
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    return texture_value<false, NOISE>(p.textures, p.texels, tex, u, v, pt, cnt);
}

// One light sample (the contract of rtx.h, "direct light sampling") at the Lambertian hit (pt, n, u, v) of device
// material (m0, m1), for the lanes with `lam`; b0 is block (e, 0) of the light event e, drawn by every lane.
struct LightSample {
    bool sampled;
    uint32_t j, draws;
    float g;
    V3 rad, w;  // (a * Le) * g; q - p, the shadow ray's direction
};
template <bool NOISE>
__device__ __forceinline__ LightSample light_sample(const LightTables& p, const bool lam, const float4 m0, const float4 m1,
                                                    const V3 pt, const V3 n, const float hu, const float hv,
                                                    const PathRng& rng, const uint32_t e, const U4 b0) {
    const float pi32 = 3.14159274101257324f;  // PiF32, math.go:48
    const float fL = (float)p.n_lights;       // exact: L <= 2^24
    LightSample s{false, 0u, 0u, 0.0f, v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f)};
    if (lam) {
        const uint32_t jf = (uint32_t)(unit_f32(b0.x) * fL);
        s.j = jf < p.n_lights - 1u ? jf : p.n_lights - 1u;
        const float4* lp = p.lights + 4u * s.j;
        const float4 l0 = lp[0], l1 = lp[1], l2 = lp[2], l3 = lp[3];
        const float area = l1.w;
        V3 q, nl;
        float lu, lv;
        s.draws = 1;
        if (__float_as_uint(l2.w) == RTX_PRIM_QUAD) {
            lu = unit_f32(b0.y);
            lv = unit_f32(b0.z);
            s.draws += 2;
            q = add(add(v3(l0.x, l0.y, l0.z), scale(v3(l1.x, l1.y, l1.z), lu)), scale(v3(l2.x, l2.y, l2.z), lv));
            nl = v3(l3.x, l3.y, l3.z);
        } else {
            V3 d = v3(0.0f, 0.0f, 0.0f);
            for (uint32_t a = 1;; ++a) {  // vec3.go:182-190, attempt a on block (e, a): the per-lane rejection loop
                const U4 b = rng.block(e, a);
                const V3 c = v3(signed_unit(b.x), signed_unit(b.y), signed_unit(b.z));
                s.draws += 3;
                if (lensq(c) < 1.0f) {
                    d = unit(c);
                    break;
                }
            }
            q = add(v3(l0.x, l0.y, l0.z), scale(d, l0.w));
            nl = d;
            const UV uv = sphere_uv(d.x, d.y, d.z);  // hittables.go:122-126
            lu = uv.u;
            lv = uv.v;
        }
        s.w = sub(q, pt);
        const float d2 = dot(s.w, s.w);
        const float dist = (float)__builtin_sqrt((double)d2);  // vec3.go:119-121
        const float cs = dot(n, s.w) / dist;
        const float cl = __builtin_fabsf(dot(nl, s.w)) / dist;
        s.sampled = d2 > 0.0f && cs > 0.0f && cl > 0.0f;  // (a NaN fails)
        if (s.sampled) {
            s.g = (((cs * cl) * area) * fL) / (pi32 * d2);
            const V3 a = material_colour<NOISE>(p, m0, m1, hu, hv, pt);
            const float4* ep = reinterpret_cast<const float4*>(p.materials + __float_as_uint(l3.w));
            const V3 le = material_colour<NOISE>(p, ep[0], ep[1], lu, lv, q);
            s.rad = scale(mul(a, le), s.g);
        }
    }
    return s;
}

// ---- multiple importance sampling (rtx.h, "multiple importance sampling of the direct light") ------
// (area, light index) of rtx_hit's prim word in the per-primitive lookup; a word that names no primitive of the
// scene (a miss, a caller's own record) is no emitter.
__device__ __forceinline__ float2 prim_light(const PrimLights& t, const uint32_t prim) {
    const uint32_t kind = prim >> 28, idx = prim & 0x0FFFFFFFu;
    const bool sph = kind == RTX_PRIM_SPHERE && idx < t.n_spheres, quad = kind == RTX_PRIM_QUAD && idx < t.n_quads;
    if (!sph && !quad) return make_float2(0.0f, __uint_as_float(RTX_LIGHT_NONE));
    return t.tab[sph ? idx : t.n_spheres + idx];
}

// The weight of a bounce that left the Lambertian hit (from_pt, from_n) and found (hit_pt, hit_n) on an emitter of
// area `area` (0: the table excludes it): the contract's g and wb = 1 - 1 / (1 + g * g), each operation rounded.
struct BounceWeight {
    bool weighted;
    float wb, g;
};
__device__ __forceinline__ BounceWeight bounce_weight(const float area, const float fL, const V3 from_pt, const V3 from_n,
                                                      const V3 hit_pt, const V3 hit_n) {
    const float pi32 = 3.14159274101257324f;  // PiF32, math.go:48
    const V3 w = sub(hit_pt, from_pt);
    const float d2 = dot(w, w);
    const float dist = (float)__builtin_sqrt((double)d2);  // vec3.go:119-121
    const float cs = dot(from_n, w) / dist;
    const float cl = __builtin_fabsf(dot(hit_n, w)) / dist;
    const float g = (((cs * cl) * area) * fL) / (pi32 * d2);
    const bool ok = area > 0.0f && d2 > 0.0f && g == g;  // (a NaN fails)
    const float wb = 1.0f - 1.0f / (1.0f + g * g);
    return BounceWeight{ok, ok ? wb : 1.0f, ok ? g : 0.0f};
}

// The light sample's weight of its own g.
__device__ __forceinline__ float light_weight(const float g) { return 1.0f / (1.0f + g * g); }

}  // namespace

// The three kernels: in rtxd itself, not in the unit's anonymous namespace (rtx_trace.hip, trace_rays).
// rtx_emitter_weight_device: a thread per record, 64 records per wave step, no walk and no cross-lane state but the
// counting instantiation's sum (every lane of a launched wave reaches it).
template <bool COUNT>
__global__ __launch_bounds__(256) void emitter_weights(EmitterWeightParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < p.n;
    const uint32_t rec = live ? i : p.n - 1u;
    // 2 x 48 B in: 3 + 3 dwordx4 loads
    const float4* fp = reinterpret_cast<const float4*>(p.from + rec);
    const float4* hp = reinterpret_cast<const float4*>(p.hits + rec);
    const float4 f0 = fp[0], f1 = fp[1], f2 = fp[2], h0 = hp[0], h1 = hp[1], h2 = hp[2];
    const uint32_t fm = __float_as_uint(f0.z), hm = __float_as_uint(h0.z), prim = __float_as_uint(h0.y);
    // (a material index outside the table is no hit: the records come from the caller)
    const bool from_ok = __float_as_uint(f0.y) != RTX_HIT_NONE && fm < p.n_materials;
    const bool hit_ok = prim != RTX_HIT_NONE && hm < p.n_materials;
    const float4 fm0 = *reinterpret_cast<const float4*>(p.materials + (from_ok ? fm : 0u));  // the device form: type in .x
    const float4 hm0 = *reinterpret_cast<const float4*>(p.materials + (hit_ok ? hm : 0u));
    const bool pair = from_ok && hit_ok && __float_as_uint(fm0.x) == RTX_MAT_LAMBERTIAN &&
                      __float_as_uint(hm0.x) == RTX_MAT_DIFFUSE_LIGHT;
    float2 pl = make_float2(0.0f, __uint_as_float(RTX_LIGHT_NONE));
    if (pair) pl = prim_light(p.prims, prim);
    const BounceWeight bw = bounce_weight(pl.x, (float)p.n_lights, v3(f1.x, f1.y, f1.z), v3(f2.x, f2.y, f2.z),
                                          v3(h1.x, h1.y, h1.z), v3(h2.x, h2.y, h2.z));
    const bool weighted = pair && bw.weighted;
    if (live)  // 16 B out: one dwordx4 store
        *reinterpret_cast<float4*>(p.out + i) = make_float4(weighted ? bw.wb : 1.0f, weighted ? bw.g : 0.0f, pl.y,
                                                            __uint_as_float(weighted ? RTX_EMITTER_WEIGHTED : 0u));
    if (COUNT) {
        const uint32_t nw = wave_sum(live && weighted ? 1u : 0u);
        if ((threadIdx.x & 63u) == 0u && nw) atomicAdd(&p.counters[EMITTER_WEIGHTED], (unsigned long long)nw);
    }
}

// COUNT: the counting instantiation (sampled, visible, rng_draws).  QUADS: the scene holds quads.  FIXED: the scene
// in the workgroup's LDS copy (scene_ref_fixed), else read from HBM.  NOISE: the scene has a Perlin texture.
template <bool COUNT, bool QUADS, bool FIXED, bool NOISE>
__global__ __launch_bounds__(64 * WALK_WAVES) void direct_lights(DirectParams p) {
    extern __shared__ float4 lds_entries[];
    const SceneRef E = stage_scene<WALK_WAVES, FIXED>(lds_entries, p.scene);
    const uint32_t end = walk_end(p.scene);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WALK_WAVES + (threadIdx.x >> 6));
    const uint64_t first = (uint64_t)wave * p.range;
    if (first >= p.n) return;  // (the whole wave)
    const uint32_t last = (uint32_t)(first + p.range < p.n ? first + p.range : p.n);  // the wave's records: [first, last)
    const LightTables tabs{p.materials, p.textures, p.texels, p.lights, p.n_lights};
    uint32_t n_sampled = 0, n_visible = 0, n_draws = 0;  // COUNT (per lane)

    for (uint32_t blk = (uint32_t)first; blk < last; blk += 64u) {
        const uint32_t i = blk + lane;
        const bool live = i < last;
        const uint32_t rec = live ? i : last - 1u;
        // 48 + 16 B in: 3 + 1 dwordx4 loads
        const float4* hp = reinterpret_cast<const float4*>(p.hits + rec);
        const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
        const uint4 key = *reinterpret_cast<const uint4*>(p.keys + rec);
        const uint32_t mi = __float_as_uint(h0.z);
        // (a material index outside the table is no hit: the record comes from the caller)
        const bool hit = live && __float_as_uint(h0.y) != RTX_HIT_NONE && mi < p.n_materials;
        const float4* mp = reinterpret_cast<const float4*>(p.materials + (hit ? mi : 0u));
        const float4 m0 = mp[0], m1 = mp[1];
        const bool lam = hit && __float_as_uint(m0.x) == RTX_MAT_LAMBERTIAN && p.n_lights != 0u;

        const V3 pt = v3(h1.x, h1.y, h1.z);  // HitInfo.point
        const V3 n = v3(h2.x, h2.y, h2.z);   // HitInfo.normal: unit, against the ray
        const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), key.x, key.y};
        const uint32_t e = DIRECT_EVENT | key.z;
        const U4 b0 = rng.block(e, 0);  // lockstep: every lane evaluates its block (e, 0) here

        const LightSample ls = light_sample<NOISE>(tabs, lam, m0, m1, pt, n, h1.w, h2.w, rng, e, b0);
        const uint32_t j = ls.j, draws = ls.draws;
        uint32_t flags = ls.sampled ? RTX_DIRECT_SAMPLED : 0u;
        const float g = ls.g;
        const V3 rad = ls.rad, w = ls.w;
        const bool sampled = ls.sampled;

        // the shadow walk (the whole wave: trav_begin's votes); a lane without a shadow ray starts parked
        const Ray r = sampled ? Ray{pt, w} : Ray{v3(0.0f, 0.0f, 0.0f), v3(1.0f, 1.0f, 1.0f)};
        const float tmin = 0.001f;
        Trav t;
        trav_begin(t, r, sampled ? p.scene.start : end);
        t.safe = t.safe && tmin >= 0x1p-42f;  // as trace_rays: the fast step forms need every accepted root in div_by's claim
        t.closest = 0.999f;                    // the running bound starts at the ray's tmax
        Counters cnt{0, 0, 0, 0, 0, 0, 0};
        while (ballot(t.i < end) != 0)
            t = walk_steps<WALK_STEPS, false, QUADS, FIXED>(t, r, E, cnt, end, p.prim_batch, tmin, true);
        const bool visible = sampled && t.hit < 0;
        if (visible) flags |= RTX_DIRECT_VISIBLE;

        if (live) {  // 64 B out: four dwordx4 stores
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float4* o = reinterpret_cast<float4*>(p.out + i);
            o[0] = make_float4(rad.x, rad.y, rad.z, __uint_as_float(flags));
            o[1] = sampled ? make_float4(pt.x, pt.y, pt.z, tmin) : zero;
            o[2] = sampled ? make_float4(w.x, w.y, w.z, 0.999f) : zero;
            o[3] = make_float4(__uint_as_float(j), __uint_as_float(draws), g, 0.0f);
        }
        if (COUNT) {
            n_sampled += sampled ? 1u : 0u;
            n_visible += visible ? 1u : 0u;
            n_draws += live ? draws : 0u;
        }
    }
    if (COUNT) {  // reduced in the wave (every lane is here): one atomic per wave and counter
        const uint32_t ns = wave_sum(n_sampled), nv = wave_sum(n_visible), nd = wave_sum(n_draws);
        if (lane == 0u) {
            if (ns) atomicAdd(&p.counters[DIRECT_SAMPLED], (unsigned long long)ns);
            if (nv) atomicAdd(&p.counters[DIRECT_VISIBLE], (unsigned long long)nv);
            if (nd) atomicAdd(&p.counters[DIRECT_RNG_DRAWS], (unsigned long long)nd);
        }
    }
}

// ---- the fused pass (rtx_accum_add_direct) ----------------------------------------------------------------------
// direct_paths is guide_images' loop (rtx_guides.hip) carried through a whole path.  A wave owns one 64-pixel tile of the
// accumulator's S / Q layout and a lane owns a pixel.  A lane's walk is either a closest-hit walk (a path segment) or a
// shadow walk; a lane whose walk has ended is parked on the end sentinel.  Once `refill` lanes are parked with work (or
// no lane walks) the whole wave runs one FOLD STEP: every lane forms the hit record of its walk (hit_record,
// rtx_walk.h), shades it with shade_hits' per-record code (rtx_shade.hip) and samples a light (light_sample); the
// parked lanes then apply the estimator of DESIGN.md §37 to their own result and start the shadow ray, or the bounce
// ray when nothing was sampled, or the next sample's camera ray; a parked shadow walk adds or drops its radiance and
// starts the saved bounce.  No ray, hit, bounce or path state goes through memory; no atomics; nothing spins (samples,
// segments and walk positions only move forward); every vote (here, in trav_begin, unit, the batched step) sits where
// the whole wave arrives, except those inside a lane's own material branch, as in shade_hits.
// QUADS: the scene holds quads.  FIXED: the scene in the workgroup's LDS copy, else read from HBM.  NOISE: the scene has
// a Perlin texture.  MIS: the estimator of rtx_accum_add_mis: the lane also keeps the normal of the
// Lambertian hit its bounce left (r.o is that hit's point), a bounce that finds an emitter is weighted by bounce_weight
// of the per-primitive lookup, a light sample by light_weight of its g.  Every MIS line is under `if (MIS)`: the
// MIS = false instantiations are what they were.
template <bool QUADS, bool FIXED, bool NOISE, bool MIS>
__global__ __launch_bounds__(64 * WALK_WAVES) void direct_paths(DirectPathParams p) {
    extern __shared__ float4 lds_entries[];
    const SceneRef E = stage_scene<WALK_WAVES, FIXED>(lds_entries, p.scene);
    const uint32_t end = walk_end(p.scene);
    const uint32_t lane = threadIdx.x & 63u;
    const Shard& sh = p.shard;
    const uint32_t twl = p.tile_w_log2;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WALK_WAVES + (threadIdx.x >> 6));
    if (wave >= tiles_x_of(sh.width, twl) * tiles_y_of(sh.rows, twl)) return;  // (the whole wave)
    const TilePixel tp = tile_pixel(sh, twl, wave, lane);
    const bool live = tp.live;  // (a lane outside a ragged tile computes on the nearest pixel)
    const uint32_t pixel = tp.pixel;
    const V3 base = tp.base;
    const uint32_t s0 = (uint32_t)sh.seed, s1 = (uint32_t)(sh.seed >> 32);
    const LightTables tabs{p.materials, p.textures, p.texels, p.lights, p.n_lights};
    const V3 bg = v3(sh.cam.background[0], sh.cam.background[1], sh.cam.background[2]);
    const V3 zero = v3(0.0f, 0.0f, 0.0f), one = v3(1.0f, 1.0f, 1.0f);
    const uint32_t depth = sh.cam.max_depth;
    const bool want_uv = p.want_uv != 0u;

    uint32_t k = sh.k0;                   // the lane's sample
    const uint32_t kend = sh.k0 + sh.kn;  // (at most 2^32 - 1: the entry's check)
    uint32_t seg = 0, cam_draws = 0;
    bool shadow = false, diffuse = false;
    V3 from_n = zero;  // MIS: the normal of the Lambertian hit the walking bounce left
    V3 T = one, Lc = zero, pending = zero, bounce = zero;  // pending: T * radiance of the walking shadow ray; bounce: the saved direction
    // the lane's slot of the tile-major moments: the pass continues the sums in k order (passes of one accumulator
    // are ordered by the caller), so they are read here and written back at the end
    const size_t slot = ((size_t)wave * 64u + lane) * 3u;
    V3 S = zero, Q = zero;
    if (live) {
        S = v3(p.acc_s[slot], p.acc_s[slot + 1], p.acc_s[slot + 2]);
        Q = v3(p.acc_q[slot], p.acc_q[slot + 1], p.acc_q[slot + 2]);
    }
    Ray r;
    {
        const PathRng rng{s0, s1, pixel, k};
        r = camera_ray<false>(sh.cam, base, rng, rng.block(0, 0), cam_draws);
    }
    Trav t{};
    trav_begin(t, r, p.scene.start);
    Counters cnt{0, 0, 0, 0, 0, 0, 0};

    for (;;) {
        const bool parked = t.i >= end;
        const bool pend = parked && k < kend;  // a finished walk, not folded yet
        const uint32_t np = (uint32_t)__popcll(ballot(pend));
        if (np >= p.refill || ballot(!parked) == 0) {
            if (np == 0u) break;  // every lane parked and out of samples
            // -- the fold step, whole wave.  What follows is computed by every lane on its own walk and kept where
            //    `seg_end` (a parked closest walk) or `sh_end` (a parked shadow walk) says so.
            const bool seg_end = pend && !shadow, sh_end = pend && shadow;
            const HitRecord h = hit_record<QUADS, MIS>(E, t, r, want_uv, p.rank_sphere);
            const bool hit = seg_end && h.hit && h.mi < p.n_materials;
            const float4* mp = reinterpret_cast<const float4*>(p.materials + (hit ? h.mi : 0u));
            const float4 m0 = mp[0], m1 = mp[1];
            const uint32_t type = hit ? __float_as_uint(m0.x) : 0xFFFFFFFFu, tex = __float_as_uint(m0.y);
            const float fuzz = m0.z, ior = m0.w;
            const V3 albedo = v3(m1.x, m1.y, m1.z);
            const PathRng rng{s0, s1, pixel, k};
            const uint32_t e = seg + 1u;    // the scatter after segment seg
            const U4 b0 = rng.block(e, 0);  // lockstep
            const V3 ud = unit(r.d);                                    // materials.go:61, 96
            const V3 mirror = reflect(ud, h.n);                         // materials.go:62, 108
            // shade_hits' material section (rtx_shade.hip)
            V3 colour = albedo;
            if ((type == RTX_MAT_LAMBERTIAN || type == RTX_MAT_DIFFUSE_LIGHT) && tex != RTX_DEV_TEX_INLINE)
                colour = texture_value<false, NOISE>(p.textures, p.texels, tex, h.u, h.v, h.pt, cnt);
            uint32_t draws = 0;
            bool scattered = false, emits = false;
            V3 att = zero, em = zero, dir = zero;
            if (type == RTX_MAT_LAMBERTIAN || type == RTX_MAT_METAL) {
                const V3 s = rand_unit_on_sphere(rng, e, b0, draws);    // the per-lane rejection loop
                if (type == RTX_MAT_LAMBERTIAN) {                       // materials.go:33-42
                    dir = add(h.n, s);
                    if (near_zero(dir)) dir = h.n;
                    att = colour;
                    scattered = true;
                } else {                                                // materials.go:60-75
                    const V3 sc = add(mirror, scale(s, fuzz));
                    if (dot(sc, h.n) > 0.0f) {                          // else absorbed
                        dir = sc;
                        att = albedo;
                        scattered = true;
                    }
                }
            } else if (type == RTX_MAT_DIELECTRIC) {                    // materials.go:91-113
                const float eta = h.front ? albedo.x : ior;
                const float d = dot(scale(ud, -1.0f), h.n);
                const float cos_t = d < 1.0f ? d : (d != d ? d : 1.0f); // float32(math.Min(float64(d), 1))
                const float sin_t = (float)__builtin_sqrt(1.0 - (double)(cos_t * cos_t));
                bool refl = sin_t * eta > 1.0f;
                if (!refl) {                                            // short-circuit: draw only here
                    const float r0 = h.front ? albedo.y : albedo.z;     // materials.go:116-118
                    const float rf = r0 + (1.0f - r0) * (float)go_pow5(1.0 - (double)cos_t);
                    refl = rf > unit_f32(b0.x);
                }
                dir = refl ? mirror : refract(ud, h.n, eta);
                att = one;
                scattered = true;
            } else if (type == RTX_MAT_DIFFUSE_LIGHT) {                 // emits, never scatters
                em = colour;
                emits = true;
            }
            // the light sample at this hit (its own event range, lockstep block 0)
            const uint32_t le = DIRECT_EVENT | e;
            const U4 lb0 = rng.block(le, 0);
            const bool lam = hit && type == RTX_MAT_LAMBERTIAN;  // (a Lambertian always scatters)
            const bool want_light = lam && seg + 1u < depth && p.n_lights != 0u;
            const LightSample ls = light_sample<NOISE>(tabs, want_light, m0, m1, h.pt, h.n, h.u, h.v, rng, le, lb0);

            // -- the estimator, per lane; every * and + rounded on its own
            bool sample_done = false, start_shadow = false, start_bounce = false;
            V3 next_o = r.o, next_d = r.d;
            if (sh_end) {
                if (t.hit < 0) Lc = add(Lc, pending);
                next_d = bounce;  // (the shadow ray started at the hit point: the origin stays)
                shadow = false;
                start_bounce = true;
            } else if (seg_end) {
                if (seg >= depth) {  // (max_depth 0: GetColor returns black before it looks, ray.go:33)
                    sample_done = true;
                } else if (!hit) {
                    Lc = add(Lc, mul(T, bg));                           // ray.go:52
                    sample_done = true;
                } else {
                    if (emits && !diffuse) Lc = add(Lc, mul(T, em));    // ray.go:41, 47
                    if (MIS && emits && diffuse) {                      // the bounce's share of this emitter point
                        const float area = prim_light(p.prims, h.prim).x;
                        const BounceWeight bw = bounce_weight(area, (float)p.n_lights, r.o, from_n, h.pt, h.n);
                        Lc = add(Lc, mul(T, scale(em, bw.wb)));
                    }
                    if (ls.sampled) pending = MIS ? mul(T, scale(ls.rad, light_weight(ls.g))) : mul(T, ls.rad);
                    if (!scattered) {
                        sample_done = true;
                    } else {
                        T = mul(T, att);                                // ray.go:47-50
                        diffuse = lam && p.n_lights != 0u;
                        if (MIS && lam) from_n = h.n;
                        ++seg;
                        if (seg >= depth) {
                            sample_done = true;                         // the depth cap: nothing more is added
                        } else if (ls.sampled) {
                            bounce = dir;
                            next_o = h.pt;
                            next_d = ls.w;
                            shadow = true;
                            start_shadow = true;
                        } else {
                            next_o = h.pt;
                            next_d = dir;
                            start_bounce = true;
                        }
                    }
                }
            }
            if (sample_done) {  // S += c; Q += c * c, in k order (a lane's samples follow one another)
                S = add(S, Lc);
                Q = v3(Q.x + __fmul_rn(Lc.x, Lc.x), Q.y + __fmul_rn(Lc.y, Lc.y), Q.z + __fmul_rn(Lc.z, Lc.z));
                ++k;
                T = one;
                Lc = zero;
                seg = 0;
                diffuse = false;
            }
            // the next sample's camera ray (the whole wave: its rejection loop and unit's votes)
            const PathRng crng{s0, s1, pixel, k};
            const Ray cr = camera_ray<false>(sh.cam, base, crng, crng.block(0, 0), cam_draws);
            Ray nr = Ray{next_o, next_d};
            if (sample_done) nr = cr;
            const bool go = start_shadow || start_bounce || (sample_done && k < kend);
            Trav nt;
            trav_begin(nt, nr, go ? p.scene.start : end);  // (whole wave: its votes)
            if (start_shadow) nt.closest = 0.999f;   // the shadow ray's tmax; tmin = 0.001 either way
            if (pend) {
                r = nr;
                t = nt;  // (out of samples: parked on the sentinel for good)
            }
        }
        // WALK_STEPS walk steps, written out here: walk_steps (rtx_walk.h) with this kernel's per-lane park flag moved
        // the hot loop's code and add_direct measured 0.45 % longer, past the parent's own spread.
        // The med3 / div_by forms when every walking lane's ray is safe (traverse_phase).
        uint32_t idle = 0;
        if (ballot(!t.safe && t.i < end) == 0) {
#pragma unroll
            for (uint32_t s = 0; s < WALK_STEPS; ++s) {
                trav_step_batched<false, QUADS, FIXED, false, true>(t, r, E, cnt, end, p.prim_batch, idle);
                if (shadow && t.hit >= 0) t.i = end;  // any-hit: park at the first accepted primitive
            }
        } else {
#pragma unroll
            for (uint32_t s = 0; s < WALK_STEPS; ++s) {
                trav_step_batched<false, QUADS, FIXED, false, false>(t, r, E, cnt, end, p.prim_batch, idle);
                if (shadow && t.hit >= 0) t.i = end;
            }
        }
    }
    if (live) {  // (a lane outside a ragged tile leaves its slot zero, as accumulate_samples does)
        p.acc_s[slot] = S.x;
        p.acc_s[slot + 1] = S.y;
        p.acc_s[slot + 2] = S.z;
        p.acc_q[slot] = Q.x;
        p.acc_q[slot + 1] = Q.y;
        p.acc_q[slot + 2] = Q.z;
    }
}

namespace {

template <bool QUADS, bool FIXED>
hipError_t launch_paths_noise(const DirectPathParams& p, bool noise, bool mis, hipStream_t stream) {
    const size_t shmem = FIXED ? walk_lds_bytes(p.scene.n_entries, p.scene.n_quads) : 0;
    const uint64_t tiles = (uint64_t)tiles_x_of(p.shard.width, p.tile_w_log2) * tiles_y_of(p.shard.rows, p.tile_w_log2);
    const dim3 grid((uint32_t)((tiles + WALK_WAVES - 1) / WALK_WAVES)), block(64 * WALK_WAVES);
    const auto kern = mis ? (noise ? &direct_paths<QUADS, FIXED, true, true> : &direct_paths<QUADS, FIXED, false, true>)
                          : (noise ? &direct_paths<QUADS, FIXED, true, false> : &direct_paths<QUADS, FIXED, false, false>);
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, shmem, stream, p);
    return hipGetLastError();
}

template <bool COUNT, bool QUADS, bool FIXED>
hipError_t launch_noise(const DirectParams& p, bool noise, hipStream_t stream) {
    const size_t shmem = FIXED ? walk_lds_bytes(p.scene.n_entries, p.scene.n_quads) : 0;
    const uint64_t waves = ((uint64_t)p.n + p.range - 1) / p.range;
    const dim3 grid((uint32_t)((waves + WALK_WAVES - 1) / WALK_WAVES)), block(64 * WALK_WAVES);
    const auto kern = noise ? &direct_lights<COUNT, QUADS, FIXED, true> : &direct_lights<COUNT, QUADS, FIXED, false>;
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, shmem, stream, p);
    return hipGetLastError();
}

template <bool COUNT>
hipError_t launch_count(const DirectParams& p, bool noise, hipStream_t stream) {
    const bool fixed = trace_placement(p.scene.n_entries, p.scene.n_quads) == RTX_SCENE_IN_LDS;
    if (p.scene.n_quads) return fixed ? launch_noise<COUNT, true, true>(p, noise, stream) : launch_noise<COUNT, true, false>(p, noise, stream);
    return fixed ? launch_noise<COUNT, false, true>(p, noise, stream) : launch_noise<COUNT, false, false>(p, noise, stream);
}

}  // namespace

hipError_t launch_direct(const DirectParams& p, bool count, bool noise, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > DIRECT_LAUNCH_MAX || p.range == 0 || p.range % 64u != 0 || !p.hits || !p.keys || !p.out || !p.scene.entries ||
        !p.materials || !p.textures || !p.texels || (p.n_lights && !p.lights) || p.n_lights > (1u << 24) ||
        (count && !p.counters))
        return hipErrorInvalidValue;
    return count ? launch_count<true>(p, noise, stream) : launch_count<false>(p, noise, stream);
}

hipError_t launch_emitter_weights(const EmitterWeightParams& p, bool count, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > DIRECT_LAUNCH_MAX || !p.from || !p.hits || !p.out || !p.materials || !p.prims.tab || p.n_lights > (1u << 24) ||
        (count && !p.counters))
        return hipErrorInvalidValue;
    const dim3 grid((p.n + 255u) / 256u), block(256);
    const auto kern = count ? &emitter_weights<true> : &emitter_weights<false>;
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_direct_paths(const DirectPathParams& p, bool noise, bool mis, hipStream_t stream) {
    const Shard& sh = p.shard;
    const uint64_t P = (uint64_t)sh.width * sh.rows;
    if (P == 0 || sh.kn == 0) return hipSuccess;
    if (P > 0xFFFFFFFFull || (uint64_t)sh.k0 + sh.kn > 0xFFFFFFFFull || p.tile_w_log2 > 6u || p.refill == 0 || p.refill > 64u ||
        sh.world == 0 || sh.rank >= sh.world || !p.scene.entries || !p.materials || !p.textures || !p.texels || !p.acc_s || !p.acc_q ||
        (p.n_lights && !p.lights) || p.n_lights > (1u << 24) || (mis && (!p.rank_sphere || !p.prims.tab)))
        return hipErrorInvalidValue;
    const bool fixed = trace_placement(p.scene.n_entries, p.scene.n_quads) == RTX_SCENE_IN_LDS;
    if (p.scene.n_quads)
        return fixed ? launch_paths_noise<true, true>(p, noise, mis, stream) : launch_paths_noise<true, false>(p, noise, mis, stream);
    return fixed ? launch_paths_noise<false, true>(p, noise, mis, stream) : launch_paths_noise<false, false>(p, noise, mis, stream);
}

}  // namespace rtxd
