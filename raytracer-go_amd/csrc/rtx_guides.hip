// rtx_guides.hip — first-hit guide images (rtx_guides_device): per pixel, the mean over a range of
// samples of the albedo, normal and depth at the first hit of the render's own camera ray.
//
// The kernel is trace_rays' loop (rtx_trace.hip) with the hand-off turned inward, on the same pieces (rtx_walk.h).  One lane owns one pixel and
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

#include "rtx_launch_name.h"
#include "rtx_trace.h"
#include "rtx_walk.h"

namespace rtxd {
namespace {

struct FirstHit {
    V3 a, n;
    float t;
    bool hit;
};

// What sample k adds for a lane's finished walk, computed by every lane (unit's votes): hit_record (rtx_walk.h), then
// the material's colour as shade_hits reads it (rtx_shade.hip).
template <bool QUADS, bool NOISE>
__device__ __forceinline__ FirstHit first_hit(const GuideParams& p, const SceneRef E, const Trav& t, const Ray& r) {
    const HitRecord h = hit_record<QUADS>(E, t, r, p.want_uv != 0u);
    V3 a = v3(1.0f, 1.0f, 1.0f);  // a miss, a Dielectric, a DiffuseLight
    if (h.hit) {
        const float4* mp = reinterpret_cast<const float4*>(p.materials + h.mi);
        const float4 m0 = mp[0], m1 = mp[1];
        const uint32_t type = __float_as_uint(m0.x), tex = __float_as_uint(m0.y);
        const V3 albedo = v3(m1.x, m1.y, m1.z);
        Counters cnt{0, 0, 0, 0, 0, 0, 0};
        if (type == RTX_MAT_METAL) a = albedo;
        else if (type == RTX_MAT_LAMBERTIAN)  // (RTX_DEV_TEX_INLINE: a SolidColor, the colour in albedo)
            a = tex == RTX_DEV_TEX_INLINE ? albedo : texture_value<false, NOISE>(p.textures, p.texels, tex, h.u, h.v, h.pt, cnt);
    }
    return FirstHit{a, h.hit ? h.n : v3(0.0f, 0.0f, 0.0f), t.closest, h.hit};
}

}  // namespace

// QUADS: the scene holds quads.  FIXED: the scene in the workgroup's LDS copy (scene_ref_fixed), else read from
// HBM.  NOISE: the scene has a Perlin texture.
// (In rtxd itself, not in the unit's anonymous namespace: rtx_trace.hip, trace_rays.)
template <bool QUADS, bool FIXED, bool NOISE>
__global__ __launch_bounds__(64 * WALK_WAVES) void guide_images(GuideParams p) {
    extern __shared__ float4 lds_entries[];
    const SceneRef E = stage_scene<WALK_WAVES, FIXED>(lds_entries, p.scene);
    const uint32_t end = walk_end(p.scene);
    const Shard& sh = p.shard;
    const uint32_t twl = p.tile_w_log2;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WALK_WAVES + (threadIdx.x >> 6));
    if (wave >= tiles_x_of(sh.width, twl) * tiles_y_of(sh.rows, twl)) return;  // (the whole wave)
    const TilePixel tp = tile_pixel(sh, twl, wave, threadIdx.x & 63u);
    const uint32_t pixel = tp.pixel;
    const V3 base = tp.base;
    const uint32_t s0 = (uint32_t)sh.seed, s1 = (uint32_t)(sh.seed >> 32);

    uint32_t k = sh.k0;                    // the lane's sample: walking it, or parked on its end
    const uint32_t kend = sh.k0 + sh.kn;   // (at most 2^32 - 1: the entry's check)
    uint32_t draws = 0;
    Ray r;
    {
        const PathRng rng{s0, s1, pixel, k};
        r = camera_ray<false>(sh.cam, base, rng, rng.block(0, 0), draws);
    }
    Trav t{};
    trav_begin(t, r, p.scene.start);
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
            const Ray nr = camera_ray<false>(sh.cam, base, rng, rng.block(0, 0), draws);
            Trav nt;
            trav_begin(nt, nr, p.scene.start);
            if (pend && k < kend) {
                r = nr;
                t = nt;
            }  // (else walking on, or out of samples: it stays on the sentinel)
        }
        t = walk_steps<WALK_STEPS, false, QUADS, FIXED>(t, r, E, cnt, end, p.prim_batch, 0.001f, false);
    }
    if (tp.live) {  // 32 B: two dwordx4 stores
        const float inv = 1.0f / (float)sh.kn;
        float4* o = reinterpret_cast<float4*>(p.out + ((uint64_t)tp.lr * sh.width + tp.xx));
        o[0] = make_float4(A.x * inv, A.y * inv, A.z * inv, (float)c * inv);
        o[1] = make_float4(N.x * inv, N.y * inv, N.z * inv, c ? Z / (float)c : 0.0f);
    }
}

namespace {

template <bool QUADS, bool FIXED>
hipError_t launch_noise(const GuideParams& p, bool noise, hipStream_t stream) {
    const size_t shmem = FIXED ? walk_lds_bytes(p.scene.n_entries, p.scene.n_quads) : 0;
    const uint64_t tiles = (uint64_t)tiles_x_of(p.shard.width, p.tile_w_log2) * tiles_y_of(p.shard.rows, p.tile_w_log2);
    const dim3 grid((uint32_t)((tiles + WALK_WAVES - 1) / WALK_WAVES)), block(64 * WALK_WAVES);
    const auto kern = noise ? &guide_images<QUADS, FIXED, true> : &guide_images<QUADS, FIXED, false>;
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, shmem, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_guides(const GuideParams& p, bool noise, hipStream_t stream) {
    const Shard& sh = p.shard;
    const uint64_t P = (uint64_t)sh.width * sh.rows;
    if (P == 0) return hipSuccess;
    if (P > 0xFFFFFFFFull || sh.kn == 0 || (uint64_t)sh.k0 + sh.kn > 0xFFFFFFFFull || p.tile_w_log2 > 6u || p.refill == 0 ||
        p.refill > 64u || sh.world == 0 || sh.rank >= sh.world || !p.scene.entries || !p.materials || !p.textures || !p.texels ||
        !p.out)
        return hipErrorInvalidValue;
    const bool fixed = trace_placement(p.scene.n_entries, p.scene.n_quads) == RTX_SCENE_IN_LDS;
    if (p.scene.n_quads) return fixed ? launch_noise<true, true>(p, noise, stream) : launch_noise<true, false>(p, noise, stream);
    return fixed ? launch_noise<false, true>(p, noise, stream) : launch_noise<false, false>(p, noise, stream);
}

}  // namespace rtxd
