// rtx_walk.h — what the kernels that walk a trace layout share (trace_rays, guide_images, direct_lights,
// direct_paths): the scene and shard parameters, the LDS staging prologue, NewHitInfo of a finished
// walk, the batched steps between two votes, and a wave's tile of pixels.  The megakernel (rtx_kernel.hip) keeps its
// own prologue and shade(): its layout also holds materials and textures, and its code object must not move.
//
// Everything here is inlined into its caller.  Every piece that votes (stage_scene's barrier, hit_record's unit(),
// walk_steps' ballots and those of the batched step) is called where the whole wave arrives; what a lane keeps of
// the result is the caller's select.
#pragma once
#include "rtx_device.h"

namespace rtxd {

// Waves per workgroup (one LDS copy of the scene each) and walk steps between two votes on the parked lanes, of
// all four kernels.
constexpr int WALK_WAVES = 8;
constexpr uint32_t WALK_STEPS = 4;

// A trace layout on the device (rtx_layout.h): n_entries + 1 'a' halves, as many 'b', 4 float4 per quad.
struct WalkScene {
    const float4* entries;
    uint32_t n_entries;
    uint32_t n_quads;
    uint32_t start;     // walk position of the root
    uint32_t prim_end;  // scene in the LDS copy: its primitives are stored below this position
};

// A region's shard and a range of samples: what a camera ray of the render is made from.
struct Shard {
    rtx_camera cam;
    uint64_t seed;
    uint32_t x0, y0, width, rows, rank, world, stripe_log2;
    uint32_t k0, kn;  // samples [k0, k0 + kn)
};

// LDS bytes of the fixed layout without materials (scene_ref_fixed with none): the 'a' halves from byte 0, the 'b'
// halves from LDS_B, then the quad table.
__host__ __device__ inline uint32_t walk_lds_bytes(uint32_t n_entries, uint32_t n_quads) {
    return LDS_B + (n_entries + 1) * 16 + n_quads * 64;
}

// The position of the end sentinel.
__device__ __forceinline__ uint32_t walk_end(const WalkScene& w) { return 16 * w.n_entries; }

// The kernel's prologue, by the whole workgroup of WAVES waves.  FIXED: the layout copied into `lds` (the
// workgroup's dynamic LDS, walk_lds_bytes of it), else read from HBM.
template <int WAVES, bool FIXED>
__device__ __forceinline__ SceneRef stage_scene(float4* lds, const WalkScene& w) {
    if constexpr (FIXED) {
        // scene_ref_fixed: the walk addresses LDS directly, so the copy must start at 0
        if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)lds != 0u) __builtin_trap();
        const uint32_t m = w.n_entries + 1, nq4 = 4 * w.n_quads;
        for (uint32_t i = threadIdx.x; i < m; i += 64 * WAVES) {
            lds[i] = w.entries[i];
            lds[LDS_B / 16 + i] = w.entries[m + i];
        }
        for (uint32_t i = threadIdx.x; i < nq4; i += 64 * WAVES) lds[LDS_B / 16 + m + i] = w.entries[2 * m + i];
        __syncthreads();
        SceneRef E = scene_ref_fixed(lds, w.n_entries, w.n_quads, 0u, 0u);
        E.prim_end = w.prim_end;
        return E;
    } else {
        return scene_ref(w.entries, w.n_entries, nullptr);
    }
}

// NewHitInfo (hittables.go:22-37) of a lane's finished walk, of what Sphere.Hit (:118-129) or Quad.Hit (:180-190)
// hand it, as shade() forms them (rtx_device.h).  Computed by every lane (unit's votes); a miss reads entry 0 and
// the caller drops the rest.  PRIM (trace_rays): also rtx_hit's prim word, a sphere's through rank_sphere; formed in
// the primitive's own branch, where write_hit formed it (after the call, from the entry's 'b' half, the QUADS
// instantiations of trace_rays took up to 2 more VGPRs).  The body keeps locals and one aggregate return for the
// same reason.
struct HitRecord {
    bool hit, front, quad;
    uint32_t mi, prim;  // prim: RTX_HIT_NONE unless PRIM and hit
    V3 pt, n;
    float u, v;
};
template <bool QUADS, bool PRIM = false>
__device__ __forceinline__ HitRecord hit_record(const SceneRef E, const Trav& t, const Ray& r, const bool want_uv,
                                                const uint32_t* rank_sphere = nullptr) {
    const bool hit = t.hit >= 0;
    const uint32_t e = hit ? (uint32_t)t.hit : 0u;
    const float4 sa = E.a[e];
    const float4 sb = E.b[e];
    const bool quad = QUADS && hit && __float_as_int(sb.w) == RTX_E_QUAD;
    const V3 pt = add(scale(r.d, t.closest), r.o);                                // ray.go:25-30
    V3 n = unit(scale(sub(pt, v3(sa.x, sa.y, sa.z)), sa.w));                      // hittables.go:119-120
    uint32_t prim = 0xFFFFFFFFu, mi = 0u;
    float u = 0.0f, v = 0.0f;
    if (quad) {
        const uint32_t qk = (uint32_t)__float_as_int(sb.x), qi = 4u * qk;
        const float4 q0 = E.q[qi];
        mi = (uint32_t)__float_as_int(q0.w);
        n = v3(sa.x, sa.y, sa.z);                                                 // q.normal
        if (PRIM) prim = (RTX_PRIM_QUAD << 28) | qk;
        if (want_uv) {  // (alpha, beta) as quad_test formed them (hittables.go:181-183)
            const float4 q1 = E.q[qi + 1], q2 = E.q[qi + 2], q3 = E.q[qi + 3];
            const V3 php = sub(pt, v3(q0.x, q0.y, q0.z));
            const V3 w = v3(q3.x, q3.y, q3.z);
            u = dot(w, cross(php, v3(q2.x, q2.y, q2.z)));
            v = dot(w, cross(v3(q1.x, q1.y, q1.z), php));
        }
    } else if (hit) {
        mi = RTX_DEV_SPHERE_MATERIAL(__float_as_int(sb.w));
        if (PRIM) prim = (RTX_PRIM_SPHERE << 28) | rank_sphere[__float_as_uint(sb.y)];
        if (want_uv) {                                                            // hittables.go:122-126
            const UV uv = sphere_uv(n.x, n.y, n.z);
            u = uv.u;
            v = uv.v;
        }
    }
    const bool front = dot(r.d, n) < 0.0f;                                        // hittables.go:23
    if (!front) n = scale(n, -1.0f);                                              // :24-26
    return HitRecord{hit, front, quad, mi, prim, pt, n, u, v};
}

// STEPS walk steps of the batched step between two votes: the med3 / div_by forms when every walking lane's ray is
// safe (traverse_phase).  park_on_hit: any-hit, the lane parks at its first accepted primitive.  The walk goes in and
// out by value: through a reference the HBM instantiations of guide_images and trace_rays took 5 to 8 more VGPRs.
template <uint32_t STEPS, bool COUNT, bool QUADS, bool FIXED>
__device__ __forceinline__ Trav walk_steps(Trav t, const Ray& r, const SceneRef E, Counters& cnt, const uint32_t end,
                                           const uint32_t prim_batch, const float tmin, const bool park_on_hit) {
    uint32_t idle = 0;
    if (ballot(!t.safe && t.i < end) == 0) {
#pragma unroll
        for (uint32_t s = 0; s < STEPS; ++s) {
            trav_step_batched<COUNT, QUADS, FIXED, false, true>(t, r, E, cnt, end, prim_batch, idle, V3{0.0f, 0.0f, 0.0f}, tmin);
            if (park_on_hit && t.hit >= 0) t.i = end;
        }
    } else {
#pragma unroll
        for (uint32_t s = 0; s < STEPS; ++s) {
            trav_step_batched<COUNT, QUADS, FIXED, false, false>(t, r, E, cnt, end, prim_batch, idle, V3{0.0f, 0.0f, 0.0f}, tmin);
            if (park_on_hit && t.hit >= 0) t.i = end;
        }
    }
    return t;
}

// Lane `lane` of wave `wave` in the shard's tiles of 64 pixels, 2^twl wide: its pixel.  A lane past the shard's edge
// (!live) computes on the nearest pixel of the shard and stores nothing.
struct TilePixel {
    bool live;
    uint32_t xx, lr;  // in the shard
    uint32_t x, y;    // in the image
    uint32_t pixel;   // the GLOBAL pixel index: the RNG's counter word
    V3 base;          // pixel_base
};
__device__ __forceinline__ TilePixel tile_pixel(const Shard& s, const uint32_t twl, const uint32_t wave, const uint32_t lane) {
    const uint32_t tw = 1u << twl, th = 64u >> twl;
    const uint32_t tiles_x = tiles_x_of(s.width, twl);
    const uint32_t tile_y = wave / tiles_x, tile_x = wave - tile_y * tiles_x;
    const uint32_t px = tile_x * tw + (lane & (tw - 1u)), py = tile_y * th + (lane >> twl);
    TilePixel t;
    t.live = px < s.width && py < s.rows;
    t.xx = px < s.width ? px : s.width - 1u;
    t.lr = py < s.rows ? py : s.rows - 1u;
    t.x = s.x0 + t.xx;
    t.y = s.y0 + region_row(t.lr, s.rank, s.world, s.stripe_log2);
    t.pixel = t.y * s.cam.image_width + t.x;
    t.base = pixel_base(s.cam, t.x, t.y);
    return t;
}

}  // namespace rtxd
