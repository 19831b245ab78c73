// rtx_direct.h — launch interface between the C-ABI layer and the direct-light block (rtx_direct.hip):
// rtx_direct_device / rtx_direct of include/rtx.h, DESIGN.md §37.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx.h"
#include "rtx_walk.h"

namespace rtxd {
// Device counters of a counting call, in memory of the scene copy's own (never the render's, the trace's or the shade's).
constexpr uint32_t DIRECT_SAMPLED = 0u, DIRECT_VISIBLE = 1u, DIRECT_RNG_DRAWS = 2u, DIRECT_COUNTER_SLOTS = 3u;

// The light events of the Philox counter: word 2 = DIRECT_EVENT | the scatter's event.
constexpr uint32_t DIRECT_EVENT = 0x40000000u;

// One launch: records [0, n) of the three arrays, n <= DIRECT_LAUNCH_MAX (record indices are 32-bit).
constexpr uint64_t DIRECT_LAUNCH_MAX = 1ull << 30;
struct DirectParams {
    WalkScene scene;  // a trace layout
    const rtx_material* materials;  // the device forms of DeviceCopy
    const rtx_texture* textures;
    const uint32_t* texels;
    uint32_t n_materials;
    uint32_t n_lights;     // L; 0: every record is all zero
    const float4* lights;  // 4 per emitter (build_lights, rtx_scene.hip)
    uint64_t seed;
    const rtx_hit* hits;
    const rtx_path_key* keys;
    rtx_direct_sample* out;
    uint32_t n;
    uint32_t range;       // records per wave, a multiple of 64: wave w owns records [w * range, (w + 1) * range)
    uint32_t prim_batch;  // primitive tests wait for this many lanes (trav_step_batched)
    unsigned long long* counters;  // DIRECT_COUNTER_SLOTS, the counting instantiation
};
// Enqueue one launch on `stream`.  count: the counting instantiation (adds to p.counters); noise: the scene has a
// Perlin texture.
hipError_t launch_direct(const DirectParams& p, bool count, bool noise, hipStream_t stream);

// The per-primitive lookup of rtx_prim_lights on the device (build_lights, rtx_scene.hip): (area, light index) of the
// caller's sphere k at [k], k < n_spheres, and of its quad k at [n_spheres + k], k < n_quads.
struct PrimLights {
    const float2* tab;
    uint32_t n_spheres, n_quads;
};

// One launch of the fused pass (rtx_accum_add_direct, direct_paths): samples [k0, k0 + kn) of the region's
// width * rows pixels (at most 2^32 - 1) by the estimator of DESIGN.md §37, folded into the accumulator's tile-major
// moments acc_s and acc_q (slot = tile * 64 + lane, 3 floats each; rtx_kernel.hip accumulate_samples' layout).
struct DirectPathParams {
    Shard shard;
    WalkScene scene;        // a trace layout
    uint32_t tile_w_log2;   // the accumulator's tiles: 2^tile_w_log2 wide, 64 pixels
    uint32_t refill;        // parked lanes with work at which a wave runs its fold step (1..64)
    uint32_t prim_batch;    // primitive tests wait for this many lanes (trav_step_batched)
    uint32_t want_uv;       // the scene has an image texture: sphere hits need (u, v)
    const rtx_material* materials;
    const rtx_texture* textures;
    const uint32_t* texels;
    uint32_t n_materials;
    uint32_t n_lights;
    const float4* lights;
    float* acc_s;
    float* acc_q;
    // the MIS instantiations alone (rtx_accum_add_mis)
    const uint32_t* rank_sphere;  // rank word of a sphere entry -> the caller's sphere index (rtx_trace.h)
    PrimLights prims;
};
// Enqueue one launch on `stream`.  noise: the scene has a Perlin texture.  mis: the estimator of rtx_accum_add_mis.
hipError_t launch_direct_paths(const DirectPathParams& p, bool noise, bool mis, hipStream_t stream);

// One launch of the emitter-weight block (rtx_emitter_weight_device, emitter_weights): records [0, n) of the three
// arrays, n <= DIRECT_LAUNCH_MAX.
constexpr uint32_t EMITTER_WEIGHTED = 0u;  // its counter's slot (the direct block's Probe)
struct EmitterWeightParams {
    const rtx_material* materials;
    uint32_t n_materials;
    uint32_t n_lights;  // L
    PrimLights prims;
    const rtx_hit* from;
    const rtx_hit* hits;
    rtx_emitter_weight_record* out;
    uint32_t n;
    unsigned long long* counters;  // the counting instantiation
};
hipError_t launch_emitter_weights(const EmitterWeightParams& p, bool count, hipStream_t stream);
}  // namespace rtxd
