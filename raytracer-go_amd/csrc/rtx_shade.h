// rtx_shade.h — launch interface between the C-ABI layer and the path building blocks (rtx_shade.hip):
// rtx_camera_rays* and rtx_shade* of include/rtx.h, DESIGN.md §34.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx.h"
#include "rtx_walk.h"

namespace rtxd {
// Device counters of a counting shade, in memory of the scene copy's own (never the render's or the trace's).
constexpr uint32_t SHADE_HITS = 0u, SHADE_SCATTERED = 1u, SHADE_RNG_DRAWS = 2u, SHADE_TEXEL_FETCHES = 3u,
                   SHADE_COUNTER_SLOTS = 4u;

// One launch: records [0, n) of the four arrays, n <= SHADE_LAUNCH_MAX (record indices are 32-bit).
constexpr uint64_t SHADE_LAUNCH_MAX = 1ull << 30;
struct ShadeParams {
    const rtx_material* materials;  // the device forms of DeviceCopy (RTX_DEV_TEX_INLINE, 1/ior and r0s in albedo)
    const rtx_texture* textures;    // the renumbered device textures (a checker's 1/scale in pad)
    const uint32_t* texels;
    uint32_t n_materials;
    uint32_t n;
    uint64_t seed;
    const rtx_ray* rays;
    const rtx_hit* hits;
    const rtx_path_key* keys;
    rtx_bounce* out;
    unsigned long long* counters;  // SHADE_COUNTER_SLOTS, the counting instantiation
};
// Enqueue one launch on `stream`.  count: the counting instantiation (adds to p.counters); noise: the scene has a
// Perlin texture (the instantiation that contains its out-of-line evaluation).
hipError_t launch_shade(const ShadeParams& p, bool count, bool noise, hipStream_t stream);

// One launch: samples [k0, k0 + kn) of the region's P = width * rows pixels, kn <= CAMERA_LAUNCH_SAMPLES (the grid's
// second dimension); record (k - k0) * P + i * width + xx goes to rays[...] (and keys[...] when keys != nullptr).
constexpr uint32_t CAMERA_LAUNCH_SAMPLES = 65535u;
struct CameraRayParams {
    Shard shard;
    rtx_ray* rays;
    rtx_path_key* keys;
};
hipError_t launch_camera_rays(const CameraRayParams& p, hipStream_t stream);
}  // namespace rtxd
