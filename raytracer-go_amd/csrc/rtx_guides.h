// rtx_guides.h — launch interfaces between the C-ABI layer and the preview kernels: the first-hit guide images
// (rtx_guides.hip) and the edge-avoiding filter (rtx_denoise.hip); rtx_guides* and rtx_denoise* of include/rtx.h,
// DESIGN.md §35.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx.h"

namespace rtxd {
// One launch: the guides of the region's width * rows pixels (at most 2^32 - 1) over samples [k0, k0 + kn), kn >= 1.
struct GuideParams {
    rtx_camera cam;
    uint64_t seed;
    uint32_t x0, y0, width, rows, rank, world, stripe_log2;
    uint32_t k0, kn;
    uint32_t tile_w_log2;   // a wave's 64 pixels: 2^tile_w_log2 wide (3: 8 x 8, 6: 64 x 1)
    const float4* entries;  // a trace layout (rtx_layout.h), as TraceParams'
    uint32_t n_entries;
    uint32_t n_quads;
    uint32_t start;
    uint32_t prim_end;
    uint32_t refill;        // folded-and-waiting lanes at which a wave folds and hands out the next samples (1..64)
    uint32_t prim_batch;    // primitive tests wait for this many lanes (trav_step_batched)
    uint32_t want_uv;       // the scene has an image texture: sphere hits need (u, v)
    const rtx_material* materials;  // the device forms of DeviceCopy, as ShadeParams'
    const rtx_texture* textures;
    const uint32_t* texels;
    rtx_guide* out;
};
// Enqueue one launch on `stream`.  noise: the scene has a Perlin texture.
hipError_t launch_guides(const GuideParams& p, bool noise, hipStream_t stream);

// The filter of rtx_denoise_device: iterations + 1 launches on `stream`.  work: two float4 images.
struct DenoiseArgs {
    const float* rgb;
    const float* var;
    const rtx_guide* guides;
    uint32_t width, rows;
    rtx_denoise_params params;
    float* out;
    float4* work;
};
hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t stream);
}  // namespace rtxd
