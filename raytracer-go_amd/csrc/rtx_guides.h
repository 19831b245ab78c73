// rtx_guides.h — launch interfaces between the C-ABI layer and the preview kernels: the first-hit guide images
// (rtx_guides.hip) and the edge-avoiding filter (rtx_denoise.hip); rtx_guides* and rtx_denoise* of include/rtx.h,
// DESIGN.md §35.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx.h"
#include "rtx_walk.h"

namespace rtxd {
// One launch: the guides of the region's width * rows pixels (at most 2^32 - 1) over samples [k0, k0 + kn), kn >= 1.
struct GuideParams {
    Shard shard;
    WalkScene scene;        // a trace layout
    uint32_t tile_w_log2;   // a wave's 64 pixels: 2^tile_w_log2 wide (3: 8 x 8, 6: 64 x 1)
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
