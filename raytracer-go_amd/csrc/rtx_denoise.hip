// rtx_denoise.hip — the preview filter (rtx_denoise_device): a variance-guided, edge-avoiding a-trous
// filter of the resolved image, steered by the first-hit guides.  include/rtx.h states the arithmetic, which is the
// contract: float32, every operation rounded on its own (the unit is built without contraction), no square root,
// no exp; rtx_denoise_pixel.h holds it per pixel, tests/denoise_ref.py restates it in numpy and the two match bit
// for bit.
//
//   denoise_prepare      (rgb, var, albedo) -> (c, v): the colour without its albedo and the summed variance, one float4
//   atrous_level<false>  (c, v) -> (c', v') at step s, read from one workspace image and written to the other
//   atrous_level<true>   the last level, which multiplies the albedo back in and writes the 3-float image
//
// The plain form: one pixel per lane, a wave on 64 consecutive pixels of a row, every tap one 16-B load from each
// of two arrays: (c, v), and (n, z), the second float4 of rtx_guide.  No LDS, no atomics, no cross-lane operation: a
// lane outside the image leaves at once.
#include "rtx_denoise_pixel.h"
#include "rtx_guides.h"
#include "rtx_launch_name.h"

namespace rtxd {
namespace {

constexpr uint32_t DN_W = 64, DN_H = 4;  // a workgroup's pixels: four waves, one 64-pixel row segment each

}  // namespace

// (The kernels: in rtxd itself, not in the unit's anonymous namespace; rtx_trace.hip, trace_rays.)
__global__ __launch_bounds__(DN_W * DN_H) void denoise_prepare(const float* __restrict__ rgb, const float* __restrict__ var,
                                                                const float4* __restrict__ guides, uint32_t width,
                                                                uint32_t rows, float4* __restrict__ cv) {
    const uint32_t x = blockIdx.x * DN_W + (threadIdx.x & (DN_W - 1u)), y = blockIdx.y * DN_H + threadIdx.x / DN_W;
    if (x >= width || y >= rows) return;
    const uint64_t i = (uint64_t)y * width + x;
    cv[i] = dn_prepare(rgb, var, guides, i);
}

template <bool LAST>
__global__ __launch_bounds__(DN_W * DN_H) void atrous_level(const float4* __restrict__ src, const float4* __restrict__ guides,
                                                             uint32_t width, uint32_t rows, uint32_t step,
                                                             rtx_denoise_params prm, float4* __restrict__ dst,
                                                             float* __restrict__ out) {
    const uint32_t x = blockIdx.x * DN_W + (threadIdx.x & (DN_W - 1u)), y = blockIdx.y * DN_H + threadIdx.x / DN_W;
    if (x >= width || y >= rows) return;
    const uint64_t i = (uint64_t)y * width + x;
    const float4 c = dn_level(src, guides, width, rows, x, y, (int32_t)step, prm.sigma_normal, prm.sigma_depth,
                              prm.sigma_luminance);
    if constexpr (LAST) dn_finish(c, guides, i, out);
    else dst[i] = c;
}

hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t stream) {
    const uint64_t P = (uint64_t)a.width * a.rows;
    if (P == 0) return hipSuccess;
    const dim3 grid((a.width + DN_W - 1) / DN_W, (a.rows + DN_H - 1) / DN_H), block(DN_W * DN_H);
    if (P > 0x7FFFFFFFull || grid.y > 65535u || a.params.iterations < 1 || a.params.iterations > 6 || !a.rgb || !a.var ||
        !a.guides || !a.out || !a.work)
        return hipErrorInvalidValue;
    static_assert(sizeof(rtx_guide) == 2 * sizeof(float4), "a guide is two float4: (albedo, cover), (normal, depth)");
    const float4* guides = reinterpret_cast<const float4*>(a.guides);
    float4* buf[2] = {a.work, a.work + P};
    name_launch(&denoise_prepare);
    hipLaunchKernelGGL(denoise_prepare, grid, block, 0, stream, a.rgb, a.var, guides, a.width, a.rows, buf[0]);
    for (uint32_t i = 0; i < a.params.iterations; ++i) {
        const float4* src = buf[i & 1u];
        name_launch(i + 1 == a.params.iterations ? &atrous_level<true> : &atrous_level<false>);
        if (i + 1 == a.params.iterations)
            hipLaunchKernelGGL(atrous_level<true>, grid, block, 0, stream, src, guides, a.width, a.rows, 1u << i, a.params,
                               (float4*)nullptr, a.out);
        else
            hipLaunchKernelGGL(atrous_level<false>, grid, block, 0, stream, src, guides, a.width, a.rows, 1u << i, a.params,
                               buf[(i + 1) & 1u], (float*)nullptr);
    }
    return hipGetLastError();
}

}  // namespace rtxd
