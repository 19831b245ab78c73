// rtx_denoise_pixel.h — the preview filter's arithmetic for one pixel (include/rtx.h states it), as
// the kernels of rtx_denoise.hip run it.  It names no HIP type beyond a four-float vector, so the plain host compiler
// builds it too: tests/test_denoise_capi.py runs these very functions on the CPU against tests/denoise_ref.py.
// float32, every operation rounded on its own: both builds are made without contraction.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RTX_DN_FN __host__ __device__ __forceinline__
namespace rtxd {
using dn_f4 = float4;
RTX_DN_FN dn_f4 dn_make(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
#else
#define RTX_DN_FN inline
namespace rtxd {
struct dn_f4 {
    float x, y, z, w;
};
RTX_DN_FN dn_f4 dn_make(float x, float y, float z, float w) { return dn_f4{x, y, z, w}; }
#endif

RTX_DN_FN float dn_albedo_floor(float a) { return a > 0.01f ? a : 0.01f; }
RTX_DN_FN float dn_edge_stop(float x) {
    const float y = 1.0f - x;
    return y > 0.0f ? y : 0.0f;  // (a NaN: 0)
}

// prepare: (c, v) of pixel i.  guides: two four-float vectors per pixel, (albedo, cover) and (normal, depth).
RTX_DN_FN dn_f4 dn_prepare(const float* rgb, const float* var, const dn_f4* guides, uint64_t i) {
    const dn_f4 g = guides[2 * i];
    const float ar = dn_albedo_floor(g.x), ag = dn_albedo_floor(g.y), ab = dn_albedo_floor(g.z);
    const float* c = rgb + 3 * i;
    const float* v = var + 3 * i;
    return dn_make(c[0] / ar, c[1] / ag, c[2] / ab, (v[0] / (ar * ar) + v[1] / (ag * ag)) + v[2] / (ab * ab));
}

// One level at step s: (c', v') of pixel (x, y) from the (c, v) image `src`.  A tap outside the image is skipped, so
// every address lies inside the width * rows pixels of its array.
RTX_DN_FN dn_f4 dn_level(const dn_f4* src, const dn_f4* guides, uint32_t width, uint32_t rows, uint32_t x, uint32_t y,
                         int32_t s, float sigma_normal, float sigma_depth, float sigma_luminance) {
    const int32_t W = (int32_t)width, H = (int32_t)rows;
    const uint64_t i = (uint64_t)y * width + x;
    const dn_f4 cp = src[i];
    const dn_f4 gp = guides[2 * i + 1];  // (n, z)

    // the 3 x 3 variance sum
    float sv = 0.0f, sk = 0.0f;
#pragma unroll
    for (int32_t b = -1; b <= 1; ++b) {
#pragma unroll
        for (int32_t a = -1; a <= 1; ++a) {
            const int32_t qx = (int32_t)x + a, qy = (int32_t)y + b;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                const float k = (float)((2 - (b < 0 ? -b : b)) * (2 - (a < 0 ? -a : a)));  // k3 = (1, 2, 1)
                sv = sv + k * src[(uint64_t)qy * width + (uint32_t)qx].w;
                sk = sk + k;
            }
        }
    }
    const float vb = sv / sk;
    const float lp = (cp.x + cp.y) + cp.z;
    const float dl = (sigma_luminance * sigma_luminance) * vb + 1e-6f;
    const float sn2 = sigma_normal * sigma_normal;

    const float K5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float Wt = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, V = 0.0f;
#pragma unroll
    for (int32_t dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int32_t dx = -2; dx <= 2; ++dx) {
            const int32_t qx = (int32_t)x + s * dx, qy = (int32_t)y + s * dy;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                const uint64_t j = (uint64_t)qy * width + (uint32_t)qx;
                const dn_f4 cq = src[j];
                const dn_f4 gq = guides[2 * j + 1];
                const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
                const float xn = ((nx * nx + ny * ny) + nz * nz) / sn2;
                const int32_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                const float m = (float)(s * (ax > ay ? ax : ay));
                const float zm = gp.w > gq.w ? gp.w : gq.w;
                const float tz = (sigma_depth * m) * zm;
                const float dz = gp.w - gq.w;
                const float xz = (dz * dz) / (tz * tz + 1e-6f);
                const float d = lp - ((cq.x + cq.y) + cq.z);
                const float xl = (d * d) / dl;
                const float w = (((K5[dy + 2] * K5[dx + 2]) * dn_edge_stop(xn)) * dn_edge_stop(xz)) * dn_edge_stop(xl);
                if (w > 0.0f) {
                    Wt = Wt + w;
                    Cr = Cr + w * cq.x;
                    Cg = Cg + w * cq.y;
                    Cb = Cb + w * cq.z;
                    V = V + (w * w) * cq.w;
                }
            }
        }
    }
    return dn_make(Cr / Wt, Cg / Wt, Cb / Wt, V / (Wt * Wt));
}

// finish: the albedo multiplied back in.
RTX_DN_FN void dn_finish(const dn_f4 c, const dn_f4* guides, uint64_t i, float* out) {
    const dn_f4 al = guides[2 * i];
    out[3 * i] = c.x * dn_albedo_floor(al.x);
    out[3 * i + 1] = c.y * dn_albedo_floor(al.y);
    out[3 * i + 2] = c.z * dn_albedo_floor(al.z);
}

}  // namespace rtxd
