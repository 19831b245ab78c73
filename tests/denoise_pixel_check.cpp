// The preview filter's per-pixel arithmetic (raytracer-go_amd/csrc/rtx_denoise_pixel.h, the functions the kernels of
// rtx_denoise.hip call) run on the CPU over a whole image, in the kernels' order: prepare, the levels between two
// workspace images, finish.  tests/test_denoise_capi.py builds it with the host compiler (no contraction) and compares
// its output with tests/denoise_ref.py bit for bit.
//   denoise_pixel_check IN OUT
// IN:  uint32 width, rows, iterations; float32 sigma_normal, sigma_depth, sigma_luminance; then rgb [P * 3], var [P * 3]
//      and guides [P * 8] as float32.  OUT: the filtered image, float32 [P * 3].
#include <cstdio>
#include <vector>

#include "rtx_denoise_pixel.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[3];
    float sigma[3];
    if (std::fread(head, 4, 3, f) != 3 || std::fread(sigma, 4, 3, f) != 3) return 2;
    const uint32_t width = head[0], rows = head[1], iterations = head[2];
    const size_t P = (size_t)width * rows;
    std::vector<float> rgb(P * 3), var(P * 3), out(P * 3);
    std::vector<rtxd::dn_f4> guides(P * 2), work(P * 2);
    if (std::fread(rgb.data(), 4, P * 3, f) != P * 3 || std::fread(var.data(), 4, P * 3, f) != P * 3 ||
        std::fread(guides.data(), 16, P * 2, f) != P * 2)
        return 2;
    std::fclose(f);
    rtxd::dn_f4* buf[2] = {work.data(), work.data() + P};
    for (size_t i = 0; i < P; ++i) buf[0][i] = rtxd::dn_prepare(rgb.data(), var.data(), guides.data(), i);
    for (uint32_t l = 0; l < iterations; ++l) {
        const rtxd::dn_f4* src = buf[l & 1u];
        for (uint32_t y = 0; y < rows; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const size_t i = (size_t)y * width + x;
                const rtxd::dn_f4 c = rtxd::dn_level(src, guides.data(), width, rows, x, y, 1 << l, sigma[0], sigma[1], sigma[2]);
                if (l + 1 == iterations) rtxd::dn_finish(c, guides.data(), i, out.data());
                else buf[(l + 1) & 1u][i] = c;
            }
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, P * 3, f) != P * 3) return 2;
    std::fclose(f);
    return 0;
}
