// coop_scatter (csrc/rtx_device.h) against the scalar loop it replaces, one 64-lane wave per case.
//
//   coop_scatter_check <input> : the input is text, "seed n_cases" and then 64 lines "type pixel sample event" per
//   case (type -1: the lane has no hit; else the material type of its hit).  The scene stub has one material per
//   type, and entry i is a sphere of material i, so a lane's hit is its type.
// Kernel 1 calls coop_scatter with the whole wave; kernel 2 lets every lane run rand_unit_on_sphere on its own
// counter (pixel, sample, event).  The two must agree bit for bit in (x, y, z, attempt, u0); every lane is printed
// ("case lane type x y z att u0", the floats as their bits), mismatches are marked and make the exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracer-go_amd/csrc/rtx_device.h"

using namespace rtxd;

struct LaneIn {
    int32_t type;
    uint32_t pixel, sample, e;
};
struct LaneOut {
    uint32_t x, y, z, att, u0;
};
static const uint32_t NO_ATT = 0xFFFFFFFFu;  // the lane drew no unit-sphere sample

__device__ SceneRef stub_scene(const float4* eb, const rtx_material* mats) {
    return SceneRef{eb, eb, nullptr, mats, nullptr, nullptr, nullptr, 0u, 0u};
}
__device__ LaneOut lane_out(V3 s, uint32_t draws, uint32_t u0) {
    return LaneOut{__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z), draws ? draws / 3u - 1u : NO_ATT, u0};
}

__global__ void __launch_bounds__(64) k_coop(Params p, const float4* eb, const rtx_material* mats, const LaneIn* in,
                                              LaneOut* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const LaneIn li = in[i];
    const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), li.pixel, li.sample};
    const Scatter sc = coop_scatter<false>(p, stub_scene(eb, mats), rng, li.e, li.type);
    out[i] = lane_out(sc.s, sc.draws, sc.u0);
}

__global__ void __launch_bounds__(64) k_scalar(Params p, const rtx_material* mats, const LaneIn* in, LaneOut* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const LaneIn li = in[i];
    const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), li.pixel, li.sample};
    V3 s = v3(0.0f, 0.0f, 0.0f);
    uint32_t draws = 0, u0 = 0;
    if (li.type >= 0) {
        const U4 b0 = rng.block(li.e, 0u);
        u0 = b0.x;
        if (mats[li.type].type < 2u) s = rand_unit_on_sphere(rng, li.e, b0, draws);
    }
    out[i] = lane_out(s, draws, u0);
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
            return 2;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long seed;
    unsigned n_cases;
    if (std::fscanf(f, "%llu %u", &seed, &n_cases) != 2 || n_cases == 0 || n_cases > 64) return 2;
    std::vector<LaneIn> in(64u * n_cases);
    for (LaneIn& li : in) {
        if (std::fscanf(f, "%d %u %u %u", &li.type, &li.pixel, &li.sample, &li.e) != 4) return 2;
        if (li.type < -1 || li.type > 3) return 2;
    }
    std::fclose(f);

    rtx_material mats[4];
    float4 eb[4];
    std::memset(mats, 0, sizeof mats);
    for (int i = 0; i < 4; ++i) {
        mats[i].type = (uint32_t)i;
        const int tag = -3 - i;  // RTX_DEV_SPHERE_MATERIAL(tag) == i
        eb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        std::memcpy(&eb[i].w, &tag, 4);
    }
    Params p;
    std::memset(&p, 0, sizeof p);
    p.seed = seed;

    const size_t nb_in = in.size() * sizeof(LaneIn), nb_out = in.size() * sizeof(LaneOut);
    float4* d_eb;
    rtx_material* d_m;
    LaneIn* d_in;
    LaneOut *d_a, *d_b;
    CHECK(hipMalloc(&d_eb, sizeof eb));
    CHECK(hipMalloc(&d_m, sizeof mats));
    CHECK(hipMalloc(&d_in, nb_in));
    CHECK(hipMalloc(&d_a, nb_out));
    CHECK(hipMalloc(&d_b, nb_out));
    CHECK(hipMemcpy(d_eb, eb, sizeof eb, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_m, mats, sizeof mats, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_in, in.data(), nb_in, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_a, 0xEE, nb_out));
    CHECK(hipMemset(d_b, 0xDD, nb_out));
    hipLaunchKernelGGL(k_coop, dim3(n_cases), dim3(64), 0, 0, p, d_eb, d_m, d_in, d_a);
    CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_scalar, dim3(n_cases), dim3(64), 0, 0, p, d_m, d_in, d_b);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<LaneOut> a(in.size()), b(in.size());
    CHECK(hipMemcpy(a.data(), d_a, nb_out, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), d_b, nb_out, hipMemcpyDeviceToHost));

    unsigned bad = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        const bool same = std::memcmp(&a[i], &b[i], sizeof(LaneOut)) == 0;
        bad += !same;
        std::printf("%zu %zu %d %08x %08x %08x %d %08x%s\n", i / 64, i % 64, in[i].type, a[i].x, a[i].y, a[i].z,
                    (int)a[i].att, a[i].u0, same ? "" : " MISMATCH");
        if (!same)
            std::printf("#   scalar loop: %08x %08x %08x %d %08x\n", b[i].x, b[i].y, b[i].z, (int)b[i].att, b[i].u0);
    }
    std::printf("mismatches %u\n", bad);
    return bad ? 1 : 0;
}
