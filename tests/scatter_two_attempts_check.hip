// coop_scatter's two own attempts and the two-block Philox (csrc/rtx_device.h), one 64-lane wave per
// case, against the scalar forms they replace.
//
//   scatter_two_attempts_check scatter <input> : text, "seed n_cases", then per case a line "quads" (0 / 1: the
//   coop_scatter instantiation) and 64 lines "hit pixel sample event".  hit -1: the lane has no hit; 0..3: a sphere of
//   that material type; 4: a quad of a Lambertian material (QUADS cases only).  The scene stub has one material per
//   type; entry i < 4 is a sphere of material i, entry 4 is quad 0, whose material is 0.
//   Kernel 1 calls coop_scatter with the whole wave; kernel 2 lets every lane run rand_unit_on_sphere on its own
//   counter.  The two must agree bit for bit in (x, y, z, attempt, u0, draws); every lane is printed ("case lane hit
//   x y z att u0 draws", the floats as their bits), mismatches are marked and make the exit status 1.
//
//   scatter_two_attempts_check philox <input> : text, "n_blocks", then per block "k0 k1" and 64 lines
//   "c0 c1 c2 c3 c3b".  One wave per block (the key is wave-uniform, as in the render): philox4x32_10_x2 on the two
//   counters against two calls of philox4x32_10; every lane is printed ("block lane a.x a.y a.z a.w b.x b.y b.z b.w",
//   the x2 words), mismatches are marked and make the exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracer-go_amd/csrc/rtx_device.h"

using namespace rtxd;

struct LaneIn {
    int32_t hit;
    uint32_t pixel, sample, e;
};
struct LaneOut {
    uint32_t x, y, z, att, u0, draws;
};
static const uint32_t NO_ATT = 0xFFFFFFFFu;  // the lane drew no unit-sphere sample
static const int N_ENTRIES = 5, QUAD_ENTRY = 4;

__device__ SceneRef stub_scene(const float4* eb, const float4* q, const rtx_material* mats) {
    return SceneRef{eb, eb, q, mats, nullptr, nullptr, nullptr, 0u, 0u};
}
__device__ LaneOut lane_out(V3 s, uint32_t draws, uint32_t u0) {
    return LaneOut{__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z),
                   draws ? draws / 3u - 1u : NO_ATT, u0, draws};
}

template <bool QUADS>
__global__ void __launch_bounds__(64) k_coop(Params p, const float4* eb, const float4* q, const rtx_material* mats,
                                              const LaneIn* in, LaneOut* out) {
    const uint32_t i = threadIdx.x;
    const LaneIn li = in[i];
    const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), li.pixel, li.sample};
    const Scatter sc = coop_scatter<QUADS>(p, stub_scene(eb, q, mats), rng, li.e, li.hit);
    out[i] = lane_out(sc.s, sc.draws, sc.u0);
}

__global__ void __launch_bounds__(64) k_scalar(Params p, const rtx_material* mats, const LaneIn* in, LaneOut* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const LaneIn li = in[i];
    const PathRng rng{(uint32_t)p.seed, (uint32_t)(p.seed >> 32), li.pixel, li.sample};
    V3 s = v3(0.0f, 0.0f, 0.0f);
    uint32_t draws = 0, u0 = 0;
    if (li.hit >= 0) {
        const U4 b0 = rng.block(li.e, 0u);
        u0 = b0.x;
        const uint32_t mi = li.hit == QUAD_ENTRY ? 0u : (uint32_t)li.hit;
        if (mats[mi].type < 2u) s = rand_unit_on_sphere(rng, li.e, b0, draws);
    }
    out[i] = lane_out(s, draws, u0);
}

struct CtrIn {
    uint32_t c0, c1, c2, c3, c3b;
};
struct U4Pair {
    U4 a, b;
};
__global__ void __launch_bounds__(64) k_philox(const uint32_t* keys, const CtrIn* in, U4Pair* x2, U4Pair* ref) {
    const uint32_t k0 = keys[2u * blockIdx.x], k1 = keys[2u * blockIdx.x + 1u];  // wave-uniform
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const CtrIn c = in[i];
    const U4x2 r = philox4x32_10_x2(c.c0, c.c1, c.c2, c.c3, c.c3b, k0, k1);
    x2[i] = U4Pair{r.a, r.b};
    ref[i] = U4Pair{philox4x32_10(c.c0, c.c1, c.c2, c.c3, k0, k1), philox4x32_10(c.c0, c.c1, c.c2, c.c3b, k0, k1)};
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
            return 2;                                                            \
        }                                                                        \
    } while (0)

static int run_scatter(FILE* f) {
    unsigned long long seed;
    unsigned n_cases;
    if (std::fscanf(f, "%llu %u", &seed, &n_cases) != 2 || n_cases == 0 || n_cases > 64) return 2;
    std::vector<LaneIn> in(64u * n_cases);
    std::vector<int> quads(n_cases);
    for (unsigned c = 0; c < n_cases; ++c) {
        if (std::fscanf(f, "%d", &quads[c]) != 1 || quads[c] < 0 || quads[c] > 1) return 2;
        for (unsigned l = 0; l < 64; ++l) {
            LaneIn& li = in[64u * c + l];
            if (std::fscanf(f, "%d %u %u %u", &li.hit, &li.pixel, &li.sample, &li.e) != 4) return 2;
            // a hit indexes the stub's entries: nothing else is read
            if (li.hit < -1 || li.hit >= N_ENTRIES || (li.hit == QUAD_ENTRY && !quads[c])) return 2;
        }
    }

    rtx_material mats[4];
    float4 eb[N_ENTRIES], q[4];
    std::memset(mats, 0, sizeof mats);
    std::memset(q, 0, sizeof q);
    for (int i = 0; i < 4; ++i) {
        mats[i].type = (uint32_t)i;
        const int tag = -3 - i;  // RTX_DEV_SPHERE_MATERIAL(tag) == i
        eb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        std::memcpy(&eb[i].w, &tag, 4);
    }
    const int quad_tag = RTX_E_QUAD, quad_index = 0, quad_material = 0;
    eb[QUAD_ENTRY] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    std::memcpy(&eb[QUAD_ENTRY].x, &quad_index, 4);
    std::memcpy(&eb[QUAD_ENTRY].w, &quad_tag, 4);
    std::memcpy(&q[0].w, &quad_material, 4);
    Params p;
    std::memset(&p, 0, sizeof p);
    p.seed = seed;

    const size_t nb_in = in.size() * sizeof(LaneIn), nb_out = in.size() * sizeof(LaneOut);
    float4 *d_eb, *d_q;
    rtx_material* d_m;
    LaneIn* d_in;
    LaneOut *d_a, *d_b;
    CHECK(hipMalloc(&d_eb, sizeof eb));
    CHECK(hipMalloc(&d_q, sizeof q));
    CHECK(hipMalloc(&d_m, sizeof mats));
    CHECK(hipMalloc(&d_in, nb_in));
    CHECK(hipMalloc(&d_a, nb_out));
    CHECK(hipMalloc(&d_b, nb_out));
    CHECK(hipMemcpy(d_eb, eb, sizeof eb, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_q, q, sizeof q, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_m, mats, sizeof mats, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_in, in.data(), nb_in, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_a, 0xEE, nb_out));
    CHECK(hipMemset(d_b, 0xDD, nb_out));
    for (unsigned c = 0; c < n_cases; ++c) {  // one wave per case
        if (quads[c])
            hipLaunchKernelGGL(k_coop<true>, dim3(1), dim3(64), 0, 0, p, d_eb, d_q, d_m, d_in + 64u * c, d_a + 64u * c);
        else
            hipLaunchKernelGGL(k_coop<false>, dim3(1), dim3(64), 0, 0, p, d_eb, d_q, d_m, d_in + 64u * c, d_a + 64u * c);
        CHECK(hipGetLastError());
    }
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
        std::printf("%zu %zu %d %08x %08x %08x %d %08x %u%s\n", i / 64, i % 64, in[i].hit, a[i].x, a[i].y, a[i].z,
                    (int)a[i].att, a[i].u0, a[i].draws, same ? "" : " MISMATCH");
        if (!same)
            std::printf("#   scalar loop: %08x %08x %08x %d %08x %u\n", b[i].x, b[i].y, b[i].z, (int)b[i].att, b[i].u0,
                        b[i].draws);
    }
    std::printf("mismatches %u\n", bad);
    return bad ? 1 : 0;
}

static int run_philox(FILE* f) {
    unsigned n_blocks;
    if (std::fscanf(f, "%u", &n_blocks) != 1 || n_blocks == 0 || n_blocks > 64) return 2;
    std::vector<uint32_t> keys(2u * n_blocks);
    std::vector<CtrIn> in(64u * n_blocks);
    for (unsigned b = 0; b < n_blocks; ++b) {
        if (std::fscanf(f, "%u %u", &keys[2u * b], &keys[2u * b + 1u]) != 2) return 2;
        for (unsigned l = 0; l < 64; ++l) {
            CtrIn& c = in[64u * b + l];
            if (std::fscanf(f, "%u %u %u %u %u", &c.c0, &c.c1, &c.c2, &c.c3, &c.c3b) != 5) return 2;
        }
    }
    const size_t nb_k = keys.size() * 4, nb_in = in.size() * sizeof(CtrIn), nb_out = in.size() * sizeof(U4Pair);
    uint32_t* d_k;
    CtrIn* d_in;
    U4Pair *d_a, *d_b;
    CHECK(hipMalloc(&d_k, nb_k));
    CHECK(hipMalloc(&d_in, nb_in));
    CHECK(hipMalloc(&d_a, nb_out));
    CHECK(hipMalloc(&d_b, nb_out));
    CHECK(hipMemcpy(d_k, keys.data(), nb_k, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_in, in.data(), nb_in, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_a, 0xEE, nb_out));
    CHECK(hipMemset(d_b, 0xDD, nb_out));
    hipLaunchKernelGGL(k_philox, dim3(n_blocks), dim3(64), 0, 0, d_k, d_in, d_a, d_b);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<U4Pair> a(in.size()), b(in.size());
    CHECK(hipMemcpy(a.data(), d_a, nb_out, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), d_b, nb_out, hipMemcpyDeviceToHost));
    unsigned bad = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        const bool same = std::memcmp(&a[i], &b[i], sizeof(U4Pair)) == 0;
        bad += !same;
        std::printf("%zu %zu %08x %08x %08x %08x %08x %08x %08x %08x%s\n", i / 64, i % 64, a[i].a.x, a[i].a.y, a[i].a.z,
                    a[i].a.w, a[i].b.x, a[i].b.y, a[i].b.z, a[i].b.w, same ? "" : " MISMATCH");
        if (!same)
            std::printf("#   two calls: %08x %08x %08x %08x %08x %08x %08x %08x\n", b[i].a.x, b[i].a.y, b[i].a.z,
                        b[i].a.w, b[i].b.x, b[i].b.y, b[i].b.z, b[i].b.w);
    }
    std::printf("mismatches %u\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    int rc = 2;
    if (!std::strcmp(argv[1], "scatter")) rc = run_scatter(f);
    else if (!std::strcmp(argv[1], "philox")) rc = run_philox(f);
    std::fclose(f);
    return rc;
}
