// The short float32 forms of csrc/rtx_device.h against the IEEE operations they replace.  The
// program calls the header's own functions: it holds no copy of a formula.
//
//   device_math_check <section>            exhaustive sections, counted on the device:
//       rcp | sqrt_fast | sqrt_rn | unit | div
//     prints "<section> checked N bad M first XXXXXXXX extra A B" (then lines that begin with #); exit status 1
//     when M != 0.
//   device_math_check <section> IN OUT     sampled sections: IN holds n records of 32-bit words (n a multiple of 64,
//     one 64-lane wave per 64 consecutive records, so the caller decides which lanes share a vote), OUT receives the
//     device function's raw outputs, which the caller judges (tests/test_device_math_gpu.py against numpy):
//       forms  1 -> 2   x -> 1.0f / x, __builtin_sqrtf(x)
//       vote   1 -> 2   x -> rcp_ieee(x), sqrt_rn(x)
//       unit3  3 -> 3   v -> unit(v)
//       trav   6 -> 12  (o, d) -> ix iy iz ra a flags of trav_begin<false>, then of trav_begin<true>
//                       (flags: nx | ny << 1 | nz << 2 | safe << 3)
//       box    14 -> 1  (o, d, bmin, bmax, closest, tmin) -> select | med3 << 1 | select-FMA << 2 | safe << 3 |
//                       safe(FMA) << 4 | near_fma_ok << 5
//       sphere 12 -> 5  (o, d, centre, radius, closest, tmin) -> hit, closest of sphere_test<false, true>, the same of
//                       sphere_test<false, false>, safe
//       ownbox 17 -> 1  (o, d, closest, kind, 9 words) -> own_box_pass (kind 0: centre, radius) or
//                       quad_own_box_pass (kind 1: Q, u, v)
//       trig   6 -> 2   (op, a, b as doubles) -> go_atan2(a, b) | go_acos(a) | go_sin(a) as a double
//       uv     3 -> 2   n -> sphere_uv(n)
//     prints "<section> records N".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raytracer-go_amd/csrc/rtx_device.h"

using namespace rtxd;

#define CHECK(x)                                                         \
    do {                                                                 \
        hipError_t e_ = (x);                                             \
        if (e_ != hipSuccess) {                                          \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            return 2;                                                    \
        }                                                                \
    } while (0)

__device__ __forceinline__ float f_of(uint32_t b) { return __uint_as_float(b); }
__device__ __forceinline__ uint32_t b_of(float f) { return __float_as_uint(f); }
__device__ __forceinline__ bool same_bits(float a, float b) { return b_of(a) == b_of(b) || (a != a && b != b); }
__device__ __forceinline__ bool non_normal(float a) {
    const uint32_t ex = (b_of(a) >> 23) & 0xFFu;
    return ex == 0u || ex == 0xFFu;
}

// ---- exhaustive sections --------------------------------------------------------------------------------------------
// A check sees one bit pattern and adds to c[0] (cases in its domain), c[1] (failures), c[2], c[3] (its own counts).
struct RcpCheck {  // rcp_fast_ok <=> exponent field in 2..252; there rcp_newton == 1.0f / x.  c[2]: predicate failures
    static __device__ void run(uint32_t bits, uint32_t* c) {
        const float x = f_of(bits);
        const uint32_t ex = (bits >> 23) & 0xFFu;
        const bool want = ex >= 2u && ex <= 252u, got = rcp_fast_ok(x);
        bool bad = want != got;
        c[2] += bad;
        if (want) {
            ++c[3];
            bad |= !same_bits(rcp_newton(x), 1.0f / x);
        }
        ++c[0];
        c[1] += bad;
    }
};
// sqrt_rn_fast's domain, the complement of sqrt_rn's guard: |x| >= 2^-96 (negatives: NaN), inf, NaN — and -0, which
// v_sqrt_f32 returns exactly.  c[2]: the patterns left out that differ (0 < x < 2^-96 misrounded without the pre-scaling,
// and the negative subnormals, which v_sqrt_f32 turns into -0 where IEEE says NaN: NEG_SUBNORMAL in the test).
struct SqrtFastCheck {
    static __device__ void run(uint32_t bits, uint32_t* c) {
        const float x = f_of(bits);
        const bool ok = same_bits(sqrt_rn_fast(x), __builtin_sqrtf(x));
        if ((bits & 0x7FFFFFFFu) < 0x0F800000u && bits != 0x80000000u) {
            c[2] += !ok;
            return;
        }
        ++c[0];
        c[1] += !ok;
    }
};
struct SqrtRnCheck {  // c[2]: lanes whose wave took the builtin
    static __device__ void run(uint32_t bits, uint32_t* c) {
        const float x = f_of(bits);
        ++c[0];
        c[2] += ballot(__builtin_fabsf(x) < 0x1p-96f) != 0;
        c[1] += !same_bits(sqrt_rn(x), __builtin_sqrtf(x));
    }
};
struct UnitCheck {  // unit()'s predicate <=> 2^-96 <= q < inf; there rcp_newton(sqrt_rn_fast(q)) == 1 / sqrt(q)
    static __device__ void run(uint32_t bits, uint32_t* c) {
        const float q = f_of(bits);
        const bool want = bits >= 0x0F800000u && bits < 0x7F800000u, got = unit_fast_ok(q);
        bool bad = want != got;
        c[2] += bad;
        if (want) {
            ++c[3];
            bad |= !same_bits(rcp_newton(sqrt_rn_fast(q)), 1.0f / __builtin_sqrtf(q));
        }
        ++c[0];
        c[1] += bad;
    }
};

template <class C>
__global__ void __launch_bounds__(256) k_exhaustive(unsigned long long* counts) {
    __shared__ uint32_t s[5];
    if (threadIdx.x < 5) s[threadIdx.x] = threadIdx.x == 4 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    uint32_t c[4] = {0, 0, 0, 0}, first = 0xFFFFFFFFu;
    // 2^16 blocks of 2^16 consecutive patterns: a wave's 64 lanes hold 64 consecutive patterns
    for (uint32_t k = 0; k < 256u; ++k) {
        const uint32_t bits = (blockIdx.x << 16) | (k << 8) | threadIdx.x;
        const uint32_t before = c[1];
        C::run(bits, c);
        if (c[1] != before && bits < first) first = bits;
    }
    for (int i = 0; i < 4; ++i)
        if (c[i]) atomicAdd(&s[i], c[i]);
    if (first != 0xFFFFFFFFu) atomicMin(&s[4], first);
    __syncthreads();
    if (threadIdx.x < 4 && s[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s[threadIdx.x]);
    if (threadIdx.x == 4 && s[4] != 0xFFFFFFFFu) atomicMin(&counts[4], (unsigned long long)s[4]);
}

__device__ __forceinline__ uint32_t mix(uint32_t x) {  // a 32-bit integer hash
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

// div_by(n, a, RN(1 / a)) against n / a: every significand of a at one exponent; per a, 64 hashed numerators over
// exponents [-40, 40] and both signs (class 0), 8 of n = a * t for t near 0.001 and near 1 (class 1), 18 whose quotient
// lies within 4 ulps of 2^-126 and of 2^128 (class 2), and 18 within 4 ulps of the claim's own ends, |n| = 2^-102 and
// 2^65 (class 3).  The claim (rtx_device.h): for 2^-102 <= |n| <= 2^65 a normal quotient is the division's, bit for bit,
// and a non-normal one (zero, subnormal, inf, NaN) stays non-normal.
// counts: [0] cases inside the claim, [1] failures among them, [2] non-normal reference quotients among them, [3] cases
// outside the claim, [4] the first failing a, [5] failures outside the claim with |n| < 2^-102 and [10] with |n| > 2^65 (reported: why the
// claim ends there), [6 + c] failures of class c.
__global__ void __launch_bounds__(256) k_div(unsigned long long* counts, int exp_a) {
    __shared__ uint32_t s[11];
    if (threadIdx.x < 11) s[threadIdx.x] = threadIdx.x == 4 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint32_t mant = blockIdx.x * 256u + threadIdx.x;  // the grid is exactly 2^23 threads
    const uint32_t abits = ((uint32_t)(exp_a + 127) << 23) | mant;
    const float a = f_of(abits);
    const float y = 1.0f / a;
    uint32_t c[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < 64u + 8u + 18u + 18u; ++k) {
        float n;
        uint32_t cls;
        const uint32_t h = mix(mant * 977u + k * 0x9E3779B9u + (uint32_t)exp_a * 131u);
        if (k < 64u) {
            cls = 0u;
            const int e = (int)(h % 81u) - 40;
            n = f_of((h & 0x80000000u) | ((uint32_t)(e + 127) << 23) | (mix(h) & 0x7FFFFFu));
        } else if (k < 72u) {  // quotients near tmin = 0.001 and near 1: n = a * t (rounded)
            cls = 1u;
            const float t = (k & 1u) ? 0.001f * (1.0f + (float)(h & 0xFFFFu) * 0x1p-20f)
                                     : 1.0f + (float)(h & 0xFFFFu) * 0x1p-18f;
            n = a * t;
        } else if (k < 81u) {  // quotients within 4 ulps of 2^-126
            cls = 2u;
            n = a * f_of(0x00800000u + (k - 72u) - 4u);
        } else if (k < 90u) {  // quotients within 4 ulps of 2^128
            cls = 2u;
            n = (a * f_of(0x7F000000u + (k - 81u) - 4u)) * 2.0f;
        } else if (k < 99u) {  // numerators within 4 ulps of 2^-102
            cls = 3u;
            n = f_of((h & 0x80000000u) | (0x0C800000u + (k - 90u) - 4u));
        } else {  // numerators within 4 ulps of 2^65
            cls = 3u;
            n = f_of((h & 0x80000000u) | (0x60000000u + (k - 99u) - 4u));
        }
        const float q = n / a;
        const float f = div_by(n, a, y);
        const bool fail = non_normal(q) ? !non_normal(f) : b_of(q) != b_of(f);
        if (__builtin_fabsf(n) >= 0x1p-102f && __builtin_fabsf(n) <= 0x1p65f) {
            ++c[0];
            c[1] += fail;
            c[2] += non_normal(q);
            c[6 + cls] += fail;
        } else {
            ++c[3];
            c[__builtin_fabsf(n) < 0x1p-102f ? 5 : 10] += fail;
        }
    }
    for (int i = 0; i < 11; ++i)
        if (i != 4 && c[i]) atomicAdd(&s[i], c[i]);
    if (c[1]) atomicMin(&s[4], abits);
    __syncthreads();
    if (threadIdx.x < 11 && threadIdx.x != 4 && s[threadIdx.x])
        atomicAdd(&counts[threadIdx.x], (unsigned long long)s[threadIdx.x]);
    if (threadIdx.x == 4 && s[4] != 0xFFFFFFFFu) atomicMin(&counts[4], (unsigned long long)s[4]);
}

template <class C>
static int exhaustive(const char* name) {
    unsigned long long* d = nullptr;
    unsigned long long h[5] = {0, 0, 0, 0, ~0ull};
    CHECK(hipMalloc(&d, sizeof h));
    CHECK(hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_exhaustive<C>, dim3(1u << 16), dim3(256), 0, 0, d);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    std::printf("%s checked %llu bad %llu first %08llx extra %llu %llu\n", name, h[0], h[1], h[4] & 0xFFFFFFFFull, h[2],
                h[3]);
    return h[1] ? 1 : 0;
}

static int div_sweep() {
    unsigned long long* d = nullptr;
    unsigned long long h[11] = {0, 0, 0, 0, ~0ull, 0, 0, 0, 0, 0, 0};
    CHECK(hipMalloc(&d, sizeof h));
    CHECK(hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice));
    for (int e = -60; e <= 60; e += 3) {  // 41 exponents, both ends of [2^-60, 2^60] among them
        hipLaunchKernelGGL(k_div, dim3((1u << 23) / 256u), dim3(256), 0, 0, d, e);
        CHECK(hipGetLastError());
    }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    std::printf("div checked %llu bad %llu first %08llx extra %llu %llu\n", h[0], h[1], h[4] & 0xFFFFFFFFull, h[2], h[3]);
    std::printf("# div: failures by class %llu %llu %llu %llu; outside the claim %llu cases, %llu fail below 2^-102, %llu above 2^65\n",
                h[6], h[7], h[8], h[9], h[3], h[5], h[10]);
    return h[1] ? 1 : 0;
}

// ---- sampled sections -----------------------------------------------------------------------------------------------
__device__ __forceinline__ Ray ray_of(const uint32_t* in) {
    return Ray{v3(f_of(in[0]), f_of(in[1]), f_of(in[2])), v3(f_of(in[3]), f_of(in[4]), f_of(in[5]))};
}
__device__ __forceinline__ uint32_t trav_flags(const Trav& t) {
    return (uint32_t)t.nx | (uint32_t)t.ny << 1 | (uint32_t)t.nz << 2 | (uint32_t)t.safe << 3;
}

struct Forms {
    static constexpr uint32_t IN = 1, OUT = 2;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const float x = f_of(in[0]);
        out[0] = b_of(1.0f / x);
        out[1] = b_of(__builtin_sqrtf(x));
    }
};
struct Vote {
    static constexpr uint32_t IN = 1, OUT = 2;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const float x = f_of(in[0]);
        out[0] = b_of(rcp_ieee(x));
        out[1] = b_of(sqrt_rn(x));
    }
};
struct Unit3 {
    static constexpr uint32_t IN = 3, OUT = 3;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const V3 u = unit(v3(f_of(in[0]), f_of(in[1]), f_of(in[2])));
        out[0] = b_of(u.x);
        out[1] = b_of(u.y);
        out[2] = b_of(u.z);
    }
};
struct TravBegin {
    static constexpr uint32_t IN = 6, OUT = 12;
    static __device__ void put(const Trav& t, uint32_t* out) {
        out[0] = b_of(t.ix);
        out[1] = b_of(t.iy);
        out[2] = b_of(t.iz);
        out[3] = b_of(t.ra);
        out[4] = b_of(t.a);
        out[5] = trav_flags(t);
    }
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const Ray r = ray_of(in);
        Trav t0, t1;
        trav_begin<false>(t0, r, 0u);
        trav_begin<true>(t1, r, 0u);
        put(t0, out);
        put(t1, out + 6);
    }
};
struct Box {
    static constexpr uint32_t IN = 14, OUT = 1;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const Ray r = ray_of(in);
        const float4 ea = make_float4(f_of(in[6]), f_of(in[7]), f_of(in[8]), 0.0f);
        const float4 eb = make_float4(f_of(in[9]), f_of(in[10]), f_of(in[11]), 0.0f);
        const float tmin = f_of(in[13]);
        Trav t0, t1;
        trav_begin<false>(t0, r, 0u);
        trav_begin<true>(t1, r, 0u);
        t0.closest = t1.closest = f_of(in[12]);
        const V3 zero = v3(0.0f, 0.0f, 0.0f);
        const V3 no = v3(-(r.o.x * t1.ix), -(r.o.y * t1.iy), -(r.o.z * t1.iz));  // as the near walk forms it
        out[0] = (uint32_t)box_hit<false, false>(t0, r, ea, eb, zero, tmin) |
                 (uint32_t)box_hit<true, false>(t0, r, ea, eb, zero, tmin) << 1 |
                 (uint32_t)box_hit<false, true>(t1, r, ea, eb, no, tmin) << 2 | (uint32_t)t0.safe << 3 |
                 (uint32_t)t1.safe << 4 | (uint32_t)near_fma_ok(r, t1) << 5;
    }
};
struct SphereHit {
    static constexpr uint32_t IN = 12, OUT = 5;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const Ray r = ray_of(in);
        const float rad = f_of(in[9]);
        const float4 ea = make_float4(f_of(in[6]), f_of(in[7]), f_of(in[8]), rad);
        const float4 eb = make_float4(rad * rad, 0.0f, 0.0f, 0.0f);  // hittables.go:100, as the upload stores it
        Trav ta;
        trav_begin<false>(ta, r, 0u);
        ta.closest = f_of(in[10]);
        Trav tb = ta;
        Counters cnt{};
        sphere_test<false, true>(ta, r, ea, eb, 16u, cnt, nullptr, f_of(in[11]));
        sphere_test<false, false>(tb, r, ea, eb, 16u, cnt, nullptr, f_of(in[11]));
        out[0] = (uint32_t)ta.hit;
        out[1] = b_of(ta.closest);
        out[2] = (uint32_t)tb.hit;
        out[3] = b_of(tb.closest);
        out[4] = (uint32_t)ta.safe;
    }
};
struct OwnBox {
    static constexpr uint32_t IN = 17, OUT = 1;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const Ray r = ray_of(in);
        Trav t;
        trav_begin<false>(t, r, 0u);
        t.closest = f_of(in[6]);
        const uint32_t* p = in + 8;
        if (in[7] == 0u) {
            out[0] = (uint32_t)own_box_pass(t, r, make_float4(f_of(p[0]), f_of(p[1]), f_of(p[2]), f_of(p[3])));
        } else {
            out[0] = (uint32_t)quad_own_box_pass(t, r, make_float4(f_of(p[0]), f_of(p[1]), f_of(p[2]), 0.0f),
                                                 make_float4(f_of(p[3]), f_of(p[4]), f_of(p[5]), 0.0f),
                                                 make_float4(f_of(p[6]), f_of(p[7]), f_of(p[8]), 0.0f));
        }
    }
};
__device__ __forceinline__ double d_of(const uint32_t* w) {
    return __longlong_as_double((long long)((unsigned long long)w[0] | (unsigned long long)w[1] << 32));
}
struct Trig {
    static constexpr uint32_t IN = 6, OUT = 2;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const double op = d_of(in), a = d_of(in + 2), b = d_of(in + 4);
        const double v = op == 0.0 ? go_atan2(a, b) : (op == 1.0 ? go_acos(a) : go_sin(a));
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        out[0] = (uint32_t)u;
        out[1] = (uint32_t)(u >> 32);
    }
};
struct SphereUv {
    static constexpr uint32_t IN = 3, OUT = 2;
    static __device__ void run(const uint32_t* in, uint32_t* out) {
        const UV uv = sphere_uv(f_of(in[0]), f_of(in[1]), f_of(in[2]));
        out[0] = b_of(uv.u);
        out[1] = b_of(uv.v);
    }
};

template <class S>
__global__ void __launch_bounds__(64) k_sampled(const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i < n) S::run(in + (size_t)i * S::IN, out + (size_t)i * S::OUT);  // (n is a multiple of 64: whole waves)
}

template <class S>
static int sampled(const char* name, const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    const size_t rec = 4u * S::IN;
    if (bytes <= 0 || (size_t)bytes % (rec * 64u) != 0 || (size_t)bytes / rec > (1u << 26)) {
        std::fprintf(stderr, "%s: the input is not whole waves of %zu-byte records\n", name, rec);
        return 2;
    }
    const uint32_t n = (uint32_t)((size_t)bytes / rec);
    std::vector<uint32_t> in((size_t)n * S::IN), out((size_t)n * S::OUT);
    if (std::fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    std::fclose(f);
    uint32_t *d_in, *d_out;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xEE, out.size() * 4));
    hipLaunchKernelGGL(k_sampled<S>, dim3(n / 64u), dim3(64), 0, 0, d_in, d_out, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f) != 0) return 2;
    std::printf("%s records %u\n", name, n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2) {
        const char* s = argv[1];
        if (!std::strcmp(s, "rcp")) return exhaustive<RcpCheck>(s);
        if (!std::strcmp(s, "sqrt_fast")) return exhaustive<SqrtFastCheck>(s);
        if (!std::strcmp(s, "sqrt_rn")) return exhaustive<SqrtRnCheck>(s);
        if (!std::strcmp(s, "unit")) return exhaustive<UnitCheck>(s);
        if (!std::strcmp(s, "div")) return div_sweep();
    } else if (argc == 4) {
        const char* s = argv[1];
        if (!std::strcmp(s, "forms")) return sampled<Forms>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "vote")) return sampled<Vote>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "unit3")) return sampled<Unit3>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "trav")) return sampled<TravBegin>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "box")) return sampled<Box>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "sphere")) return sampled<SphereHit>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "ownbox")) return sampled<OwnBox>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "trig")) return sampled<Trig>(s, argv[2], argv[3]);
        if (!std::strcmp(s, "uv")) return sampled<SphereUv>(s, argv[2], argv[3]);
    }
    std::fprintf(stderr, "usage: device_math_check <section> [IN OUT]\n");
    return 2;
}
