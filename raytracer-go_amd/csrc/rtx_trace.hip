// rtx_trace.hip — ray queries: the closest (or any) hit of the CALLER's rays (rtx_trace_device).
//
// The reference's public interface under Render is Hittable.Hit(r *Ray, rayT Interval) (HitInfo, bool)
// (hittables.go:7-20, bvh.go:220-249).  This kernel is that call for a batch: one ray per lane over the threaded
// layout (rtx_layout.h) with the megakernel's own pieces (rtx_device.h: trav_begin, load_entry, box_step,
// sphere_test, quad_test, unit, sphere_uv), each test taking the ray's own tmin and the running bound starting at
// the ray's tmax instead of a render's (0.001, +inf).
//
// Work distribution: no atomics, no cross-wave state.  Wave w owns rays [w * range, (w + 1) * range).  A lane whose
// walk has ended is parked on the end sentinel, where a step changes nothing.  Once `refill` lanes are parked (or all
// are) the whole wave writes the finished lanes' hits and the parked lanes take the next indices of the range by
// ballot and prefix count; refill = 64 is the plain form: a block of 64 rays walked until every lane is parked.
// Walk positions only move forward and the range is finite, so the loop ends; nothing spins.  Every wave vote
// (the ballots here and those inside trav_begin, unit and the batched step) sits where the whole wave arrives:
// rays are begun and hit records computed on all 64 lanes, and only the selects and stores are per lane.
#include "rtx_trace.h"

#include "rtx_launch_name.h"
#include "rtx_walk.h"

namespace rtxd {
namespace {

constexpr uint32_t TRACE_NO_RAY = 0xFFFFFFFFu;
constexpr uint32_t TRACE_LDS_MAX = 64 * 1024;

struct Query {
    Ray r;
    float tmin;
    uint32_t index;  // the lane's ray, TRACE_NO_RAY when it has none
};

// The rtx_hit of a lane's finished walk: hit_record (rtx_walk.h) by every lane, stored where `fin`.  A miss:
// t = +inf, prim = RTX_HIT_NONE, the rest 0.
template <bool QUADS>
__device__ __forceinline__ void write_hit(const TraceParams& p, const SceneRef E, const Trav& t, const Query& q,
                                          const bool fin) {
    const HitRecord h = hit_record<QUADS, true>(E, t, q.r, (p.flags & RTX_TRACE_UV) != 0u, p.rank_sphere);
    if (fin) {
        float4 h0, h1, h2;
        if (h.hit) {
            h0 = make_float4(t.closest, __uint_as_float(h.prim), __uint_as_float(h.mi), __uint_as_float(h.front ? 1u : 0u));
            h1 = make_float4(h.pt.x, h.pt.y, h.pt.z, h.u);
            h2 = make_float4(h.n.x, h.n.y, h.n.z, h.v);
        } else {
            h0 = make_float4(__builtin_inff(), __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f);
            h1 = h2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        float4* o = reinterpret_cast<float4*>(p.hits + q.index);  // 48 B: three 16-byte stores
        o[0] = h0;
        o[1] = h1;
        o[2] = h2;
    }
}

}  // namespace

// COUNT: the counting instantiation (node_visits, prim_tests, hits).  QUADS: the scene holds quads.  FIXED: the
// scene in the workgroup's LDS copy (scene_ref_fixed), else read from HBM.  ANY: RTX_TRACE_ANY, a lane parks at
// its first accepted primitive.
// (In rtxd itself, not in the unit's anonymous namespace: the kernel's host-side handle is then a symbol of the
// library's dynamic table, which is how rtx_launch_name.h names a launch and tests/block_kernels.txt lists it.)
template <bool COUNT, bool QUADS, bool FIXED, bool ANY>
__global__ __launch_bounds__(64 * WALK_WAVES) void trace_rays(TraceParams p) {
    extern __shared__ float4 lds_entries[];
    const SceneRef E = stage_scene<WALK_WAVES, FIXED>(lds_entries, p.scene);
    const uint32_t end = walk_end(p.scene);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WALK_WAVES + (threadIdx.x >> 6));
    const uint64_t first = (uint64_t)wave * p.range;
    if (first >= p.n) return;  // (the whole wave)
    uint32_t next = (uint32_t)first;
    const uint32_t last = (uint32_t)(first + p.range < p.n ? first + p.range : p.n);  // the wave's rays: [next, last)

    Query q{Ray{v3(0.0f, 0.0f, 0.0f), v3(1.0f, 1.0f, 1.0f)}, 0.0f, TRACE_NO_RAY};
    Trav t{};
    trav_begin(t, q.r, end);  // parked on the sentinel until its first ray
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    unsigned long long visits = 0, tests = 0, nhits = 0;  // COUNT

    for (;;) {
        const bool parked = t.i >= end;
        const uint64_t pm = ballot(parked);
        const uint32_t np = (uint32_t)__popcll(pm), rem = last - next;
        if (np == 64u || (rem != 0u && np >= p.refill)) {
            const bool fin = parked && q.index != TRACE_NO_RAY;
            write_hit<QUADS>(p, E, t, q, fin);
            if (COUNT) {
                visits += cnt.node_visits;
                tests += cnt.prim_tests;
                if (fin && t.hit >= 0) ++nhits;
                cnt.node_visits = cnt.prim_tests = 0;
            }
            if (rem == 0u) break;  // every lane parked and written, nothing left to hand out
            // the parked lanes take the next rays of the range, in lane order
            const uint32_t k = (uint32_t)__popcll(pm & below);
            const bool take = parked && k < rem;
            const uint32_t mine = next + k;  // (< last <= n when taken)
            next += np < rem ? np : rem;
            Query nq = q;
            float tmax = 0.0f;
            if (take) {  // 32 B: one dwordx4 pair
                const float4* src = reinterpret_cast<const float4*>(p.rays + mine);
                const float4 ra = src[0], rb = src[1];
                nq.r = Ray{v3(ra.x, ra.y, ra.z), v3(rb.x, rb.y, rb.z)};
                nq.tmin = ra.w;
                tmax = rb.w;
                nq.index = mine;
                // a NaN bound: Interval.In and InBoundary's `min < max` are false for every value: the empty interval
                if (nq.tmin != nq.tmin || tmax != tmax) {
                    nq.tmin = __builtin_inff();
                    tmax = -__builtin_inff();
                }
            }
            Trav nt;
            trav_begin(nt, nq.r, p.scene.start);  // (whole wave: its votes)
            // the fast step forms (med3 boxes, div_by roots) also need every accepted root inside div_by's claim:
            // |n| = |root| a >= 2^-102 (rtx_device.h), so tmin >= 2^-42 for a >= 2^-60
            nt.safe = nt.safe && nq.tmin >= 0x1p-42f;
            nt.closest = tmax;  // the running bound starts at the ray's tmax
            if (take) {
                q = nq;
                t = nt;
            } else if (parked) {
                q.index = TRACE_NO_RAY;  // written above; stays on the sentinel
            }
        }
        t = walk_steps<WALK_STEPS, COUNT, QUADS, FIXED>(t, q.r, E, cnt, end, p.prim_batch, q.tmin, ANY);
    }
    if (COUNT) {
        if (visits) atomicAdd(&p.counters[TRACE_NODE_VISITS], visits);
        if (tests) atomicAdd(&p.counters[TRACE_PRIM_TESTS], tests);
        if (nhits) atomicAdd(&p.counters[TRACE_HITS], nhits);
    }
}

namespace {

template <bool COUNT, bool QUADS, bool FIXED>
hipError_t launch_any(const TraceParams& p, hipStream_t stream) {
    const size_t shmem = FIXED ? walk_lds_bytes(p.scene.n_entries, p.scene.n_quads) : 0;
    const uint64_t waves = ((uint64_t)p.n + p.range - 1) / p.range;
    const dim3 grid((uint32_t)((waves + WALK_WAVES - 1) / WALK_WAVES)), block(64 * WALK_WAVES);
    const auto kern = p.flags & RTX_TRACE_ANY ? &trace_rays<COUNT, QUADS, FIXED, true> : &trace_rays<COUNT, QUADS, FIXED, false>;
    name_launch(kern);
    hipLaunchKernelGGL(kern, grid, block, shmem, stream, p);
    return hipGetLastError();
}

template <bool COUNT>
hipError_t launch_count(const TraceParams& p, hipStream_t stream) {
    const bool fixed = trace_placement(p.scene.n_entries, p.scene.n_quads) == RTX_SCENE_IN_LDS;
    if (p.scene.n_quads) return fixed ? launch_any<COUNT, true, true>(p, stream) : launch_any<COUNT, true, false>(p, stream);
    return fixed ? launch_any<COUNT, false, true>(p, stream) : launch_any<COUNT, false, false>(p, stream);
}

}  // namespace

uint32_t trace_placement(uint32_t n_entries, uint32_t n_quads) {
    // as scene_placement (rtx_kernel.hip) without materials: the 'a' halves below LDS_B and all of it in 64 KB
    return ((uint64_t)n_entries + 1) * 16 <= LDS_B && (uint64_t)walk_lds_bytes(n_entries, 0) + (uint64_t)n_quads * 64 <= TRACE_LDS_MAX
               ? RTX_SCENE_IN_LDS
               : RTX_SCENE_IN_HBM;
}

hipError_t launch_trace(const TraceParams& p, bool count, hipStream_t stream) {
    if (p.n == 0) return hipSuccess;
    if (p.n > TRACE_LAUNCH_MAX || p.range == 0 || p.range % 64u != 0 || p.refill == 0 || p.refill > 64u || !p.rays ||
        !p.hits || !p.scene.entries || !p.rank_sphere || (count && !p.counters))
        return hipErrorInvalidValue;
    return count ? launch_count<true>(p, stream) : launch_count<false>(p, stream);
}

}  // namespace rtxd
