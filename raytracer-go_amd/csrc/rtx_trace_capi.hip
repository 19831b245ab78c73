// rtx_trace_capi.hip — ray queries (rtx.h): the entry points around rtx_trace.hip's kernels.
#include <algorithm>
#include <cstring>
#include <limits>

#include "rtx_internal.h"
#include "rtx_trace.h"

using namespace rtxh;

namespace {

constexpr uint32_t TRACE_FLAGS = RTX_TRACE_ANY | RTX_TRACE_UV | RTX_TRACE_COUNTERS | RTX_TRACE_OCTANT(7);

// The checks of both entries that need no device.  *empty: nothing to do (n == 0).
int check_trace(const rtx_scene* s, const void* rays, uint64_t n, const void* hits, uint32_t flags, bool* empty) {
    *empty = false;
    if (!s) return fail(RTX_ERR_INVALID_ARG, "NULL scene");
    if (flags & ~TRACE_FLAGS) return fail(RTX_ERR_INVALID_ARG, "unknown trace flags 0x%x", flags & ~TRACE_FLAGS);
    if (n == 0) {
        *empty = true;
        return RTX_OK;
    }
    if (!rays || !hits) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)rays | (uintptr_t)hits) & 15u) return fail(RTX_ERR_INVALID_ARG, "rays and hits must be aligned to 16 B");
    if (n > (uint64_t)std::numeric_limits<size_t>::max() / sizeof(rtx_hit)) return fail(RTX_ERR_INVALID_ARG, "too many rays");
    return RTX_OK;
}

}  // namespace

namespace rtxh {

// What a trace on copy c needs beside the scene (s->mu held, current device = c's), made on first use: the
// rank table (the inverse of rank_spheres: one word per sphere entry of `base`, so every entry of a sphere referenced
// more than once names it), the trace's counters and events, and the trace layout for `oct`: the rebuilt tree for
// that octant when the scene has one, else the caller's tree, uncollapsed (the collapse plan is made from a camera's
// sample paths) and stored by upload_layout's rules: primitives first for the LDS copy, the top levels first for a
// big scene.
int ensure_trace(rtx_scene* s, DeviceCopy* c, uint32_t oct, const DeviceLayout** out) {
    if (!c->rank_sphere.ptr) {
        std::vector<uint32_t> tab;
        for (const rtx_entry& e : s->base) {
            int32_t tag, si;
            std::memcpy(&tag, &e.b[3], 4);
            std::memcpy(&si, &e.b[1], 4);
            if (tag >= 0) tab.push_back((uint32_t)si);
        }
        HIP_TRY(c->rank_sphere.reserve(std::max<size_t>(1, tab.size()) * sizeof(uint32_t)));
        if (!tab.empty()) {
            const hipError_t e = hipMemcpy(c->rank_sphere.ptr, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                c->rank_sphere.release();
                return fail(RTX_ERR_HIP, "the rank table: %s", hipGetErrorString(e));
            }
        }
    }
    HIP_TRY(c->trace_counters.reserve(rtxd::TRACE_COUNTER_SLOTS * sizeof(unsigned long long)));
    if (!c->tev0) HIP_TRY(hipEventCreate(&c->tev0));
    if (!c->tev1) HIP_TRY(hipEventCreate(&c->tev1));
    DeviceLayout& lay = c->trace_lay[s->rebuilt ? oct & 7u : 0u];
    if (!lay.entries.ptr) {
        std::vector<rtx_entry> full;
        if (s->rebuilt) rtxd::emit_topology(s->topo, oct & 7u, full);
        if (int rc = upload_layout(s, s->rebuilt ? full : s->base, nullptr, lay)) return rc;
    }
    *out = &lay;
    return RTX_OK;
}

}  // namespace rtxh

extern "C" {

int rtx_trace_device(rtx_scene* s, const rtx_ray* d_rays, uint64_t n, rtx_hit* d_hits, uint32_t flags, void* hip_stream,
                     rtx_trace_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_trace(s, d_rays, n, d_hits, flags, &empty)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (empty) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const auto it = s->copies.find(cur);
    if (it == s->copies.end()) return fail(RTX_ERR_INVALID_ARG, "the scene has no copy on the current device %d", cur);
    DeviceCopy* c = it->second.get();
    const uint32_t oct = (flags >> 8) & 7u;
    const DeviceLayout* lay = nullptr;
    if (int rc = ensure_trace(s, c, oct, &lay)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_TRACE_COUNTERS);
    rtxd::TraceParams p;
    std::memset(&p, 0, sizeof(p));
    p.entries = lay->entries.as<const float4>();
    p.n_entries = lay->n_entries;
    p.n_quads = (uint32_t)(s->quadtab.size() / 16);
    p.start = lay->start;
    p.prim_end = lay->prim_end;
    p.rank_sphere = c->rank_sphere.as<uint32_t>();
    p.flags = flags;
    p.counters = c->trace_counters.as<unsigned long long>();
    // A/B knobs (read per call): rays per wave, the parked lanes at which a wave refills (64: whole blocks of 64
    // rays, the plain form; 48 measured -0.7 % on camera rays and +54 % on incoherent ones against it, DESIGN.md
    // §32), the lanes a primitive test waits for
    p.range = env_knob("RTX_TRACE_RANGE", 512, 64, 1 << 20) / 64u * 64u;
    p.refill = env_knob("RTX_TRACE_REFILL", 48, 1, 64);
    p.prim_batch = env_knob("RTX_TRACE_PRIM_BATCH", 16, 1, 65);
    // rays per launch (32-bit ray indices; RTX_TRACE_LAUNCH_RAYS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_TRACE_LAUNCH_RAYS", (long)rtxd::TRACE_LAUNCH_MAX, 64, (long)rtxd::TRACE_LAUNCH_MAX);
    if (count) HIP_TRY(hipMemsetAsync(c->trace_counters.ptr, 0, c->trace_counters.bytes, stream));
    if (stats) HIP_TRY(hipEventRecord(c->tev0, stream));
    for (uint64_t off = 0; off < n; off += per_launch) {
        p.rays = d_rays + off;
        p.hits = d_hits + off;
        p.n = (uint32_t)std::min<uint64_t>(per_launch, n - off);
        if (const hipError_t e = rtxd::launch_trace(p, count, stream))
            return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "trace launch failed: %s", hipGetErrorString(e));
    }
    if (!stats) return RTX_OK;
    HIP_TRY(hipEventRecord(c->tev1, stream));
    HIP_TRY(hipEventSynchronize(c->tev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->tev0, c->tev1));
    stats->rays = n;
    stats->kernel_ms = ms;
    stats->walk_layout = s->rebuilt ? oct : RTX_LAYOUT_REFERENCE;
    stats->scene_placement = rtxd::trace_placement(p.n_entries, p.n_quads);
    if (count) {
        unsigned long long h[rtxd::TRACE_COUNTER_SLOTS] = {0};
        HIP_TRY(hipMemcpy(h, c->trace_counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
        stats->hits = h[rtxd::TRACE_HITS];
        stats->node_visits = h[rtxd::TRACE_NODE_VISITS];
        stats->prim_tests = h[rtxd::TRACE_PRIM_TESTS];
    }
    return RTX_OK;
}

int rtx_trace(rtx_scene* s, const rtx_ray* rays, uint64_t n, rtx_hit* hits, uint32_t flags, rtx_trace_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_trace(s, rays, n, hits, flags, &empty)) return rc;
    if (empty) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RTX_OK;
    }
    DeviceBuffer d_rays, d_hits;
    rtx_trace_stats local;
    int rc = RTX_OK;
    hipError_t e = d_rays.reserve((size_t)n * sizeof(rtx_ray));
    if (e == hipSuccess) e = d_hits.reserve((size_t)n * sizeof(rtx_hit));
    if (e == hipSuccess) e = hipMemcpy(d_rays.ptr, rays, (size_t)n * sizeof(rtx_ray), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // (with stats: it returns after the kernels; without the caller's, the timed kernel)
        rc = rtx_trace_device(s, d_rays.as<rtx_ray>(), n, d_hits.as<rtx_hit>(), stats ? flags : flags & ~RTX_TRACE_COUNTERS,
                              nullptr, &local);
        if (rc == RTX_OK) e = hipMemcpy(hits, d_hits.ptr, (size_t)n * sizeof(rtx_hit), hipMemcpyDeviceToHost);
    }
    d_rays.release();
    d_hits.release();
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "rtx_trace's buffers: %s", hipGetErrorString(e));
    if (stats) *stats = local;
    return RTX_OK;
}

}  // extern "C"
