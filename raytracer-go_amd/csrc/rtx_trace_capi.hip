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
    return check_batch(s, flags, TRACE_FLAGS, "trace", n, sizeof(rtx_hit), {{rays, "rays"}, {hits, "hits"}}, empty);
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
    if (int rc = c->trace.ensure(rtxd::TRACE_COUNTER_SLOTS)) return rc;
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
    DeviceCopy* c = nullptr;
    if (int rc = current_copy(s, &c)) return rc;
    const uint32_t oct = (flags >> 8) & 7u;
    const DeviceLayout* lay = nullptr;
    if (int rc = ensure_trace(s, c, oct, &lay)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_TRACE_COUNTERS);
    rtxd::TraceParams p;
    std::memset(&p, 0, sizeof(p));
    p.scene = walk_scene(s, lay);
    p.rank_sphere = c->rank_sphere.as<uint32_t>();
    p.flags = flags;
    p.counters = c->trace.slots();
    // A/B knobs (read per call): rays per wave, the parked lanes at which a wave refills (64: whole blocks of 64
    // rays, the plain form; 48 measured -0.7 % on camera rays and +54 % on incoherent ones against it, DESIGN.md
    // §32), the lanes a primitive test waits for
    p.range = env_knob("RTX_TRACE_RANGE", 512, 64, 1 << 20) / 64u * 64u;
    p.refill = env_knob("RTX_TRACE_REFILL", 48, 1, 64);
    p.prim_batch = env_knob("RTX_TRACE_PRIM_BATCH", 16, 1, 65);
    // rays per launch (32-bit ray indices; RTX_TRACE_LAUNCH_RAYS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_TRACE_LAUNCH_RAYS", (long)rtxd::TRACE_LAUNCH_MAX, 64, (long)rtxd::TRACE_LAUNCH_MAX);
    if (int rc = c->trace.begin(count, stats != nullptr, stream)) return rc;
    if (int rc = for_launches(n, per_launch, [&](uint64_t off, uint32_t m) {
            p.rays = d_rays + off;
            p.hits = d_hits + off;
            p.n = m;
            const hipError_t e = rtxd::launch_trace(p, count, stream);
            return e == hipSuccess ? RTX_OK : hip_fail(e, "trace launch failed");
        }))
        return rc;
    if (!stats) return RTX_OK;
    float ms = 0.0f;
    if (int rc = c->trace.end(stream, &ms)) return rc;
    stats->rays = n;
    stats->kernel_ms = ms;
    stats->walk_layout = s->rebuilt ? oct : RTX_LAYOUT_REFERENCE;
    stats->scene_placement = rtxd::trace_placement(p.scene.n_entries, p.scene.n_quads);
    if (count) {
        unsigned long long h[rtxd::TRACE_COUNTER_SLOTS] = {0};
        if (int rc = c->trace.read(h, rtxd::TRACE_COUNTER_SLOTS)) return rc;
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
    rtxd::Staging st({{rays, (size_t)n * sizeof(rtx_ray), rtxd::Stage::in}, {hits, (size_t)n * sizeof(rtx_hit), rtxd::Stage::out}});
    rtx_trace_stats local;
    // (with stats: the device entry returns after the kernels; without the caller's, the timed kernel)
    if (int rc = run_staged(st, "rtx_trace's buffers", [&] {
            return rtx_trace_device(s, st.dev<rtx_ray>(0), n, st.dev<rtx_hit>(1), stats ? flags : flags & ~RTX_TRACE_COUNTERS,
                                    nullptr, &local);
        }))
        return rc;
    if (stats) *stats = local;
    return RTX_OK;
}

}  // extern "C"
