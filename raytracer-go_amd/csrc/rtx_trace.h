// rtx_trace.h — launch interface between the C-ABI layer and the ray-query kernel (rtx_trace.hip):
// rtx_trace_device / rtx_trace of include/rtx.h, DESIGN.md §32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx.h"
#include "rtx_walk.h"

namespace rtxd {
// Device counters of a counting trace, in memory of the scene copy's own (never the render's).
constexpr uint32_t TRACE_HITS = 0u, TRACE_NODE_VISITS = 1u, TRACE_PRIM_TESTS = 2u, TRACE_COUNTER_SLOTS = 3u;

// One launch: rays [0, n) of `rays` into `hits`, n <= TRACE_LAUNCH_MAX (ray indices are 32-bit).
constexpr uint64_t TRACE_LAUNCH_MAX = 1ull << 30;
struct TraceParams {
    WalkScene scene;  // a trace layout
    const uint32_t* rank_sphere;  // rank word of a sphere entry (its 'b'.y) -> index into the caller's sphere table
    const rtx_ray* rays;
    rtx_hit* hits;
    uint32_t n;
    uint32_t range;       // rays per wave, a multiple of 64: wave w owns rays [w * range, (w + 1) * range)
    uint32_t refill;      // parked lanes at which a wave hands out the next rays of its range (64: whole blocks)
    uint32_t prim_batch;  // primitive tests wait for this many lanes (trav_step_batched)
    uint32_t flags;       // RTX_TRACE_*
    unsigned long long* counters;  // TRACE_COUNTER_SLOTS, the counting instantiation
};
// RTX_SCENE_IN_LDS when the layout fits the workgroup's LDS copy, else RTX_SCENE_IN_HBM.
uint32_t trace_placement(uint32_t n_entries, uint32_t n_quads);
// Enqueue one launch on `stream`.  count: the counting instantiation (adds to p.counters).
hipError_t launch_trace(const TraceParams& p, bool count, hipStream_t stream);
}  // namespace rtxd
