// rtx_direct_capi.hip — direct light sampling and its multiple importance sampling (rtx.h): the
// entry points around rtx_direct.hip's kernels.
// The emitter table itself is host-only code (rtx_scene.hip: build_lights, rtx_lights, rtx_scene_lights).
#include <algorithm>
#include <cstring>
#include <limits>

#include "rtx_direct.h"
#include "rtx_internal.h"

using namespace rtxh;

namespace {

constexpr uint32_t DIRECT_FLAGS = RTX_DIRECT_COUNTERS;

// The checks of both entries that need no device.  *empty: nothing to do (n == 0).
int check_direct(const rtx_scene* s, const void* hits, const void* keys, uint64_t n, const void* out, uint32_t flags,
                 bool* empty) {
    return check_batch(s, flags, DIRECT_FLAGS, "direct", n, sizeof(rtx_direct_sample),
                       {{hits, "hits"}, {keys, "keys"}, {out, "light samples"}}, empty);
}

constexpr uint32_t EMITTER_FLAGS = RTX_EMITTER_COUNTERS;

int check_emitter(const rtx_scene* s, const void* from, const void* hits, uint64_t n, const void* out, uint32_t flags,
                  bool* empty) {
    return check_batch(s, flags, EMITTER_FLAGS, "emitter weight", n, sizeof(rtx_hit),
                       {{from, "from hits"}, {hits, "hits"}, {out, "weights"}}, empty);
}

// One table of a copy, uploaded on first use (a blocking copy).
int upload_table(DeviceBuffer& buf, const void* src, size_t bytes, const char* what) {
    if (buf.ptr) return RTX_OK;
    HIP_TRY(buf.reserve(std::max<size_t>(64, bytes)));
    if (bytes) {
        const hipError_t e = hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            buf.release();
            return fail(RTX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        }
    }
    return RTX_OK;
}

// What a call on copy c needs beside the trace layout (s->mu held, current device = c's), made on first use: the
// emitter records and the per-primitive lookup, and counters and events of its own, so that a counting call changes
// nobody else's stats.
int ensure_direct(rtx_scene* s, DeviceCopy* c) {
    if (int rc = scene_lights(s)) return rc;
    if (int rc = upload_table(c->lights, s->lighttab.data(), s->lighttab.size() * sizeof(float), "the emitter table")) return rc;
    if (int rc = upload_table(c->prim_lights, s->primlights.data(), s->primlights.size() * sizeof(rtx_prim_light),
                              "the per-primitive emitter lookup"))
        return rc;
    return c->direct.ensure(rtxd::DIRECT_COUNTER_SLOTS);
}

rtxd::PrimLights prim_lights(const rtx_scene* s, const DeviceCopy* c) {
    return rtxd::PrimLights{c->prim_lights.as<const float2>(), (uint32_t)s->sphere_rank.size(), (uint32_t)(s->quadtab.size() / 16)};
}

}  // namespace

namespace rtxh {

// One fused pass (rtx_accum_add_direct after its checks; s->mu held, current device = the accumulator's): samples
// [first, first + count) of the region by direct_paths into the tile-major moments acc_s / acc_q.
int direct_pass_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t tile_w_log2,
                       uint32_t first, uint32_t count, float* acc_s, float* acc_q, hipStream_t stream, rtx_stats* stats,
                       bool mis) {
    DeviceCopy* c = nullptr;
    int cur = 0;
    if (int rc = current_copy(s, &c, &cur)) return rc;
    const uint32_t oct = rtx_camera_octant(cam);
    const DeviceLayout* lay = nullptr;
    if (int rc = ensure_trace(s, c, oct, &lay)) return rc;
    if (int rc = ensure_direct(s, c)) return rc;
    rtxd::DirectPathParams p;
    std::memset(&p, 0, sizeof(p));
    p.shard = shard_of(cam, seed, region, first, count);
    p.scene = walk_scene(s, lay);
    p.tile_w_log2 = tile_w_log2;
    p.want_uv = s->has_image ? 1u : 0u;
    p.materials = c->materials.as<const rtx_material>();
    p.textures = c->textures.as<const rtx_texture>();
    p.texels = c->texels.as<const uint32_t>();
    p.n_materials = (uint32_t)s->materials.size();
    p.n_lights = (uint32_t)s->lights.size();
    p.lights = c->lights.as<const float4>();
    p.acc_s = acc_s;
    p.acc_q = acc_q;
    p.rank_sphere = c->rank_sphere.as<uint32_t>();  // (ensure_trace's)
    p.prims = prim_lights(s, c);
    // A/B knobs (read per call): the parked lanes at which a wave runs its fold step, the lanes a primitive test waits for
    p.refill = env_knob("RTX_DIRECT_REFILL", 32, 1, 64);
    p.prim_batch = env_knob("RTX_DIRECT_PRIM_BATCH", 16, 1, 65);
    {   // ordered like a render on the device (enqueue_on): after the last one, and the readers of an accumulator
        // (resolve, ppm, preview: wait_for_renders) wait for this pass through the same event
        std::lock_guard<std::mutex> sl(g_scratch_mu);
        Scratch& scr = g_scratch[cur];
        if (!scr.last) HIP_TRY(hipEventCreateWithFlags(&scr.last, hipEventDisableTiming));
        else HIP_TRY(hipStreamWaitEvent(stream, scr.last, 0));
        if (int rc = c->direct.begin(false, stats != nullptr, stream)) return rc;
        if (const hipError_t e = rtxd::launch_direct_paths(p, s->has_noise, mis, stream)) return hip_fail(e, "direct pass launch failed");
        HIP_TRY(hipEventRecord(scr.last, stream));
    }
    if (!stats) return RTX_OK;
    // (the closing event follows scr.last's record, outside the lock: no kernel runs between the two)
    float ms = 0.0f;
    if (int rc = c->direct.end(stream, &ms)) return rc;
    std::memset(stats, 0, sizeof(*stats));
    stats->samples = (uint64_t)p.shard.rows * p.shard.width * count;
    stats->kernel_ms = ms;
    stats->sample_chunks = 1;
    stats->walk_layout = s->rebuilt ? oct : RTX_LAYOUT_REFERENCE;
    return RTX_OK;
}

}  // namespace rtxh

extern "C" {

int rtx_direct_device(rtx_scene* s, uint64_t seed, const rtx_hit* d_hits, const rtx_path_key* d_keys, uint64_t n,
                      rtx_direct_sample* d_out, uint32_t flags, void* hip_stream, rtx_direct_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_direct(s, d_hits, d_keys, n, d_out, flags, &empty)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (empty) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = current_copy(s, &c)) return rc;
    // (a shadow ray has no camera to hint an octant with: every hint gives the same hits, so octant 0's layout)
    const DeviceLayout* lay = nullptr;
    if (int rc = ensure_trace(s, c, 0u, &lay)) return rc;
    if (int rc = ensure_direct(s, c)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_DIRECT_COUNTERS);
    rtxd::DirectParams p;
    std::memset(&p, 0, sizeof(p));
    p.scene = walk_scene(s, lay);
    p.materials = c->materials.as<const rtx_material>();
    p.textures = c->textures.as<const rtx_texture>();
    p.texels = c->texels.as<const uint32_t>();
    p.n_materials = (uint32_t)s->materials.size();
    p.n_lights = (uint32_t)s->lights.size();
    p.lights = c->lights.as<const float4>();
    p.seed = seed;
    p.counters = c->direct.slots();
    // A/B knobs (read per call): records per wave, the lanes a primitive test waits for
    p.range = env_knob("RTX_DIRECT_RANGE", 256, 64, 1 << 20) / 64u * 64u;
    p.prim_batch = env_knob("RTX_DIRECT_PRIM_BATCH", 16, 1, 65);
    // records per launch (32-bit record indices; RTX_DIRECT_LAUNCH_RECORDS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_DIRECT_LAUNCH_RECORDS", (long)rtxd::DIRECT_LAUNCH_MAX, 64, (long)rtxd::DIRECT_LAUNCH_MAX);
    if (int rc = c->direct.begin(count, stats != nullptr, stream)) return rc;
    if (int rc = for_launches(n, per_launch, [&](uint64_t off, uint32_t m) {
            p.hits = d_hits + off;
            p.keys = d_keys + off;
            p.out = d_out + off;
            p.n = m;
            const hipError_t e = rtxd::launch_direct(p, count, s->has_noise, stream);
            return e == hipSuccess ? RTX_OK : hip_fail(e, "direct launch failed");
        }))
        return rc;
    if (!stats) return RTX_OK;
    float ms = 0.0f;
    if (int rc = c->direct.end(stream, &ms)) return rc;
    stats->n = n;
    stats->kernel_ms = ms;
    if (count) {
        unsigned long long h[rtxd::DIRECT_COUNTER_SLOTS] = {0};
        if (int rc = c->direct.read(h, rtxd::DIRECT_COUNTER_SLOTS)) return rc;
        stats->sampled = h[rtxd::DIRECT_SAMPLED];
        stats->visible = h[rtxd::DIRECT_VISIBLE];
        stats->rng_draws = h[rtxd::DIRECT_RNG_DRAWS];
    }
    return RTX_OK;
}

int rtx_emitter_weight_device(rtx_scene* s, const rtx_hit* d_from, const rtx_hit* d_hits, uint64_t n,
                              rtx_emitter_weight_record* d_out, uint32_t flags, void* hip_stream, rtx_emitter_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_emitter(s, d_from, d_hits, n, d_out, flags, &empty)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (empty) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = current_copy(s, &c)) return rc;
    if (int rc = ensure_direct(s, c)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_EMITTER_COUNTERS);
    rtxd::EmitterWeightParams p;
    std::memset(&p, 0, sizeof(p));
    p.materials = c->materials.as<const rtx_material>();
    p.n_materials = (uint32_t)s->materials.size();
    p.n_lights = (uint32_t)s->lights.size();
    p.prims = prim_lights(s, c);
    p.counters = c->direct.slots();
    // records per launch (32-bit record indices; RTX_EMITTER_LAUNCH_RECORDS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_EMITTER_LAUNCH_RECORDS", (long)rtxd::DIRECT_LAUNCH_MAX, 64, (long)rtxd::DIRECT_LAUNCH_MAX);
    if (int rc = c->direct.begin(count, stats != nullptr, stream)) return rc;
    if (int rc = for_launches(n, per_launch, [&](uint64_t off, uint32_t m) {
            p.from = d_from + off;
            p.hits = d_hits + off;
            p.out = d_out + off;
            p.n = m;
            const hipError_t e = rtxd::launch_emitter_weights(p, count, stream);
            return e == hipSuccess ? RTX_OK : hip_fail(e, "emitter-weight launch failed");
        }))
        return rc;
    if (!stats) return RTX_OK;
    float ms = 0.0f;
    if (int rc = c->direct.end(stream, &ms)) return rc;
    stats->n = n;
    stats->kernel_ms = ms;
    if (count) {
        unsigned long long h[1] = {0};
        if (int rc = c->direct.read(h, 1)) return rc;
        stats->weighted = h[rtxd::EMITTER_WEIGHTED];
    }
    return RTX_OK;
}

int rtx_emitter_weight(rtx_scene* s, const rtx_hit* from, const rtx_hit* hits, uint64_t n, rtx_emitter_weight_record* out,
                       uint32_t flags, rtx_emitter_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_emitter(s, from, hits, n, out, flags, &empty)) return rc;
    if (empty) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RTX_OK;
    }
    const size_t N = (size_t)n;
    rtxd::Staging st({{from, N * sizeof(rtx_hit), rtxd::Stage::in},
                      {hits, N * sizeof(rtx_hit), rtxd::Stage::in},
                      {out, N * sizeof(rtx_emitter_weight_record), rtxd::Stage::out}});
    rtx_emitter_stats local;
    if (int rc = run_staged(st, "rtx_emitter_weight's buffers", [&] {
            return rtx_emitter_weight_device(s, st.dev<rtx_hit>(0), st.dev<rtx_hit>(1), n, st.dev<rtx_emitter_weight_record>(2),
                                             stats ? flags : flags & ~RTX_EMITTER_COUNTERS, nullptr, &local);
        }))
        return rc;
    if (stats) *stats = local;
    return RTX_OK;
}

int rtx_direct(rtx_scene* s, uint64_t seed, const rtx_hit* hits, const rtx_path_key* keys, uint64_t n, rtx_direct_sample* out,
               uint32_t flags, rtx_direct_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_direct(s, hits, keys, n, out, flags, &empty)) return rc;
    if (empty) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RTX_OK;
    }
    const size_t N = (size_t)n;
    rtxd::Staging st({{hits, N * sizeof(rtx_hit), rtxd::Stage::in},
                      {keys, N * sizeof(rtx_path_key), rtxd::Stage::in},
                      {out, N * sizeof(rtx_direct_sample), rtxd::Stage::out}});
    rtx_direct_stats local;
    // (with stats: the device entry returns after the kernels; without the caller's, the timed kernel)
    if (int rc = run_staged(st, "rtx_direct's buffers", [&] {
            return rtx_direct_device(s, seed, st.dev<rtx_hit>(0), st.dev<rtx_path_key>(1), n, st.dev<rtx_direct_sample>(2),
                                     stats ? flags : flags & ~RTX_DIRECT_COUNTERS, nullptr, &local);
        }))
        return rc;
    if (stats) *stats = local;
    return RTX_OK;
}

}  // extern "C"
