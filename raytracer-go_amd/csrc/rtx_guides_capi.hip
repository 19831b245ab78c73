// rtx_guides_capi.hip — denoised previews (rtx.h): the entry points around rtx_guides.hip's and
// rtx_denoise.hip's kernels.  The previews of an accumulator are in rtx_accum.hip.
#include <algorithm>
#include <cstring>
#include <limits>

#include "rtx_guides.h"
#include "rtx_internal.h"

using namespace rtxh;

namespace {

// The checks of both guide entries, none of which needs a device.  *pixels: the shard's (0: nothing to do).
int check_guides(const rtx_scene* s, const rtx_camera* cam, const rtx_region* region, uint32_t first_sample, uint32_t count,
                 const void* guides, bool device, uint64_t* pixels) {
    *pixels = 0;
    if (!s) return fail(RTX_ERR_INVALID_ARG, "NULL scene");
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_region(cam, region)) return rc;
    if (count == 0) return fail(RTX_ERR_INVALID_ARG, "guides over 0 samples (a mean over nothing)");
    if (int rc = check_sample_range(first_sample, count)) return rc;
    const uint64_t P = (uint64_t)region_rows(region) * region->width;
    if (P == 0) return RTX_OK;
    if (!guides) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (device && ((uintptr_t)guides & 15u)) return fail(RTX_ERR_INVALID_ARG, "guides must be aligned to 16 B");
    *pixels = P;
    return RTX_OK;
}

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int check_params(const rtx_denoise_params* p) {
    if (!p) return fail(RTX_ERR_INVALID_ARG, "NULL parameters");
    if (p->iterations < 1 || p->iterations > 6) return fail(RTX_ERR_INVALID_ARG, "%u iterations: 1 to 6", p->iterations);
    if (!(p->sigma_normal > 0.0f) || !(p->sigma_depth >= 0.0f) || !(p->sigma_luminance >= 0.0f))
        return fail(RTX_ERR_INVALID_ARG, "sigma_normal > 0, sigma_depth >= 0 and sigma_luminance >= 0 are required");
    return RTX_OK;
}

// The checks of rtx_denoise_device, none of which needs a device.  *pixels: width * rows (0: nothing to do).
int check_denoise(const float* rgb, const float* var, const rtx_guide* guides, uint32_t width, uint32_t rows,
                  const rtx_denoise_params* p, const float* out, const void* work, uint64_t work_bytes, uint64_t* pixels) {
    *pixels = 0;
    if (int rc = check_params(p)) return rc;
    const uint64_t P = (uint64_t)width * rows;
    if (P == 0) return RTX_OK;
    if (P > 0x7FFFFFFFull || rows > 4u * 65535u) return fail(RTX_ERR_INVALID_ARG, "image too large for the filter");
    if (!rgb || !var || !guides || !out || !work) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)rgb | (uintptr_t)var | (uintptr_t)guides | (uintptr_t)out | (uintptr_t)work) & 15u)
        return fail(RTX_ERR_INVALID_ARG, "images, guides and workspace must be aligned to 16 B");
    const uint64_t need = rtx_denoise_workspace_bytes(width, rows);
    if (work_bytes < need)
        return fail(RTX_ERR_INVALID_ARG, "workspace of %llu B < rtx_denoise_workspace_bytes %llu", (unsigned long long)work_bytes,
                    (unsigned long long)need);
    const uint64_t img = P * 3 * sizeof(float), gb = P * sizeof(rtx_guide);
    if (overlap(out, img, rgb, img) || overlap(out, img, var, img) || overlap(out, img, guides, gb) ||
        overlap(out, img, work, need) || overlap(work, need, rgb, img) || overlap(work, need, var, img) ||
        overlap(work, need, guides, gb))
        return fail(RTX_ERR_INVALID_ARG, "the output, the workspace and the inputs must not overlap");
    *pixels = P;
    return RTX_OK;
}

}  // namespace

namespace rtxh {

int guides_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                  uint32_t count, rtx_guide* d_guides, hipStream_t stream, rtx_guide_stats* stats) {
    DeviceCopy* c = nullptr;
    if (int rc = current_copy(s, &c)) return rc;
    const DeviceLayout* lay = nullptr;
    // (and the trace's probe: a timed call borrows its events, the guides having no counters of their own)
    if (int rc = ensure_trace(s, c, rtx_camera_octant(cam), &lay)) return rc;
    rtxd::GuideParams p;
    std::memset(&p, 0, sizeof(p));
    p.shard = shard_of(cam, seed, region, first_sample, count);
    p.scene = walk_scene(s, lay);
    p.want_uv = s->has_image ? 1u : 0u;
    p.materials = c->materials.as<const rtx_material>();
    p.textures = c->textures.as<const rtx_texture>();
    p.texels = c->texels.as<const uint32_t>();
    p.out = d_guides;
    // A/B knobs (read per call): the width of a wave's 64 pixels (3: 8 x 8; 6: 64 x 1, measured 24 % slower), the
    // parked lanes at which a wave folds and hands out the next samples (64: when the whole wave is parked, the plain
    // form; 48 measured 17 % slower: a fold costs the whole wave a hit record, a camera ray and a walk's start),
    // the lanes a primitive test waits for
    p.tile_w_log2 = env_knob("RTX_GUIDES_TILE_W_LOG2", 3, 0, 6);
    p.refill = env_knob("RTX_GUIDES_REFILL", 64, 1, 64);
    p.prim_batch = env_knob("RTX_GUIDES_PRIM_BATCH", 16, 1, 65);
    if (int rc = c->trace.begin(false, stats != nullptr, stream)) return rc;
    if (const hipError_t e = rtxd::launch_guides(p, s->has_noise, stream)) return hip_fail(e, "guides launch failed");
    if (!stats) return RTX_OK;
    float ms = 0.0f;
    if (int rc = c->trace.end(stream, &ms)) return rc;
    stats->rays = (uint64_t)p.shard.width * p.shard.rows * count;
    stats->kernel_ms = ms;
    return RTX_OK;
}

}  // namespace rtxh

extern "C" {

int rtx_guides_device(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                      uint32_t count, rtx_guide* d_guides, void* hip_stream, rtx_guide_stats* stats) {
    g_last_error.clear();
    uint64_t pixels = 0;
    if (int rc = check_guides(s, cam, region, first_sample, count, d_guides, true, &pixels)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (pixels == 0) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    return guides_locked(s, cam, seed, region, first_sample, count, d_guides, (hipStream_t)hip_stream, stats);
}

int rtx_guides(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
               uint32_t count, rtx_guide* guides, rtx_guide_stats* stats) {
    g_last_error.clear();
    uint64_t pixels = 0;
    if (int rc = check_guides(s, cam, region, first_sample, count, guides, false, &pixels)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (pixels == 0) return RTX_OK;
    rtxd::Staging st({{guides, (size_t)pixels * sizeof(rtx_guide), rtxd::Stage::out}});
    rtx_guide_stats local;
    if (int rc = run_staged(st, "rtx_guides' buffer", [&] {
            return rtx_guides_device(s, cam, seed, region, first_sample, count, st.dev<rtx_guide>(0), nullptr, &local);
        }))
        return rc;
    if (stats) *stats = local;
    return RTX_OK;
}

void rtx_denoise_defaults(rtx_denoise_params* p) {
    if (!p) return;
    p->iterations = 5;
    p->sigma_normal = 0.45f;
    p->sigma_depth = 0.05f;
    p->sigma_luminance = 8.0f;
}

uint64_t rtx_denoise_workspace_bytes(uint32_t width, uint32_t rows) { return (uint64_t)width * rows * 2 * sizeof(float4); }

int rtx_denoise_device(const float* d_rgb, const float* d_var, const rtx_guide* d_guides, uint32_t width, uint32_t rows,
                       const rtx_denoise_params* params, float* d_out, void* d_work, uint64_t work_bytes, void* hip_stream) {
    g_last_error.clear();
    uint64_t pixels = 0;
    if (int rc = check_denoise(d_rgb, d_var, d_guides, width, rows, params, d_out, d_work, work_bytes, &pixels)) return rc;
    if (pixels == 0) return RTX_OK;
    const rtxd::DenoiseArgs a{d_rgb, d_var, d_guides, width, rows, *params, d_out, static_cast<float4*>(d_work)};
    if (const hipError_t e = rtxd::launch_denoise(a, (hipStream_t)hip_stream)) return hip_fail(e, "denoise launch failed");
    return RTX_OK;
}

int rtx_denoise(const float* rgb, const float* var, const rtx_guide* guides, uint32_t width, uint32_t rows,
                const rtx_denoise_params* params, float* out_rgb) {
    g_last_error.clear();
    if (int rc = check_params(params)) return rc;
    const uint64_t P = (uint64_t)width * rows;
    if (P == 0) return RTX_OK;
    if (P > 0x7FFFFFFFull) return fail(RTX_ERR_INVALID_ARG, "image too large for the filter");
    if (!rgb || !var || !guides || !out_rgb) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    const size_t img = (size_t)P * 3 * sizeof(float), gb = (size_t)P * sizeof(rtx_guide);
    const uint64_t wb = rtx_denoise_workspace_bytes(width, rows);
    rtxd::Staging st({{rgb, img, rtxd::Stage::in},
                      {var, img, rtxd::Stage::in},
                      {guides, gb, rtxd::Stage::in},
                      {out_rgb, img, rtxd::Stage::out},
                      {nullptr, (size_t)wb, rtxd::Stage::scratch}});
    return run_staged(st, "rtx_denoise's buffers", [&] {
        return rtx_denoise_device(st.dev<float>(0), st.dev<float>(1), st.dev<rtx_guide>(2), width, rows, params, st.dev<float>(3),
                                  st.dev<void>(4), wb, nullptr);
    });
}

}  // extern "C"
