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
    if ((uint64_t)first_sample + count > 0xFFFFFFFFull)
        return fail(RTX_ERR_INVALID_ARG, "samples %u + %u pass 2^32 - 1 (the RNG's sample word is 32-bit)", first_sample, count);
    const uint64_t P = (uint64_t)region_rows(region) * region->width;
    if (P == 0) return RTX_OK;
    if (!guides) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (device && ((uintptr_t)guides & 15u)) return fail(RTX_ERR_INVALID_ARG, "guides must be aligned to 16 B");
    *pixels = P;
    return RTX_OK;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
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
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const auto it = s->copies.find(cur);
    if (it == s->copies.end()) return fail(RTX_ERR_INVALID_ARG, "the scene has no copy on the current device %d", cur);
    DeviceCopy* c = it->second.get();
    const DeviceLayout* lay = nullptr;
    if (int rc = ensure_trace(s, c, rtx_camera_octant(cam), &lay)) return rc;  // (and the events a timed call uses)
    rtxd::GuideParams p;
    std::memset(&p, 0, sizeof(p));
    p.cam = *cam;
    p.seed = seed;
    p.x0 = region->x0;
    p.y0 = region->y0;
    p.width = region->width;
    p.rows = region_rows(region);
    p.rank = region->rank;
    p.world = region->world;
    p.stripe_log2 = region->stripe > 1u ? (uint32_t)(31 - __builtin_clz(region->stripe)) : 0u;
    p.k0 = first_sample;
    p.kn = count;
    p.entries = lay->entries.as<const float4>();
    p.n_entries = lay->n_entries;
    p.n_quads = (uint32_t)(s->quadtab.size() / 16);
    p.start = lay->start;
    p.prim_end = lay->prim_end;
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
    if (stats) HIP_TRY(hipEventRecord(c->tev0, stream));
    if (const hipError_t e = rtxd::launch_guides(p, s->has_noise, stream))
        return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "guides launch failed: %s", hipGetErrorString(e));
    if (!stats) return RTX_OK;
    HIP_TRY(hipEventRecord(c->tev1, stream));
    HIP_TRY(hipEventSynchronize(c->tev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->tev0, c->tev1));
    stats->rays = (uint64_t)p.width * p.rows * count;
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
    DeviceBuffer d;
    const size_t bytes = (size_t)pixels * sizeof(rtx_guide);
    hipError_t e = d.reserve(bytes);
    int rc = RTX_OK;
    if (e == hipSuccess) {
        rtx_guide_stats local;
        rc = rtx_guides_device(s, cam, seed, region, first_sample, count, d.as<rtx_guide>(), nullptr, &local);
        if (rc == RTX_OK) e = hipMemcpy(guides, d.ptr, bytes, hipMemcpyDeviceToHost);
        if (rc == RTX_OK && stats) *stats = local;
    }
    d.release();
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "rtx_guides' buffer");
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
    DeviceBuffer d_rgb, d_var, d_guides, d_out, d_work;
    const size_t img = (size_t)P * 3 * sizeof(float), gb = (size_t)P * sizeof(rtx_guide);
    const uint64_t wb = rtx_denoise_workspace_bytes(width, rows);
    int rc = RTX_OK;
    hipError_t e = d_rgb.reserve(img);
    if (e == hipSuccess) e = d_var.reserve(img);
    if (e == hipSuccess) e = d_guides.reserve(gb);
    if (e == hipSuccess) e = d_out.reserve(img);
    if (e == hipSuccess) e = d_work.reserve((size_t)wb);
    if (e == hipSuccess) e = hipMemcpy(d_rgb.ptr, rgb, img, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_var.ptr, var, img, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_guides.ptr, guides, gb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = rtx_denoise_device(d_rgb.as<float>(), d_var.as<float>(), d_guides.as<rtx_guide>(), width, rows, params,
                                d_out.as<float>(), d_work.ptr, wb, nullptr);
        if (rc == RTX_OK) e = hipMemcpy(out_rgb, d_out.ptr, img, hipMemcpyDeviceToHost);  // (blocking: after the kernels)
    }
    d_rgb.release();
    d_var.release();
    d_guides.release();
    d_out.release();
    d_work.release();
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "rtx_denoise's buffers");
    return RTX_OK;
}

}  // extern "C"
