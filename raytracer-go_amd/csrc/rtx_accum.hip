// rtx_accum.hip — progressive rendering (ABI 10, additive).
#include <algorithm>
#include <new>

#include "rtx_guides.h"
#include "rtx_internal.h"
#include "rtx_ppm.h"

using namespace rtxh;

// One (scene, device, camera, seed, region): the running sums S and Q of its shard's sample colours, tile-major
// (rtx_kernel.hip accumulate_samples), owned by the accumulator and not part of the per-device scratch, and the
// samples done.
struct rtx_accum {
    rtx_scene* scene = nullptr;
    int device = -1;
    rtx_camera cam;
    uint64_t seed = 0;
    rtx_region region;
    uint32_t rows = 0;         // region_rows(&region)
    uint32_t tile_w_log2 = 0;  // the tiles S and Q are laid out in (make_params)
    uint64_t slots = 0;        // tiles x 64
    rtxd::DeviceBuffer sums;   // S: slots x 3 floats, then Q's slots x 3
    rtxd::DeviceBuffer noisy;  // resolve_accum's count (one u64)
    // previews, made by the first one: the resolved image, its variance, the guides and the filter's
    // workspace, 12 + 12 + 32 + 32 B per pixel of the shard
    rtxd::DeviceBuffer preview;
    // adaptive passes: the open-tile count (u32, padded to 8 B) and the open-pixel count (u64) of the
    // last selection, then one word per tile (0: open, else the n it closed at), then the list of open tiles
    rtxd::DeviceBuffer adapt;
    bool adaptive = false;  // an adaptive pass since create / reset: the tiles no longer share one n
    bool direct = false;    // a direct-light pass since create / reset: another estimator's samples
    bool mis = false;       // an MIS pass since create / reset: a third estimator's
    uint32_t n = 0;         // the frontier: the samples offered so far
    float* s() const { return sums.as<float>(); }
    float* q() const { return s() + slots * 3; }
    uint32_t tiles() const { return (uint32_t)(slots / 64); }
    uint32_t* n_open() const { return adapt.as<uint32_t>(); }
    unsigned long long* open_pixels() const { return adapt.as<unsigned long long>() + 1; }
    uint32_t* tile_n() const { return adapt.as<uint32_t>() + 4; }
    uint32_t* tile_list() const { return tile_n() + tiles(); }
    size_t adapt_bytes() const { return 16 + 2 * sizeof(uint32_t) * (size_t)tiles(); }
    const uint32_t* closed_at() const { return adaptive ? tile_n() : nullptr; }  // what a reader of S and Q divides by
};

namespace {
// The accumulator's device is the current one (every entry that touches its memory).
int accum_device(const rtx_accum* a) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != a->device)
        return fail(RTX_ERR_INVALID_ARG, "the accumulator lives on device %d, the current device is %d", a->device, cur);
    return RTX_OK;
}
size_t accum_bytes(const rtx_accum* a) { return (size_t)a->slots * 3 * sizeof(float); }  // of S, and of Q

// rtx_accum_resolve_device with a->scene->mu held.
int accum_resolve_locked(rtx_accum* a, float* d_rgb, float* d_var, float rel_tol, hipStream_t st, uint64_t* noisy) {
    if (noisy) HIP_TRY(hipMemsetAsync(a->noisy.ptr, 0, sizeof(unsigned long long), st));
    const rtxd::ResolveArgs ra{a->s(), a->q(), d_rgb, d_var, noisy ? a->noisy.as<unsigned long long>() : nullptr,
                               a->region.width, a->rows, a->tile_w_log2, a->n, rel_tol, a->closed_at()};
    HIP_TRY(rtxd::launch_resolve(ra, st));
    if (noisy) {
        unsigned long long h = 0;
        HIP_TRY(hipMemcpyAsync(&h, a->noisy.ptr, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *noisy = h;
    }
    return RTX_OK;
}

// The checks of the three preview entries that need no device.
int check_preview(const rtx_accum* a, uint32_t guide_samples, const rtx_denoise_params** params, rtx_denoise_params* dflt) {
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (guide_samples == 0) return fail(RTX_ERR_INVALID_ARG, "guides over 0 samples (a mean over nothing)");
    if (a->n == 0) return fail(RTX_ERR_INVALID_ARG, "nothing accumulated yet");
    if (!*params) {
        rtx_denoise_defaults(dflt);
        *params = dflt;
    }
    return RTX_OK;
}

// rtx_accum_preview_device with a->scene->mu held: resolve, guides over [0, min(n, guide_samples)), filter.
int accum_preview_locked(rtx_accum* a, uint32_t guide_samples, const rtx_denoise_params* params, float* d_out, hipStream_t st) {
    const uint64_t P = (uint64_t)a->rows * a->region.width;
    if (P == 0) return RTX_OK;
    // the four images, each starting on a 16-B boundary
    const size_t img = ((size_t)P * 3 * sizeof(float) + 15) / 16 * 16, gb = (size_t)P * sizeof(rtx_guide);
    const uint64_t wb = rtx_denoise_workspace_bytes(a->region.width, a->rows);
    HIP_TRY(a->preview.reserve(2 * img + gb + (size_t)wb));
    char* base = a->preview.as<char>();
    float* rgb = reinterpret_cast<float*>(base);
    float* var = reinterpret_cast<float*>(base + img);
    rtx_guide* guides = reinterpret_cast<rtx_guide*>(base + 2 * img);
    void* work = base + 2 * img + gb;
    if (int rc = accum_resolve_locked(a, rgb, var, 0.0f, st, nullptr)) return rc;
    if (int rc = guides_locked(a->scene, &a->cam, a->seed, &a->region, 0, std::min(a->n, guide_samples), guides, st, nullptr))
        return rc;
    return rtx_denoise_device(rgb, var, guides, a->region.width, a->rows, params, d_out, work, wb, st);
}
}  // namespace

extern "C" {

int rtx_accum_create(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, rtx_accum** out) {
    g_last_error.clear();
    if (!s || !out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_region(cam, region)) return rc;
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, cur, &c)) return rc;
    rtx_accum* a = new (std::nothrow) rtx_accum();
    if (!a) return fail(RTX_ERR_OOM, "host memory for an accumulator");
    a->scene = s;
    a->device = cur;
    a->cam = *cam;
    a->seed = seed;
    a->region = *region;
    a->rows = region_rows(region);
    a->tile_w_log2 = make_params(s, c, layout_slot(s, cam), cam, seed, region, nullptr).tile_w_log2;
    a->slots = (uint64_t)rtxd::tiles_x_of(region->width, a->tile_w_log2) * rtxd::tiles_y_of(a->rows, a->tile_w_log2) * 64;
    hipError_t e = a->sums.reserve(std::max<size_t>(2 * accum_bytes(a), sizeof(float)));
    if (e == hipSuccess) e = zero_now(a->sums.ptr, a->sums.bytes);  // (the first pass may run on any stream, at once)
    if (e == hipSuccess) e = a->noisy.reserve(sizeof(unsigned long long));
    if (e == hipSuccess) e = a->adapt.reserve(a->adapt_bytes());
    if (e == hipSuccess) e = zero_now(a->adapt.ptr, a->adapt.bytes);  // every tile open
    if (e != hipSuccess) {
        a->sums.release();
        a->noisy.release();
        a->adapt.release();
        delete a;
        return hip_fail(e, "the accumulator's buffers");
    }
    *out = a;
    return RTX_OK;
}

int rtx_accum_add(rtx_accum* a, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (count == 0) return fail(RTX_ERR_INVALID_ARG, "a pass of 0 samples");
    if (int rc = check_sample_range(a->n, count)) return rc;
    if (a->adaptive)
        return fail(RTX_ERR_INVALID_ARG, "a uniform pass after an adaptive one: the tiles no longer share one n (reset first)");
    if (a->direct) return fail(RTX_ERR_INVALID_ARG, "a plain pass after a direct-light one: another estimator (reset first)");
    if (a->mis) return fail(RTX_ERR_INVALID_ARG, "a plain pass after an MIS one: another estimator (reset first)");
    if (int rc = accum_device(a)) return rc;
    rtx_scene* s = a->scene;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, a->device, &c)) return rc;
    const rtxd::SampleRange pass{a->n, count, a->s(), a->q()};
    uint32_t chunks = 0;
    bool tiered = false;
    if (int rc = enqueue_on(s, c, &a->cam, a->seed, &a->region, nullptr, (hipStream_t)hip_stream, flags, stats != nullptr,
                            &chunks, &tiered, &pass, a->slots))
        return rc;
    a->n += count;
    if (!stats) return RTX_OK;
    const int rc = collect_on(c, (flags & RTX_FLAG_COUNTERS) != 0, (uint64_t)a->rows * a->region.width * count, chunks, stats);
    stats->walk_layout = walk_layout(s, &a->cam, tiered);
    return rc;
}

int rtx_accum_add_adaptive(rtx_accum* a, uint32_t count, float rel_tol, uint32_t min_samples, void* hip_stream,
                           uint32_t flags, rtx_stats* stats, rtx_adapt_stats* adapt_stats) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (count == 0) return fail(RTX_ERR_INVALID_ARG, "a pass of 0 samples");
    if (int rc = check_sample_range(a->n, count)) return rc;
    if (!(rel_tol >= 0.0f)) return fail(RTX_ERR_INVALID_ARG, "rel_tol %g: a tolerance is >= 0", (double)rel_tol);
    if (a->direct) return fail(RTX_ERR_INVALID_ARG, "an adaptive pass after a direct-light one: another estimator (reset first)");
    if (a->mis) return fail(RTX_ERR_INVALID_ARG, "an adaptive pass after an MIS one: another estimator (reset first)");
    if (int rc = accum_device(a)) return rc;
    rtx_scene* s = a->scene;
    hipStream_t st = (hipStream_t)hip_stream;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, a->device, &c)) return rc;
    const bool live = a->slots != 0;  // (an empty shard: no tile, nothing to select or render)
    if (live) {
        // select: on the pass's stream, after every render on the device (the last pass may have run on another stream)
        if (int rc = wait_for_renders(a->device, st)) return rc;
        HIP_TRY(hipMemsetAsync(a->adapt.ptr, 0, 16, st));
        const rtxd::SelectArgs sel{a->s(), a->q(), a->tile_n(), a->tile_list(), a->n_open(), a->open_pixels(),
                                   a->region.width, a->rows, a->tile_w_log2, a->n, rel_tol,
                                   a->n >= std::max(min_samples, 1u) ? 1u : 0u};
        HIP_TRY(rtxd::launch_select(sel, st));
        a->adaptive = true;  // (from here on: the selection may have closed tiles even if the pass fails below)
    }
    // sample: the pass's launches read the list and its count from device memory
    const rtxd::SampleRange pass{a->n, count, a->s(), a->q(), live ? a->tile_list() : nullptr, live ? a->n_open() : nullptr};
    uint32_t chunks = 0;
    bool tiered = false;
    if (int rc = enqueue_on(s, c, &a->cam, a->seed, &a->region, nullptr, st, flags, stats != nullptr, &chunks, &tiered, &pass,
                            a->slots))
        return rc;
    a->n += count;
    a->adaptive = true;
    if (!stats && !adapt_stats) return RTX_OK;
    struct {
        uint32_t n_open, pad;
        unsigned long long open_pixels;
    } h = {0u, 0u, 0ull};
    HIP_TRY(hipStreamSynchronize(st));
    if (live) HIP_TRY(hipMemcpy(&h, a->adapt.ptr, sizeof(h), hipMemcpyDeviceToHost));
    if (adapt_stats) {
        adapt_stats->tiles = a->tiles();
        adapt_stats->open_tiles = h.n_open;
        adapt_stats->open_pixels = h.open_pixels;
    }
    if (!stats) return RTX_OK;
    const int rc = collect_on(c, (flags & RTX_FLAG_COUNTERS) != 0, (uint64_t)h.open_pixels * count, chunks, stats);
    stats->walk_layout = walk_layout(s, &a->cam, tiered);
    return rc;
}

namespace {
// rtx_accum_add_direct and rtx_accum_add_mis: one fused pass of the estimator `mis` names, after the checks that need no
// device.  The accumulator's first pass, or one more of the same estimator.
int add_light_pass(rtx_accum* a, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats, bool mis) {
    const char* what = mis ? "an MIS" : "a direct-light";
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (count == 0) return fail(RTX_ERR_INVALID_ARG, "a pass of 0 samples");
    if (int rc = check_sample_range(a->n, count)) return rc;
    if (flags != 0u) return fail(RTX_ERR_INVALID_ARG, "%s pass flags 0x%x: must be 0", mis ? "MIS" : "direct", flags);
    if (a->adaptive) return fail(RTX_ERR_INVALID_ARG, "%s pass after an adaptive one (reset first)", what);
    if (a->n != 0u && !(mis ? a->mis : a->direct))
        return fail(RTX_ERR_INVALID_ARG, "%s pass after %s one: another estimator (reset first)", what,
                    a->direct ? "a direct-light" : a->mis ? "an MIS" : "a plain");
    if (int rc = accum_device(a)) return rc;
    rtx_scene* s = a->scene;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, a->device, &c)) return rc;
    if (a->slots != 0) {  // (an empty shard: nothing to render)
        if (int rc = direct_pass_locked(s, &a->cam, a->seed, &a->region, a->tile_w_log2, a->n, count, a->s(), a->q(),
                                        (hipStream_t)hip_stream, stats, mis))
            return rc;
    } else if (stats) {
        *stats = rtx_stats{};
    }
    (mis ? a->mis : a->direct) = true;
    a->n += count;
    return RTX_OK;
}
}  // namespace

int rtx_accum_add_direct(rtx_accum* a, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats) {
    g_last_error.clear();
    return add_light_pass(a, count, hip_stream, flags, stats, false);
}

int rtx_accum_add_mis(rtx_accum* a, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats) {
    g_last_error.clear();
    return add_light_pass(a, count, hip_stream, flags, stats, true);
}

uint32_t rtx_accum_samples(const rtx_accum* a) { return a ? a->n : 0u; }

int rtx_accum_tile_shape(const rtx_accum* a, uint32_t* tile_width, uint32_t* tile_height) {
    g_last_error.clear();
    if (!a || !tile_width || !tile_height) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    *tile_width = 1u << a->tile_w_log2;
    *tile_height = 64u >> a->tile_w_log2;
    return RTX_OK;
}

int rtx_accum_sample_counts_device(rtx_accum* a, uint32_t* d_counts, void* hip_stream) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (!d_counts && (uint64_t)a->rows * a->region.width) return fail(RTX_ERR_INVALID_ARG, "NULL output");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    HIP_TRY(rtxd::launch_counts(a->closed_at(), d_counts, a->region.width, a->rows, a->tile_w_log2, a->n,
                                (hipStream_t)hip_stream));
    return RTX_OK;
}

int rtx_accum_sample_counts(rtx_accum* a, uint32_t* out_counts) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    const size_t bytes = (size_t)a->rows * a->region.width * sizeof(uint32_t);
    if (!out_counts && bytes) return fail(RTX_ERR_INVALID_ARG, "NULL output");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);  // the cached buffer and stream
    hipStream_t st = render_stream(a->device);
    uint32_t* cnt = static_cast<uint32_t*>(render_buffer(a->device, -6, std::max<size_t>(1, bytes)));
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", a->device);
    if (!cnt) return fail(RTX_ERR_OOM, "device buffer for a %ux%u count map", a->region.width, a->rows);
    if (int rc = wait_for_renders(a->device, st)) return rc;  // the selections ran on the passes' streams, before them
    int rc = RTX_OK;
    if (rtxd::launch_counts(a->closed_at(), cnt, a->region.width, a->rows, a->tile_w_log2, a->n, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "the count map's launch");
    if (rc == RTX_OK && bytes && copy_to_host(out_counts, cnt, bytes, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "copying the count map to the host");
    (void)hipStreamSynchronize(st);
    return rc;
}

int rtx_accum_resolve_device(rtx_accum* a, float* d_rgb, float* d_var, float rel_tol, void* hip_stream, uint64_t* noisy) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (!d_rgb && (uint64_t)a->rows * a->region.width) return fail(RTX_ERR_INVALID_ARG, "NULL output");
    if (a->n == 0) return fail(RTX_ERR_INVALID_ARG, "nothing accumulated yet");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    return accum_resolve_locked(a, d_rgb, d_var, rel_tol, (hipStream_t)hip_stream, noisy);
}

int rtx_accum_resolve(rtx_accum* a, float* out_rgb, float* out_var, float rel_tol, uint64_t* noisy) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    const size_t bytes = (size_t)a->rows * a->region.width * 3 * sizeof(float);
    if (!out_rgb && !noisy) return fail(RTX_ERR_INVALID_ARG, "NULL output");  // (out_rgb NULL: the count alone)
    if (a->n == 0) return fail(RTX_ERR_INVALID_ARG, "nothing accumulated yet");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);  // the cached image buffers and stream
    hipStream_t st = render_stream(a->device);
    float* rgb = static_cast<float*>(render_buffer(a->device, -3, std::max<size_t>(1, bytes)));
    float* var = out_var ? static_cast<float*>(render_buffer(a->device, -5, std::max<size_t>(1, bytes))) : nullptr;
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", a->device);
    if (!rgb || (out_var && !var)) return fail(RTX_ERR_OOM, "device buffers for a %ux%u resolve", a->region.width, a->rows);
    // the passes may have run on any stream: every render on the device precedes the resolve (scr->last)
    if (int rc = wait_for_renders(a->device, st)) return rc;
    int rc = accum_resolve_locked(a, rgb, var, rel_tol, st, noisy);
    if (rc == RTX_OK && bytes && out_rgb && copy_to_host(out_rgb, rgb, bytes, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "copying the resolved image to the host");
    if (rc == RTX_OK && bytes && out_var && copy_to_host(out_var, var, bytes, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "copying the variance to the host");
    (void)hipStreamSynchronize(st);
    return rc;
}

int rtx_accum_ppm(rtx_accum* a, char* out_text, uint64_t capacity, uint64_t* out_len) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (!out_text || !out_len) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (a->n == 0) return fail(RTX_ERR_INVALID_ARG, "nothing accumulated yet");
    if (int rc = accum_device(a)) return rc;
    const uint32_t W = a->region.width, H = a->rows;
    const uint64_t need = rtxd::ppm_max_bytes(W, H);
    std::lock_guard<std::mutex> lk(a->scene->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);
    hipStream_t st = render_stream(a->device);
    float* rgb = static_cast<float*>(render_buffer(a->device, -3, std::max<size_t>(1, (size_t)W * H * 3 * sizeof(float))));
    char* text = static_cast<char*>(render_buffer(a->device, -4, need));
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", a->device);
    if (!rgb || !text) return fail(RTX_ERR_OOM, "device buffers for a %ux%u PPM", W, H);
    if (int rc = wait_for_renders(a->device, st)) return rc;
    const int rc = accum_resolve_locked(a, rgb, nullptr, 0.0f, st, nullptr);
    return ppm_to_host(rc, rgb, W, H, text, st, out_text, capacity, out_len);
}

int rtx_accum_preview_device(rtx_accum* a, uint32_t guide_samples, const rtx_denoise_params* params, float* d_out,
                             void* hip_stream) {
    g_last_error.clear();
    rtx_denoise_params dflt;
    if (int rc = check_preview(a, guide_samples, &params, &dflt)) return rc;
    if (!d_out && (uint64_t)a->rows * a->region.width) return fail(RTX_ERR_INVALID_ARG, "NULL output");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    return accum_preview_locked(a, guide_samples, params, d_out, (hipStream_t)hip_stream);
}

int rtx_accum_preview(rtx_accum* a, uint32_t guide_samples, const rtx_denoise_params* params, float* out_rgb) {
    g_last_error.clear();
    rtx_denoise_params dflt;
    if (int rc = check_preview(a, guide_samples, &params, &dflt)) return rc;
    const size_t bytes = (size_t)a->rows * a->region.width * 3 * sizeof(float);
    if (!out_rgb && bytes) return fail(RTX_ERR_INVALID_ARG, "NULL output");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);  // the cached image buffer and stream
    hipStream_t st = render_stream(a->device);
    float* rgb = static_cast<float*>(render_buffer(a->device, -3, std::max<size_t>(1, bytes)));
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", a->device);
    if (!rgb) return fail(RTX_ERR_OOM, "device buffer for a %ux%u preview", a->region.width, a->rows);
    if (int rc = wait_for_renders(a->device, st)) return rc;
    int rc = accum_preview_locked(a, guide_samples, params, rgb, st);
    if (rc == RTX_OK && bytes && copy_to_host(out_rgb, rgb, bytes, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "copying the preview to the host");
    (void)hipStreamSynchronize(st);
    return rc;
}

int rtx_accum_preview_ppm(rtx_accum* a, uint32_t guide_samples, const rtx_denoise_params* params, char* out_text,
                          uint64_t capacity, uint64_t* out_len) {
    g_last_error.clear();
    rtx_denoise_params dflt;
    if (int rc = check_preview(a, guide_samples, &params, &dflt)) return rc;
    if (!out_text || !out_len) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = accum_device(a)) return rc;
    const uint32_t W = a->region.width, H = a->rows;
    const uint64_t need = rtxd::ppm_max_bytes(W, H);
    std::lock_guard<std::mutex> lk(a->scene->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);
    hipStream_t st = render_stream(a->device);
    float* rgb = static_cast<float*>(render_buffer(a->device, -3, std::max<size_t>(1, (size_t)W * H * 3 * sizeof(float))));
    char* text = static_cast<char*>(render_buffer(a->device, -4, need));
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", a->device);
    if (!rgb || !text) return fail(RTX_ERR_OOM, "device buffers for a %ux%u PPM", W, H);
    if (int rc = wait_for_renders(a->device, st)) return rc;
    const int rc = accum_preview_locked(a, guide_samples, params, rgb, st);
    return ppm_to_host(rc, rgb, W, H, text, st, out_text, capacity, out_len);
}

int rtx_accum_reset(rtx_accum* a) {
    g_last_error.clear();
    if (!a) return fail(RTX_ERR_INVALID_ARG, "NULL accumulator");
    if (int rc = accum_device(a)) return rc;
    std::lock_guard<std::mutex> lk(a->scene->mu);
    HIP_TRY(hipDeviceSynchronize());  // passes and resolves in flight, on any stream
    HIP_TRY(zero_now(a->sums.ptr, a->sums.bytes));
    HIP_TRY(zero_now(a->adapt.ptr, a->adapt.bytes));  // every tile open again
    a->adaptive = false;
    a->direct = false;
    a->mis = false;
    a->n = 0;
    return RTX_OK;
}

void rtx_accum_destroy(rtx_accum* a) {
    if (!a) return;
    {
        DeviceGuard on(a->device);
        if (on.error() == hipSuccess) {
            (void)hipDeviceSynchronize();
            a->sums.release();
            a->noisy.release();
            a->preview.release();
            a->adapt.release();
        }
    }
    delete a;
}

}  // extern "C"
