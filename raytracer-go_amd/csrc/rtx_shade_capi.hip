// rtx_shade_capi.hip — path building blocks (rtx.h): the entry points around rtx_shade.hip's kernels.
#include <algorithm>
#include <cstring>
#include <limits>

#include "rtx_internal.h"
#include "rtx_shade.h"

using namespace rtxh;

namespace {

constexpr uint32_t SHADE_FLAGS = RTX_SHADE_COUNTERS;

// The checks of both shade entries that need no device.  *empty: nothing to do (n == 0).
int check_shade(const rtx_scene* s, const void* rays, const void* hits, const void* keys, uint64_t n, const void* out,
                uint32_t flags, bool* empty) {
    *empty = false;
    if (!s) return fail(RTX_ERR_INVALID_ARG, "NULL scene");
    if (flags & ~SHADE_FLAGS) return fail(RTX_ERR_INVALID_ARG, "unknown shade flags 0x%x", flags & ~SHADE_FLAGS);
    if (n == 0) {
        *empty = true;
        return RTX_OK;
    }
    if (!rays || !hits || !keys || !out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)rays | (uintptr_t)hits | (uintptr_t)keys | (uintptr_t)out) & 15u)
        return fail(RTX_ERR_INVALID_ARG, "rays, hits, keys and bounces must be aligned to 16 B");
    if (n > (uint64_t)std::numeric_limits<size_t>::max() / sizeof(rtx_bounce)) return fail(RTX_ERR_INVALID_ARG, "too many records");
    return RTX_OK;
}

// The checks of both camera-ray entries, none of which needs a device.  *records: count * the shard's pixels (0:
// nothing to do).
int check_camera_rays(const rtx_camera* cam, const rtx_region* region, uint32_t first_sample, uint32_t count,
                      const void* rays, const void* keys, uint64_t* records) {
    *records = 0;
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_region(cam, region)) return rc;
    if ((uint64_t)first_sample + count > 0xFFFFFFFFull)
        return fail(RTX_ERR_INVALID_ARG, "samples %u + %u pass 2^32 - 1 (the RNG's sample word is 32-bit)", first_sample, count);
    const uint64_t P = (uint64_t)region_rows(region) * region->width;
    if (count == 0 || P == 0) return RTX_OK;
    if (!rays) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)rays | (uintptr_t)keys) & 15u) return fail(RTX_ERR_INVALID_ARG, "rays and keys must be aligned to 16 B");
    if (P > (uint64_t)std::numeric_limits<size_t>::max() / sizeof(rtx_ray) / count) return fail(RTX_ERR_INVALID_ARG, "too many rays");
    *records = P * count;
    return RTX_OK;
}

// A shade's counters and events on copy c (s->mu held, current device = c's), made on first use: its own, so that a
// counting shade changes no render's and no trace's stats.
int ensure_shade(DeviceCopy* c) {
    HIP_TRY(c->shade_counters.reserve(rtxd::SHADE_COUNTER_SLOTS * sizeof(unsigned long long)));
    if (!c->sev0) HIP_TRY(hipEventCreate(&c->sev0));
    if (!c->sev1) HIP_TRY(hipEventCreate(&c->sev1));
    return RTX_OK;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int rtx_camera_rays_device(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                           uint32_t count, rtx_ray* d_rays, rtx_path_key* d_keys, void* hip_stream) {
    g_last_error.clear();
    uint64_t records = 0;
    if (int rc = check_camera_rays(cam, region, first_sample, count, d_rays, d_keys, &records)) return rc;
    if (records == 0) return RTX_OK;
    rtxd::CameraRayParams p;
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
    const uint64_t P = (uint64_t)p.rows * p.width;
    // samples per launch: the grid's second dimension, and 32-bit ray indices (RTX_CAMERA_LAUNCH_RAYS: tests of the cut)
    const uint64_t max_rays = env_knob("RTX_CAMERA_LAUNCH_RAYS", (long)rtxd::SHADE_LAUNCH_MAX, 1, (long)rtxd::SHADE_LAUNCH_MAX);
    const uint32_t per_launch =
        (uint32_t)std::min<uint64_t>(rtxd::CAMERA_LAUNCH_SAMPLES, std::max<uint64_t>(1, max_rays / P));
    for (uint32_t done = 0; done < count; done += per_launch) {
        p.k0 = first_sample + done;
        p.kn = std::min(per_launch, count - done);
        p.rays = d_rays + (uint64_t)done * P;
        p.keys = d_keys ? d_keys + (uint64_t)done * P : nullptr;
        if (const hipError_t e = rtxd::launch_camera_rays(p, (hipStream_t)hip_stream)) return hip_fail(e, "camera-ray launch failed");
    }
    return RTX_OK;
}

int rtx_camera_rays(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample, uint32_t count,
                    rtx_ray* rays, rtx_path_key* keys) {
    g_last_error.clear();
    uint64_t records = 0;
    if (int rc = check_camera_rays(cam, region, first_sample, count, rays, keys, &records)) return rc;
    if (records == 0) return RTX_OK;
    DeviceBuffer d_rays, d_keys;
    int rc = RTX_OK;
    hipError_t e = d_rays.reserve((size_t)records * sizeof(rtx_ray));
    if (e == hipSuccess && keys) e = d_keys.reserve((size_t)records * sizeof(rtx_path_key));
    if (e == hipSuccess) {
        rc = rtx_camera_rays_device(cam, seed, region, first_sample, count, d_rays.as<rtx_ray>(),
                                    keys ? d_keys.as<rtx_path_key>() : nullptr, nullptr);
        // (blocking copies on the null stream: after the kernels)
        if (rc == RTX_OK) e = hipMemcpy(rays, d_rays.ptr, (size_t)records * sizeof(rtx_ray), hipMemcpyDeviceToHost);
        if (rc == RTX_OK && e == hipSuccess && keys)
            e = hipMemcpy(keys, d_keys.ptr, (size_t)records * sizeof(rtx_path_key), hipMemcpyDeviceToHost);
    }
    d_rays.release();
    d_keys.release();
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "rtx_camera_rays' buffers");
    return RTX_OK;
}

int rtx_shade_device(rtx_scene* s, uint64_t seed, const rtx_ray* d_rays, const rtx_hit* d_hits, const rtx_path_key* d_keys,
                     uint64_t n, rtx_bounce* d_out, uint32_t flags, void* hip_stream, rtx_shade_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_shade(s, d_rays, d_hits, d_keys, n, d_out, flags, &empty)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (empty) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const auto it = s->copies.find(cur);
    if (it == s->copies.end()) return fail(RTX_ERR_INVALID_ARG, "the scene has no copy on the current device %d", cur);
    DeviceCopy* c = it->second.get();
    if (int rc = ensure_shade(c)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_SHADE_COUNTERS);
    rtxd::ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.materials = c->materials.as<const rtx_material>();
    p.textures = c->textures.as<const rtx_texture>();
    p.texels = c->texels.as<const uint32_t>();
    p.n_materials = (uint32_t)s->materials.size();
    p.seed = seed;
    p.counters = c->shade_counters.as<unsigned long long>();
    // records per launch (32-bit record indices; RTX_SHADE_LAUNCH_RECORDS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_SHADE_LAUNCH_RECORDS", (long)rtxd::SHADE_LAUNCH_MAX, 64, (long)rtxd::SHADE_LAUNCH_MAX);
    if (count) HIP_TRY(hipMemsetAsync(c->shade_counters.ptr, 0, c->shade_counters.bytes, stream));
    if (stats) HIP_TRY(hipEventRecord(c->sev0, stream));
    for (uint64_t off = 0; off < n; off += per_launch) {
        p.rays = d_rays + off;
        p.hits = d_hits + off;
        p.keys = d_keys + off;
        p.out = d_out + off;
        p.n = (uint32_t)std::min<uint64_t>(per_launch, n - off);
        if (const hipError_t e = rtxd::launch_shade(p, count, s->has_noise, stream)) return hip_fail(e, "shade launch failed");
    }
    if (!stats) return RTX_OK;
    HIP_TRY(hipEventRecord(c->sev1, stream));
    HIP_TRY(hipEventSynchronize(c->sev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->sev0, c->sev1));
    stats->n = n;
    stats->kernel_ms = ms;
    if (count) {
        unsigned long long h[rtxd::SHADE_COUNTER_SLOTS] = {0};
        HIP_TRY(hipMemcpy(h, c->shade_counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
        stats->hits = h[rtxd::SHADE_HITS];
        stats->scattered = h[rtxd::SHADE_SCATTERED];
        stats->rng_draws = h[rtxd::SHADE_RNG_DRAWS];
        stats->texel_fetches = h[rtxd::SHADE_TEXEL_FETCHES];
    }
    return RTX_OK;
}

int rtx_shade(rtx_scene* s, uint64_t seed, const rtx_ray* rays, const rtx_hit* hits, const rtx_path_key* keys, uint64_t n,
              rtx_bounce* out, uint32_t flags, rtx_shade_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_shade(s, rays, hits, keys, n, out, flags, &empty)) return rc;
    if (empty) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RTX_OK;
    }
    DeviceBuffer d_rays, d_hits, d_keys, d_out;
    rtx_shade_stats local;
    int rc = RTX_OK;
    const size_t N = (size_t)n;
    hipError_t e = d_rays.reserve(N * sizeof(rtx_ray));
    if (e == hipSuccess) e = d_hits.reserve(N * sizeof(rtx_hit));
    if (e == hipSuccess) e = d_keys.reserve(N * sizeof(rtx_path_key));
    if (e == hipSuccess) e = d_out.reserve(N * sizeof(rtx_bounce));
    if (e == hipSuccess) e = hipMemcpy(d_rays.ptr, rays, N * sizeof(rtx_ray), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_hits.ptr, hits, N * sizeof(rtx_hit), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_keys.ptr, keys, N * sizeof(rtx_path_key), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // (with stats: it returns after the kernels; without the caller's, the timed kernel)
        rc = rtx_shade_device(s, seed, d_rays.as<rtx_ray>(), d_hits.as<rtx_hit>(), d_keys.as<rtx_path_key>(), n,
                              d_out.as<rtx_bounce>(), stats ? flags : flags & ~RTX_SHADE_COUNTERS, nullptr, &local);
        if (rc == RTX_OK) e = hipMemcpy(out, d_out.ptr, N * sizeof(rtx_bounce), hipMemcpyDeviceToHost);
    }
    d_rays.release();
    d_hits.release();
    d_keys.release();
    d_out.release();
    if (rc != RTX_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "rtx_shade's buffers");
    if (stats) *stats = local;
    return RTX_OK;
}

}  // extern "C"
