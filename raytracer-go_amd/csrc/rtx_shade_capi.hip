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
    return check_batch(s, flags, SHADE_FLAGS, "shade", n, sizeof(rtx_bounce),
                       {{rays, "rays"}, {hits, "hits"}, {keys, "keys"}, {out, "bounces"}}, empty);
}

// The checks of both camera-ray entries, none of which needs a device.  *records: count * the shard's pixels (0:
// nothing to do).
int check_camera_rays(const rtx_camera* cam, const rtx_region* region, uint32_t first_sample, uint32_t count,
                      const void* rays, const void* keys, uint64_t* records) {
    *records = 0;
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_region(cam, region)) return rc;
    if (int rc = check_sample_range(first_sample, count)) return rc;
    const uint64_t P = (uint64_t)region_rows(region) * region->width;
    if (count == 0 || P == 0) return RTX_OK;
    if (!rays) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)rays | (uintptr_t)keys) & 15u) return fail(RTX_ERR_INVALID_ARG, "rays and keys must be aligned to 16 B");
    if (P > (uint64_t)std::numeric_limits<size_t>::max() / sizeof(rtx_ray) / count) return fail(RTX_ERR_INVALID_ARG, "too many rays");
    *records = P * count;
    return RTX_OK;
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
    p.shard = shard_of(cam, seed, region, first_sample, count);
    const uint64_t P = (uint64_t)p.shard.rows * p.shard.width;
    // samples per launch: the grid's second dimension, and 32-bit ray indices (RTX_CAMERA_LAUNCH_RAYS: tests of the cut)
    const uint64_t max_rays = env_knob("RTX_CAMERA_LAUNCH_RAYS", (long)rtxd::SHADE_LAUNCH_MAX, 1, (long)rtxd::SHADE_LAUNCH_MAX);
    const uint32_t per_launch =
        (uint32_t)std::min<uint64_t>(rtxd::CAMERA_LAUNCH_SAMPLES, std::max<uint64_t>(1, max_rays / P));
    return for_launches(count, per_launch, [&](uint64_t done, uint32_t kn) {
        p.shard.k0 = first_sample + (uint32_t)done;
        p.shard.kn = kn;
        p.rays = d_rays + done * P;
        p.keys = d_keys ? d_keys + done * P : nullptr;
        const hipError_t e = rtxd::launch_camera_rays(p, (hipStream_t)hip_stream);
        return e == hipSuccess ? RTX_OK : hip_fail(e, "camera-ray launch failed");
    });
}

int rtx_camera_rays(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample, uint32_t count,
                    rtx_ray* rays, rtx_path_key* keys) {
    g_last_error.clear();
    uint64_t records = 0;
    if (int rc = check_camera_rays(cam, region, first_sample, count, rays, keys, &records)) return rc;
    if (records == 0) return RTX_OK;
    rtxd::Staging st({{rays, (size_t)records * sizeof(rtx_ray), rtxd::Stage::out},
                      {keys, (size_t)records * sizeof(rtx_path_key), rtxd::Stage::out}});
    return run_staged(st, "rtx_camera_rays' buffers", [&] {
        return rtx_camera_rays_device(cam, seed, region, first_sample, count, st.dev<rtx_ray>(0), st.dev<rtx_path_key>(1), nullptr);
    });
}

int rtx_shade_device(rtx_scene* s, uint64_t seed, const rtx_ray* d_rays, const rtx_hit* d_hits, const rtx_path_key* d_keys,
                     uint64_t n, rtx_bounce* d_out, uint32_t flags, void* hip_stream, rtx_shade_stats* stats) {
    g_last_error.clear();
    bool empty = false;
    if (int rc = check_shade(s, d_rays, d_hits, d_keys, n, d_out, flags, &empty)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (empty) return RTX_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    DeviceCopy* c = nullptr;
    if (int rc = current_copy(s, &c)) return rc;
    // (its own counters and events: a counting shade changes no render's and no trace's stats)
    if (int rc = c->shade.ensure(rtxd::SHADE_COUNTER_SLOTS)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool count = stats && (flags & RTX_SHADE_COUNTERS);
    rtxd::ShadeParams p;
    std::memset(&p, 0, sizeof(p));
    p.materials = c->materials.as<const rtx_material>();
    p.textures = c->textures.as<const rtx_texture>();
    p.texels = c->texels.as<const uint32_t>();
    p.n_materials = (uint32_t)s->materials.size();
    p.seed = seed;
    p.counters = c->shade.slots();
    // records per launch (32-bit record indices; RTX_SHADE_LAUNCH_RECORDS: tests of the cut)
    const uint64_t per_launch = env_knob("RTX_SHADE_LAUNCH_RECORDS", (long)rtxd::SHADE_LAUNCH_MAX, 64, (long)rtxd::SHADE_LAUNCH_MAX);
    if (int rc = c->shade.begin(count, stats != nullptr, stream)) return rc;
    if (int rc = for_launches(n, per_launch, [&](uint64_t off, uint32_t m) {
            p.rays = d_rays + off;
            p.hits = d_hits + off;
            p.keys = d_keys + off;
            p.out = d_out + off;
            p.n = m;
            const hipError_t e = rtxd::launch_shade(p, count, s->has_noise, stream);
            return e == hipSuccess ? RTX_OK : hip_fail(e, "shade launch failed");
        }))
        return rc;
    if (!stats) return RTX_OK;
    float ms = 0.0f;
    if (int rc = c->shade.end(stream, &ms)) return rc;
    stats->n = n;
    stats->kernel_ms = ms;
    if (count) {
        unsigned long long h[rtxd::SHADE_COUNTER_SLOTS] = {0};
        if (int rc = c->shade.read(h, rtxd::SHADE_COUNTER_SLOTS)) return rc;
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
    const size_t N = (size_t)n;
    rtxd::Staging st({{rays, N * sizeof(rtx_ray), rtxd::Stage::in},
                      {hits, N * sizeof(rtx_hit), rtxd::Stage::in},
                      {keys, N * sizeof(rtx_path_key), rtxd::Stage::in},
                      {out, N * sizeof(rtx_bounce), rtxd::Stage::out}});
    rtx_shade_stats local;
    // (with stats: the device entry returns after the kernels; without the caller's, the timed kernel)
    if (int rc = run_staged(st, "rtx_shade's buffers", [&] {
            return rtx_shade_device(s, seed, st.dev<rtx_ray>(0), st.dev<rtx_hit>(1), st.dev<rtx_path_key>(2), n,
                                    st.dev<rtx_bounce>(3), stats ? flags : flags & ~RTX_SHADE_COUNTERS, nullptr, &local);
        }))
        return rc;
    if (stats) *stats = local;
    return RTX_OK;
}

}  // extern "C"
