// rtx_batch.hip — what the batch entry points share (rtx_trace_capi.hip, rtx_shade_capi.hip, rtx_guides_capi.hip,
// rtx_direct_capi.hip; declared in rtx_internal.h).
#include <limits>
#include <string>

#include "rtx_internal.h"

namespace rtxh {

int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

int current_copy(rtx_scene* s, DeviceCopy** out, int* device) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const auto it = s->copies.find(cur);
    if (it == s->copies.end()) return fail(RTX_ERR_INVALID_ARG, "the scene has no copy on the current device %d", cur);
    *out = it->second.get();
    if (device) *device = cur;
    return RTX_OK;
}

int Probe::ensure(uint32_t slots) {
    HIP_TRY(counters.reserve(slots * sizeof(unsigned long long)));
    if (!ev0) HIP_TRY(hipEventCreate(&ev0));
    if (!ev1) HIP_TRY(hipEventCreate(&ev1));
    return RTX_OK;
}

int Probe::begin(bool count, bool timed, hipStream_t st) {
    if (count) HIP_TRY(hipMemsetAsync(counters.ptr, 0, counters.bytes, st));
    if (timed) HIP_TRY(hipEventRecord(ev0, st));
    return RTX_OK;
}

int Probe::end(hipStream_t st, float* ms) {
    HIP_TRY(hipEventRecord(ev1, st));
    HIP_TRY(hipEventSynchronize(ev1));
    HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
    return RTX_OK;
}

int Probe::read(unsigned long long* h, uint32_t n) {
    HIP_TRY(hipMemcpy(h, counters.ptr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RTX_OK;
}

void Probe::release() {
    counters.release();
    for (hipEvent_t* ev : {&ev0, &ev1}) {
        if (*ev) (void)hipEventDestroy(*ev);
        *ev = nullptr;
    }
}

int check_batch(const rtx_scene* s, uint32_t flags, uint32_t allowed, const char* feature, uint64_t n, size_t record_bytes,
                std::initializer_list<BatchArg> args, bool* empty) {
    *empty = false;
    if (!s) return fail(RTX_ERR_INVALID_ARG, "NULL scene");
    if (flags & ~allowed) return fail(RTX_ERR_INVALID_ARG, "unknown %s flags 0x%x", feature, flags & ~allowed);
    if (n == 0) {
        *empty = true;
        return RTX_OK;
    }
    uintptr_t bits = 0;
    std::string names;
    for (const BatchArg& a : args) {
        if (!a.ptr) return fail(RTX_ERR_INVALID_ARG, "NULL argument (%s)", a.name);
        bits |= (uintptr_t)a.ptr;
        names += names.empty() ? "" : ", ";
        names += a.name;
    }
    if (bits & 15u) return fail(RTX_ERR_INVALID_ARG, "%s must be aligned to 16 B", names.c_str());
    if (n > (uint64_t)std::numeric_limits<size_t>::max() / record_bytes) return fail(RTX_ERR_INVALID_ARG, "too many records");
    return RTX_OK;
}

int check_sample_range(uint32_t first, uint32_t count) {
    if ((uint64_t)first + count > 0xFFFFFFFFull)
        return fail(RTX_ERR_INVALID_ARG, "samples %u + %u pass 2^32 - 1 (the RNG's sample word is 32-bit)", first, count);
    return RTX_OK;
}

rtxd::Shard shard_of(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first, uint32_t count) {
    rtxd::Shard sh{};
    sh.cam = *cam;
    sh.seed = seed;
    sh.x0 = region->x0;
    sh.y0 = region->y0;
    sh.width = region->width;
    sh.rows = region_rows(region);
    sh.rank = region->rank;
    sh.world = region->world;
    sh.stripe_log2 = region->stripe > 1u ? (uint32_t)(31 - __builtin_clz(region->stripe)) : 0u;
    sh.k0 = first;
    sh.kn = count;
    return sh;
}

rtxd::WalkScene walk_scene(const rtx_scene* s, const DeviceLayout* lay) {
    return rtxd::WalkScene{lay->entries.as<const float4>(), lay->n_entries, (uint32_t)(s->quadtab.size() / 16), lay->start,
                           lay->prim_end};
}

}  // namespace rtxh
