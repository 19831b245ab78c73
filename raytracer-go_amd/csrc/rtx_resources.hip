// rtx_resources.hip — what librtx.so keeps per device between calls: the sample scratch, the pinned host stages, the
// sticky error word, rtx_render's buffers, streams and events, and the RCCL communicators; and the entry points
// that free or check them.  Nothing here is freed at process exit (rtx_devmem.h): rtx_release_device_memory does.
#include <dlfcn.h>

#include <algorithm>
#include <cstring>

#include "rtx_internal.h"

namespace rtxh {

std::mutex g_scratch_mu;
std::map<int, Scratch> g_scratch;

std::mutex g_ppm_mu;
std::map<int, DeviceBuffer> g_ppm;

namespace {
// Two pinned host stages for copies into the caller's (pageable) buffer, allocated on first
// use and freed by rtx_release_device_memory(-1): the DMA of chunk k+1 runs while the CPU copies
// chunk k out.  (hipMemcpy into pageable memory stages through the runtime's own buffers: the
// 24.9 MB image of C2 cost ~7 ms that way.)
struct HostStage {
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
};
constexpr size_t kStageBytes = 4u << 20;
std::mutex g_stage_mu;
HostStage g_stage;

}  // namespace

hipError_t copy_to_host(void* dst, const void* src, size_t bytes, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        if (!g_stage.buf[i]) e = hipHostMalloc(&g_stage.buf[i], kStageBytes, hipHostMallocDefault);
        if (e == hipSuccess && !g_stage.ev[i]) e = hipEventCreateWithFlags(&g_stage.ev[i], hipEventDisableTiming);
    }
    const size_t n = (bytes + kStageBytes - 1) / kStageBytes;
    auto len = [&](size_t k) { return std::min(kStageBytes, bytes - k * kStageBytes); };
    for (size_t k = 0; k <= n && e == hipSuccess; ++k) {
        if (k < n) {  // chunk k into stage k % 2 (its previous chunk, k - 2, is already copied out)
            e = hipMemcpyAsync(g_stage.buf[k % 2], static_cast<const char*>(src) + k * kStageBytes, len(k),
                               hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(g_stage.ev[k % 2], st);
        }
        if (k >= 1 && e == hipSuccess) {  // chunk k - 1 out of its stage while chunk k is in flight
            e = hipEventSynchronize(g_stage.ev[(k - 1) % 2]);
            if (e == hipSuccess)
                std::memcpy(static_cast<char*>(dst) + (k - 1) * kStageBytes, g_stage.buf[(k - 1) % 2], len(k - 1));
        }
    }
    // on a failure no copy into a stage may still be in flight when the lock is released
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    return e;
}

hipError_t zero_now(void* ptr, size_t bytes) {
    const hipError_t e = hipMemsetAsync(ptr, 0, bytes, nullptr);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}

namespace {
void release_stage_locked() {
    for (int i = 0; i < 2; ++i) {
        if (g_stage.ev[i]) (void)hipEventDestroy(g_stage.ev[i]);
        if (g_stage.buf[i]) (void)hipHostFree(g_stage.buf[i]);
    }
    g_stage = HostStage{};
}

// The sticky error word of a device: rtxd::KERR_WORDS counters the kernels only add to — waves
// stopped by the watchdog, lanes of waves that found a partial wave at a claim.  No render zeroes them (the stats
// slots are zeroed by every render, so a flag there was wiped by the next render enqueued behind a failed one):
// `seen` is what the host has already reported, and a change since is the error of some render after that report.
// collect_on (every render that returns stats) and rtx_device_check (any number of renders enqueued without
// stats, e.g. a pipelined benchmark) read it.  8 bytes per device, kept for the process's life.
struct KernErr {
    DeviceBuffer d;
    uint32_t seen[rtxd::KERR_WORDS] = {0, 0};
};
std::mutex g_kerr_mu;
std::map<int, KernErr> g_kerr;

}  // namespace

// The device's word (allocated and zeroed on first use: zero when this returns, whatever stream renders next), or nullptr.
uint32_t* kerr_word(int device) {
    std::lock_guard<std::mutex> lk(g_kerr_mu);
    KernErr& k = g_kerr[device];
    if (!k.d.ptr) {
        if (k.d.reserve(rtxd::KERR_WORDS * sizeof(uint32_t)) != hipSuccess) return nullptr;
        if (zero_now(k.d.ptr, k.d.bytes) != hipSuccess) k.d.release();
    }
    return k.d.as<uint32_t>();
}

// Read the current device's word (the renders to report must have completed) and report what changed since the
// last read: RTX_OK, or RTX_ERR_HIP naming the failure.  The change is then acknowledged.
int kerr_take(int device) {
    std::lock_guard<std::mutex> lk(g_kerr_mu);
    auto it = g_kerr.find(device);
    if (it == g_kerr.end() || !it->second.d.ptr) return RTX_OK;  // nothing ever rendered on it
    KernErr& k = it->second;
    uint32_t h[rtxd::KERR_WORDS] = {0, 0};
    HIP_TRY(hipMemcpy(h, k.d.ptr, sizeof(h), hipMemcpyDeviceToHost));
    const uint32_t wd = h[rtxd::KERR_WATCHDOG] - k.seen[rtxd::KERR_WATCHDOG];
    const uint32_t pw = h[rtxd::KERR_PARTIAL_WAVE] - k.seen[rtxd::KERR_PARTIAL_WAVE];
    std::memcpy(k.seen, h, sizeof(h));
    if (pw)
        return fail(RTX_ERR_HIP, "render kernel: a wave-level claim was reached without the whole wave (partial EXEC; "
                                 "%u lanes on device %d): output invalid", pw, device);
    if (wd)
        return fail(RTX_ERR_HIP, "render kernel watchdog fired (RTX_WATCHDOG_S; %u waves on device %d): output "
                                 "incomplete", wd, device);
    return RTX_OK;
}

// Free a device's scratch buffers (g_scratch_mu held).
void release_scratch_locked(int device) {
    auto it = g_scratch.find(device);
    if (it == g_scratch.end()) return;
    Scratch& sc = it->second;
    {
        DeviceGuard on(device);
        if (on.error() == hipSuccess) {
            if (sc.last) (void)hipEventSynchronize(sc.last);
            for (DeviceBuffer* b : {&sc.samples, &sc.defer, &sc.redo, &sc.drain}) b->release();
            if (sc.last) (void)hipEventDestroy(sc.last);
        }
    }
    const int scenes = sc.scenes;
    sc = Scratch{};
    sc.scenes = scenes;
}

int wait_for_renders(int device, hipStream_t st) {
    std::lock_guard<std::mutex> sl(g_scratch_mu);
    Scratch& scr = g_scratch[device];
    if (scr.last) HIP_TRY(hipStreamWaitEvent(st, scr.last, 0));
    return RTX_OK;
}

// ---- RCCL, loaded on first use (rtx_render with n_gpus > 1) --------------------------
std::mutex g_rccl_mu;
std::map<int, std::vector<ncclComm_t>> g_comms;
namespace {
RcclApi g_rccl;
}

const RcclApi* rccl_api() {  // g_rccl_mu held
    if (g_rccl.tried) return g_rccl.ok ? &g_rccl : nullptr;
    g_rccl.tried = true;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) {
        g_rccl.err = std::string("cannot load librccl: ") + dlerror();
        return nullptr;
    }
    bool ok = true;
    auto sym = [&](auto& fn, const char* name) {
        fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
        ok = ok && fn != nullptr;
    };
    sym(g_rccl.CommInitAll, "ncclCommInitAll");
    sym(g_rccl.CommDestroy, "ncclCommDestroy");
    sym(g_rccl.GroupStart, "ncclGroupStart");
    sym(g_rccl.GroupEnd, "ncclGroupEnd");
    sym(g_rccl.Gather, "ncclGather");
    sym(g_rccl.GetErrorString, "ncclGetErrorString");
    if (!ok) g_rccl.err = "librccl lacks ncclGather / ncclCommInitAll";
    g_rccl.ok = ok;
    return ok ? &g_rccl : nullptr;
}

namespace {
void release_comms_locked() {  // g_rccl_mu held
    for (auto& kv : g_comms)
        for (ncclComm_t c : kv.second)
            if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
    g_comms.clear();
}

std::map<std::pair<int, int>, DeviceBuffer> g_render_bufs;
std::map<int, hipStream_t> g_render_streams;
std::map<std::pair<int, int>, hipEvent_t> g_render_events;
}  // namespace
std::mutex g_render_mu;

void* render_buffer(int device, int slot, size_t bytes) {
    DeviceBuffer& b = g_render_bufs[{device, slot}];
    return b.reserve(bytes) == hipSuccess ? b.ptr : nullptr;
}
hipStream_t render_stream(int device) {  // current device = device
    hipStream_t& st = g_render_streams[device];
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;
    return st;
}
hipEvent_t render_event(int device, int k) {  // current device = device
    hipEvent_t& ev = g_render_events[{device, k}];
    if (!ev && hipEventCreate(&ev) != hipSuccess) ev = nullptr;
    return ev;
}

namespace {
// Erase from a map keyed by device (or by (device, slot)) the entries of `device` (-1: all), each freed by `free`
// with its device current; entries whose device cannot be set stay.
template <class Map, class Free>
void release_of(Map& m, int device, Free free) {
    auto dev_of = [](const auto& key) {
        if constexpr (std::is_same_v<std::decay_t<decltype(key)>, int>) return key;
        else return key.first;
    };
    for (auto it = m.begin(); it != m.end();) {
        const int dv = dev_of(it->first);
        if ((device < 0 || dv == device) && hipSetDevice(dv) == hipSuccess) {
            free(it->second);
            it = m.erase(it);
        } else {
            ++it;
        }
    }
}
void release_render_locked(int device) {  // g_render_mu held; device -1: all
    DeviceGuard restore;
    release_of(g_render_bufs, device, [](DeviceBuffer& b) {
        (void)hipDeviceSynchronize();
        b.release();
    });
    release_of(g_render_streams, device, [](hipStream_t st) {
        if (st) (void)hipStreamDestroy(st);
    });
    release_of(g_render_events, device, [](hipEvent_t ev) {
        if (ev) (void)hipEventDestroy(ev);
    });
}
}  // namespace

}  // namespace rtxh

using namespace rtxh;

extern "C" {

int rtx_release_device_memory(int device) {
    g_last_error.clear();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    if (device < -1 || device >= ndev) return fail(RTX_ERR_INVALID_ARG, "device %d of %d", device, ndev);
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        for (auto& kv : g_scratch)
            if (device < 0 || kv.first == device) release_scratch_locked(kv.first);
    }
    {
        std::lock_guard<std::mutex> lk(g_ppm_mu);
        DeviceGuard restore;
        for (auto& kv : g_ppm)
            if ((device < 0 || kv.first == device) && hipSetDevice(kv.first) == hipSuccess) kv.second.release();
    }
    if (device < 0) {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        release_stage_locked();
    }
    {
        std::lock_guard<std::mutex> lk(g_render_mu);
        release_render_locked(device);
    }
    {  // communicators span devices 0..n-1: any release drops them all
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        release_comms_locked();
    }
    return RTX_OK;
}

int rtx_device_check(int device) {
    g_last_error.clear();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(RTX_ERR_INVALID_ARG, "device %d of %d", device, ndev);
    DeviceGuard on(device);
    HIP_TRY(on.error());
    const hipError_t e = hipDeviceSynchronize();  // every render enqueued on the device has ended
    return e == hipSuccess ? kerr_take(device)
                           : fail(RTX_ERR_HIP, "hipDeviceSynchronize(%d): %s", device, hipGetErrorString(e));
}

uint64_t rtx_device_scratch_bytes(int device) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    auto it = g_scratch.find(device);
    return it == g_scratch.end() ? 0 : (uint64_t)it->second.samples.bytes;
}

}  // extern "C"
