// rtx_bands.hip — rtx_render / rtx_render_ex: the image in bands, one per device, and their assembly on device 0
// (an RCCL gather, device copies of simulated bands, or per-band copies into the caller's rows).
#include <algorithm>
#include <cstring>

#include "rtx_internal.h"

namespace {

// rtx_render's band assembly on device 0: the RCCL-gathered bands g[d][r][:] (n bands
// of R rows, row_floats = 3 W floats each; band d holds image rows y = d + r n) -> img[y][:].
__global__ __launch_bounds__(256) void deinterleave_bands(const float* __restrict__ g, float* __restrict__ img,
                                                          uint32_t n, uint32_t R, uint32_t H, uint32_t row_floats,
                                                          uint32_t S) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)H * row_floats) return;
    const uint32_t y = (uint32_t)(i / row_floats), x = (uint32_t)(i % row_floats);
    const uint32_t st = y / S, d = st % n, lr = (st / n) * S + y % S;  // stripe st of band d: its row lr
    img[i] = g[((uint64_t)d * R + lr) * row_floats + x];
}

}  // namespace

namespace rtxh {

namespace {

// The bands of one render: band d (the stripes d, d + n, ... of S rows each) renders on device dev_of(d).
struct Bands {
    int n = 0;
    uint32_t sim = 1;  // RTX_SIM_BANDS=k (tests, one device): k bands, all on device 0, gathered by device copies
    uint32_t kflags = 0;
    uint32_t W = 0, H = 0;
    uint32_t S = 0;  // rows per stripe (single rows unless RTX_STRIPE says otherwise)
    uint32_t R = 0;  // rows of band 0, the longest: every band is sent padded to R
    size_t band_floats = 0, band_bytes = 0, img_bytes = 0;
    std::vector<float*> bufs;
    std::vector<hipStream_t> streams;
    std::vector<rtx_region> regs;
    std::vector<uint32_t> chunks;
    int dev_of(int d) const { return sim > 1 ? 0 : d; }
};

// 1. Each band (rows y % n == d) renders on its device, the devices concurrently.
int enqueue_bands(rtx_scene* s, const rtx_camera* cam, uint64_t seed, Bands& b, rtx_stats* total, bool* tiered) {
    for (int d = 0; d < b.n; ++d) {
        const int dv = b.dev_of(d);
        DeviceCopy* c = nullptr;
        if (int rc = ensure_device(s, dv, &c)) return rc;
        if (hipSetDevice(dv) != hipSuccess) return fail(RTX_ERR_HIP, "hipSetDevice(%d)", dv);
        b.regs[d] = rtx_region{0, 0, b.W, b.H, (uint32_t)d, (uint32_t)b.n, b.S};
        if (!(b.streams[d] = render_stream(dv))) return fail(RTX_ERR_HIP, "stream on device %d", dv);
        if (!(b.bufs[d] = static_cast<float*>(render_buffer(dv, d, b.band_bytes))))
            return fail(RTX_ERR_OOM, "hipMalloc band %zu B", b.band_bytes);
        if (int rc = enqueue_on(s, c, cam, seed, &b.regs[d], b.bufs[d], b.streams[d], b.kflags, true, &b.chunks[d], tiered))
            return rc;
        if (b.sim > 1) {  // simulated bands share device 0's counters and events: read each now
            rtx_stats st;
            const uint64_t samples = (uint64_t)region_rows(&b.regs[d]) * b.W * cam->samples_per_pixel;
            if (int rc = collect_on(c, b.kflags != 0, samples, b.chunks[d], &st)) return rc;
            add_stats(total, st);
        }
    }
    return RTX_OK;
}

// 2. Wait for every band (and read its counters), so gather_ms times only the gather.
int collect_bands(rtx_scene* s, const rtx_camera* cam, const Bands& b, rtx_stats* total) {
    for (int d = 0; d < b.n && b.sim == 1; ++d) {
        if (hipSetDevice(d) != hipSuccess) return fail(RTX_ERR_HIP, "hipSetDevice(%d)", d);
        rtx_stats st;
        const uint64_t samples = (uint64_t)region_rows(&b.regs[d]) * b.W * cam->samples_per_pixel;
        if (int rc = collect_on(s->copies[d].get(), b.kflags != 0, samples, b.chunks[d], &st)) return rc;
        add_stats(total, st);
    }
    return RTX_OK;
}

// 3. Assemble on device 0: the padded bands gathered (one ncclGather over xGMI, or device
//    copies of simulated bands), de-interleaved by a kernel, copied into the caller's buffer;
//    or, without RCCL, each band's rows copied straight into the caller's rows.
//    rl: g_rccl_mu, taken here for an RCCL gather and held by the caller until the render's end.
int assemble_bands(const Bands& b, float* out_rgb, float** dev_img, std::unique_lock<std::mutex>& rl, rtx_stats* total) {
    const int n = b.n;
    const uint32_t W = b.W, H = b.H, S = b.S;
    const std::vector<float*>& bufs = b.bufs;
    const std::vector<hipStream_t>& streams = b.streams;
    // the gather: RCCL for more than one device (RTX_FORCE_RCCL=1: also for one, a 1-rank gather);
    // per-band copies into the caller's rows when RCCL is unavailable or fails (RTX_NO_RCCL=1: always)
    const bool want_rccl = b.sim == 1 && (n > 1 || env_knob("RTX_FORCE_RCCL", 0, 0, 1) == 1);
    const bool no_rccl = env_knob("RTX_NO_RCCL", 0, 0, 1) == 1;
    uint32_t kind = n == 1 && !want_rccl ? RTX_GATHER_NONE : (b.sim > 1 ? RTX_GATHER_DEVICE : RTX_GATHER_RCCL);
    std::vector<ncclComm_t>* comms = nullptr;
    const RcclApi* api = nullptr;
    if (kind == RTX_GATHER_RCCL) {
        rl.lock();
        api = no_rccl ? nullptr : rccl_api();
        if (api) {
            auto it = g_comms.find(n);
            if (it == g_comms.end()) {
                std::vector<ncclComm_t> cs(n, nullptr);
                std::vector<int> devs(n);
                for (int d = 0; d < n; ++d) devs[d] = d;
                if (api->CommInitAll(cs.data(), n, devs.data()) == ncclSuccess) it = g_comms.emplace(n, cs).first;
            }
            if (it != g_comms.end()) comms = &it->second;
        }
        if (!comms) kind = RTX_GATHER_HOST;  // RCCL unavailable: per-band copies
    }
    if (b.sim > 1 && no_rccl) kind = RTX_GATHER_HOST;
    hipEvent_t g0 = nullptr, g1 = nullptr;
    if (kind != RTX_GATHER_NONE) {
        (void)hipSetDevice(0);
        g0 = render_event(0, 0);
        g1 = render_event(0, 1);
        if (!g0 || !g1 || hipEventRecord(g0, streams[0]) != hipSuccess) return fail(RTX_ERR_HIP, "gather events");
    }
    float* gathered = nullptr;
    float* img = nullptr;
    if (kind == RTX_GATHER_RCCL || kind == RTX_GATHER_DEVICE) {
        (void)hipSetDevice(0);
        gathered = static_cast<float*>(render_buffer(0, -1, (size_t)n * b.band_bytes));
        img = static_cast<float*>(render_buffer(0, -2, b.img_bytes));
        if (!gathered || !img) return fail(RTX_ERR_OOM, "device-0 buffers for the gather of %d bands", n);
    }
    if (kind == RTX_GATHER_RCCL) {
        ncclResult_t e = api->GroupStart();
        for (int d = 0; d < n && e == ncclSuccess; ++d)
            e = api->Gather(bufs[d], d == 0 ? gathered : nullptr, b.band_floats, ncclFloat, 0, (*comms)[d], streams[d]);
        const ncclResult_t e2 = api->GroupEnd();
        if (e == ncclSuccess) e = e2;
        if (e != ncclSuccess) {  // degrade to per-band copies (the bands are intact)
            for (int d = 0; d < n; ++d)
                if (hipSetDevice(d) == hipSuccess) (void)hipStreamSynchronize(streams[d]);
            (void)hipSetDevice(0);
            (void)hipEventRecord(g0, streams[0]);
            kind = RTX_GATHER_HOST;
        }
    }
    if (kind == RTX_GATHER_DEVICE) {
        for (int d = 0; d < n; ++d)
            if (hipMemcpyAsync(gathered + (size_t)d * (b.band_bytes / sizeof(float)), bufs[d], b.band_bytes,
                               hipMemcpyDeviceToDevice, streams[0]) != hipSuccess)
                return fail(RTX_ERR_HIP, "band copy %d", d);
    }
    if (kind == RTX_GATHER_RCCL || kind == RTX_GATHER_DEVICE) {
        (void)hipSetDevice(0);
        const uint64_t total_floats = (uint64_t)H * W * 3;
        hipLaunchKernelGGL(deinterleave_bands, dim3((uint32_t)((total_floats + 255) / 256)), dim3(256), 0, streams[0],
                           gathered, img, (uint32_t)n, b.R, H, W * 3, S);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(g1, streams[0]);
        if (e == hipSuccess && out_rgb) e = copy_to_host(out_rgb, img, total_floats * sizeof(float), streams[0]);
        for (int d = 1; d < n && e == hipSuccess; ++d)
            if ((e = hipSetDevice(b.dev_of(d))) == hipSuccess) e = hipStreamSynchronize(streams[d]);
        if (e != hipSuccess) return fail(RTX_ERR_HIP, "band assembly: %s", hipGetErrorString(e));
        if (!out_rgb) *dev_img = img;
    } else if (kind == RTX_GATHER_HOST) {
        // band d holds the stripes d, d + n, ... (S rows each): one strided copy per band of its whole stripes
        // into the caller's rows, the partial last stripe separately (for a device image, rows of a host image that
        // then goes to device 0 in one copy: RCCL's fallback only)
        std::vector<float> host_img(out_rgb ? 0 : (size_t)H * W * 3);
        float* dst = out_rgb ? out_rgb : host_img.data();
        const size_t row_b = (size_t)W * 3 * sizeof(float);
        int rc = RTX_OK;
        for (int d = 0; d < n && rc == RTX_OK; ++d) {
            const uint32_t rows = region_rows(&b.regs[d]);
            if (!rows) continue;
            const uint32_t full = rows / S, part = rows % S;  // whole stripes, rows of a partial last one
            hipError_t e = hipSetDevice(b.dev_of(d));
            if (e == hipSuccess && full)
                e = hipMemcpy2DAsync(dst + (size_t)d * S * W * 3, (size_t)n * S * row_b, bufs[d], S * row_b, S * row_b,
                                     full, hipMemcpyDeviceToHost, streams[d]);
            if (e == hipSuccess && part)
                e = hipMemcpyAsync(dst + (size_t)((size_t)full * n + d) * S * W * 3, bufs[d] + (size_t)full * S * W * 3,
                                   part * row_b, hipMemcpyDeviceToHost, streams[d]);
            if (e != hipSuccess) rc = fail(RTX_ERR_HIP, "band %d copy to the host", d);
        }
        for (int d = 0; d < n; ++d)
            if (hipSetDevice(b.dev_of(d)) == hipSuccess && hipStreamSynchronize(streams[d]) != hipSuccess && rc == RTX_OK)
                rc = fail(RTX_ERR_HIP, "band %d copy to the host", d);
        if (rc == RTX_OK && !out_rgb) {
            (void)hipSetDevice(0);
            if (!(img = static_cast<float*>(render_buffer(0, -2, b.img_bytes)))) rc = fail(RTX_ERR_OOM, "device-0 image");
            else if (hipMemcpyAsync(img, dst, b.img_bytes, hipMemcpyHostToDevice, streams[0]) != hipSuccess)
                rc = fail(RTX_ERR_HIP, "image copy to device 0");
            else *dev_img = img;
        }
        if (rc == RTX_OK && (hipSetDevice(0) != hipSuccess || hipEventRecord(g1, streams[0]) != hipSuccess ||
                             hipEventSynchronize(g1) != hipSuccess))
            rc = fail(RTX_ERR_HIP, "gather event");
        if (rc != RTX_OK) return rc;
    } else {  // one device, no gather: the band is the image
        (void)hipSetDevice(0);
        if (out_rgb) {
            hipError_t e = copy_to_host(out_rgb, bufs[0], b.img_bytes, streams[0]);
            if (e != hipSuccess) return fail(RTX_ERR_HIP, "copy image: %s", hipGetErrorString(e));
        } else {
            *dev_img = bufs[0];
        }
    }
    total->gather_kind = kind;
    if (kind != RTX_GATHER_NONE) {
        float ms = 0.0f;
        if (hipSetDevice(0) == hipSuccess && hipEventElapsedTime(&ms, g0, g1) == hipSuccess) total->gather_ms = ms;
    }
    return RTX_OK;
}

}  // namespace

// rtx_render_ex's bands (rows y % n == d on device d) and their assembly, with s->mu and g_render_mu
// held by the caller.  out_rgb: the caller's host buffer.  Or out_rgb == nullptr: the assembled image
// stays on device 0 in *dev_img (a cached render buffer, valid until the next render under
// g_render_mu), written by *dev_stream (rtx_render_ppm_ex encodes it there).
int render_bands_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, int n_gpus, uint32_t flags, float* out_rgb,
                        float** dev_img, hipStream_t* dev_stream, rtx_stats* stats) {
    Bands b;
    b.sim = n_gpus == 1 ? env_knob("RTX_SIM_BANDS", 1, 1, 64) : 1u;
    b.n = b.sim > 1 ? (int)b.sim : n_gpus;
    if ((uint32_t)b.n > cam->image_height) b.n = (int)cam->image_height;
    const int n = b.n;
    b.kflags = flags & RTX_FLAG_COUNTERS;
    b.W = cam->image_width;
    b.H = cam->image_height;
    b.S = band_stripe(n);
    rtx_region reg0{0, 0, b.W, b.H, 0, (uint32_t)n, b.S};
    b.R = region_rows(&reg0);
    b.band_floats = (size_t)b.R * b.W * 3;
    b.band_bytes = std::max<size_t>(b.band_floats, 1) * sizeof(float);
    b.img_bytes = (size_t)b.H * b.W * 3 * sizeof(float);
    b.bufs.assign(n, nullptr);
    b.streams.assign(n, nullptr);
    b.regs.resize(n);
    b.chunks.assign(n, 0);
    rtx_stats total;
    std::memset(&total, 0, sizeof(total));
    bool tiered = false;
    DeviceGuard restore;  // the steps set each band's device
    HIP_TRY(restore.error());
    std::unique_lock<std::mutex> rl(g_rccl_mu, std::defer_lock);
    int rc = enqueue_bands(s, cam, seed, b, &total, &tiered);
    if (rc == RTX_OK) rc = collect_bands(s, cam, b, &total);
    if (rc == RTX_OK) rc = assemble_bands(b, out_rgb, dev_img, rl, &total);
    if (rc == RTX_OK && dev_stream) *dev_stream = b.streams[0];
    for (int d = 0; d < n; ++d)  // nothing of this call still in flight when the buffers are reused
        if (b.streams[d] && hipSetDevice(b.dev_of(d)) == hipSuccess) (void)hipStreamSynchronize(b.streams[d]);
    total.walk_layout = walk_layout(s, cam, tiered);
    if (rc == RTX_OK && stats) *stats = total;
    return rc;
}

}  // namespace rtxh

using namespace rtxh;

extern "C" {

int rtx_render(rtx_scene* s, const rtx_camera* cam, uint64_t seed, int n_gpus, float* out_rgb, rtx_stats* stats) {
    return rtx_render_ex(s, cam, seed, n_gpus, 0u, out_rgb, stats);
}

int rtx_render_ex(rtx_scene* s, const rtx_camera* cam, uint64_t seed, int n_gpus, uint32_t flags, float* out_rgb,
                  rtx_stats* stats) {
    g_last_error.clear();
    if (!s || !out_rgb) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_camera(cam)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    if (n_gpus <= 0) n_gpus = 1;
    if (n_gpus > ndev) return fail(RTX_ERR_INVALID_ARG, "n_gpus=%d but %d devices visible", n_gpus, ndev);
    std::lock_guard<std::mutex> lk(s->mu);
    std::lock_guard<std::mutex> bl(g_render_mu);  // the cached band / gather / image buffers
    return render_bands_locked(s, cam, seed, n_gpus, flags, out_rgb, nullptr, nullptr, stats);
}

}  // extern "C"
