// rtx_devmem.h — the three owner types of the host code's device resources.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rtxd {

// A grow-only device buffer on the current device.  The destructor does nothing to the device: buffers live in
// objects of static storage (the per-device maps), and at process exit the runtime may already be gone; and a
// DeviceCopy is copied by value into its scene.  release() is explicit, with the buffer's device current.  The type
// knows nothing about streams or events: where the buffer may still be in use, the caller waits before reserve().
struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;

    // At least `want` bytes: freed and allocated anew only when too small (what it held is lost); on failure the
    // buffer is left empty.
    hipError_t reserve(size_t want) {
        if (want <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&ptr, want);
        if (e != hipSuccess) ptr = nullptr;
        else bytes = want;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
};

// The current device for a scope: reads it, optionally sets another, and sets the one it read again on the way out,
// error paths included.
class DeviceGuard {
public:
    DeviceGuard() { err_ = hipGetDevice(&prev_); }
    explicit DeviceGuard(int device) : DeviceGuard() {
        if (err_ == hipSuccess) err_ = hipSetDevice(device);
    }
    ~DeviceGuard() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    hipError_t error() const { return err_; }  // of the constructor's get / set
    int previous() const { return prev_; }     // the device that was current (-1: unknown)

private:
    int prev_ = -1;
    hipError_t err_ = hipSuccess;
};

// The device buffers of one host-pointer entry (rtx_trace, rtx_shade, ..): each of the caller's arrays with its
// device twin for the length of the call.  Unlike DeviceBuffer this one frees in its destructor, and may: it lives in
// the entry's own scope alone, never in static storage and never copied, so it dies on every path out of a call
// that has just used the runtime, with the device the buffers were made on still current.
enum class Stage { in, out, scratch };  // copied to the device before the call, back after it, neither
struct StageItem {
    const void* host;  // nullptr (but for scratch): an array the caller left out, which gets no buffer
    size_t bytes;
    Stage dir;
};
template <size_t N>
class Staging {
public:
    explicit Staging(const StageItem (&items)[N]) {
        for (size_t i = 0; i < N; ++i) item_[i] = items[i];
    }
    ~Staging() {
        for (DeviceBuffer& b : buf_) b.release();
    }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    template <class T>
    T* dev(size_t i) const { return buf_[i].template as<T>(); }

    // Reserves the buffers, copies the inputs in, runs call() (the _device entry on the null stream; *rc: its RTX_*
    // code) and after an RTX_OK (0) copies the outputs out (blocking copies: after the kernels).  Returns the first
    // failure of a reserve or a copy; call()'s code, where it is not 0, is the one to report.
    template <class F>
    hipError_t run(F&& call, int* rc) {
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < N && e == hipSuccess; ++i)
            if (item_[i].host || item_[i].dir == Stage::scratch) e = buf_[i].reserve(item_[i].bytes);
        for (size_t i = 0; i < N && e == hipSuccess; ++i)
            if (item_[i].host && item_[i].dir == Stage::in)
                e = hipMemcpy(buf_[i].ptr, item_[i].host, item_[i].bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess || (*rc = call()) != 0) return e;
        for (size_t i = 0; i < N && e == hipSuccess; ++i)
            if (item_[i].host && item_[i].dir == Stage::out)
                e = hipMemcpy(const_cast<void*>(item_[i].host), buf_[i].ptr, item_[i].bytes, hipMemcpyDeviceToHost);
        return e;
    }

private:
    StageItem item_[N];
    DeviceBuffer buf_[N];
};

}  // namespace rtxd
