// rtx_devmem.h — the two owner types of the host code's device resources.
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

}  // namespace rtxd
