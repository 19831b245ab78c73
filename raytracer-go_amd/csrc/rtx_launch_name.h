// rtx_launch_name.h — which compiled instantiation a launch runs (host code only).
// With RTX_DEBUG_LAUNCH=1 every launch of a templated kernel prints "rtx launch: <name>" to stderr beside its
// launch-shape line; tests/test_kernel_census.py holds the names it sees to tests/render_kernels.txt, the list of
// every instantiation librtx.so contains.
//
// <name> is the mangled name of the kernel.  hipcc emits, for every __global__ function, a host-side handle — an
// object in librtx.so's dynamic symbol table under the kernel's own mangled name — and that handle's address is what
// host code gets when it names the kernel (the pointer hipLaunchKernelGGL and hipOccupancy* are given).  dladdr
// turns the pointer back into the symbol: the same string `nm -D librtx.so` lists, so the launch lines and the
// list compare like with like, with no table of names to keep in step with the template arguments.
#pragma once
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>

namespace rtxd {

// The symbol whose address is exactly `kern`, or "?" (a pointer that is no kernel handle of this library).
inline const char* kernel_symbol(const void* kern) {
    Dl_info info;
    if (kern && dladdr(kern, &info) && info.dli_sname && info.dli_saddr == kern) return info.dli_sname;
    return "?";
}

// One "rtx launch:" line; the caller checks Params::debug_launch.
inline void print_launch_name(const void* kern) { fprintf(stderr, "rtx launch: %s\n", kernel_symbol(kern)); }

// The block launchers (launch_trace, launch_direct, launch_direct_paths, launch_emitter_weights, launch_guides,
// launch_shade, launch_camera_rays, launch_denoise): their argument structs go to the device as they are and have no
// debug_launch field, so RTX_DEBUG_LAUNCH is read here, per launch, as env_knob reads it (clamped to 0 / 1).
inline bool debug_launch_env() {
    const char* e = std::getenv("RTX_DEBUG_LAUNCH");
    return e && std::strtol(e, nullptr, 10) >= 1;
}

// One "rtx launch:" line for the kernel a block launcher is about to launch; tests/test_block_census.py holds the
// names to tests/block_kernels.txt.
template <class K>
inline void name_launch(K* kern) {
    if (debug_launch_env()) print_launch_name((const void*)kern);
}

}  // namespace rtxd
