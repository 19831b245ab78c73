// rtx_kernel.h — launch interface between the C-ABI layer and the megakernel.
#pragma once
#include <hip/hip_runtime.h>

namespace rtxd {
struct Params;
// One pass of an accumulator (rtx_accum): the samples [first, first + count) of every pixel, their
// colours added by accumulate_samples to the tile-major moments s and q (3 floats per scratch slot, ragged tiles
// padded: tiles x 64 x 3 floats each) instead of being averaged into p.out.
// tile_list != nullptr: an ADAPTIVE pass: only the *n_open tiles listed there (device memory, written by
// launch_select earlier on the stream) are rendered and folded; the other tiles' s and q are not touched.
struct SampleRange {
    uint32_t first, count;
    float* s;
    float* q;
    const uint32_t* tile_list = nullptr;
    const uint32_t* n_open = nullptr;
};
// Enqueue a render of p's region on `stream` (render_items + reduce_samples per sample
// chunk; the caller provides p.scratch / p.kn / p.sub).  flags: RTX_FLAG_COUNTERS selects
// the instantiation that accumulates the work counters into p.counters; RTX_FLAG_NO_LDS
// reads the scene from global memory (A/B, identical output).
// far != nullptr: a tiered walk: p is the near pass (p.tier = 1), *far the far
// pass over the same region (tier 2), per chunk: near pass, far pass, redo pass (the far layout
// over the samples whose records did not fit the near pass's queue, if any), then the reduction.
// pass == nullptr: the samples [0, p.cam.samples_per_pixel) averaged into p.out.  Else that pass of an accumulator:
// the same launches in the same order over its samples, each chunk ending in accumulate_samples; p.out is not written.
hipError_t launch_render(const Params& p, uint32_t flags, hipStream_t stream, const Params* far = nullptr,
                         const SampleRange* pass = nullptr);
// rtx_accum_resolve_device (resolve_accum): from the tile-major s and q after n samples (the tiles of a width x rows
// shard, tile_w_log2 as the passes had it) the row-major mean rgb, the variance of the mean var (or nullptr) and, added
// to *noisy (or nullptr; the caller zeroes it), the pixels whose summed variance exceeds (rel_tol * max(sum of the
// mean's channels, 0.01))^2.
struct ResolveArgs {
    const float* s;
    const float* q;
    float* rgb;
    float* var;
    unsigned long long* noisy;
    uint32_t width, rows, tile_w_log2, n;
    float rel_tol;
    // an accumulator with adaptive passes: one word per tile, 0 = open (its pixels have n samples), else the n its
    // pixels stopped at; nullptr: every pixel has n
    const uint32_t* tile_n = nullptr;
};
hipError_t launch_resolve(const ResolveArgs& a, hipStream_t stream);
// The selection of an adaptive pass (select_tiles): with close != 0, every open tile of the width x rows shard none of
// whose live pixels is noisy by resolve's test at (n, rel_tol) gets its word in tile_n set to n; the tiles still open
// are listed in tile_list (any order), *n_open receives their number and *open_pixels their live pixels (the caller
// zeroes both).
struct SelectArgs {
    const float* s;
    const float* q;
    uint32_t* tile_n;
    uint32_t* tile_list;
    uint32_t* n_open;
    unsigned long long* open_pixels;
    uint32_t width, rows, tile_w_log2, n;
    float rel_tol;
    uint32_t close;
};
hipError_t launch_select(const SelectArgs& a, hipStream_t stream);
// rtx_accum_sample_counts_device: the samples every pixel received, row-major, from the tiles' words (or nullptr) and n.
hipError_t launch_counts(const uint32_t* tile_n, uint32_t* out, uint32_t width, uint32_t rows, uint32_t tile_w_log2,
                         uint32_t n, hipStream_t stream);
// Where a launch reads the scene (RTX_SCENE_IN_LDS / LDS_CACHE / IN_HBM, rtx.h).
uint32_t scene_placement(const Params& p, uint32_t flags);
// Where a tiered walk reads both layouts: their common placement, or RTX_SCENE_IN_HBM when they differ.
uint32_t tier_placement(const Params& near, const Params& far, uint32_t flags);
}  // namespace rtxd
