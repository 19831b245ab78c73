// rtx_internal.h — what the units of the C-ABI (include/rtx.h) share; library-internal.
//
//   rtx_scene.hip      host only: the caller's tree validated and flattened, the walk planner's glue, the storage
//                      order of a device layout (pack_layout), and the entry points that need no device
//   rtx_resources.hip  per-device resources kept between calls: sample scratch, pinned stages, the sticky error
//                      word, render buffers / streams / events, RCCL; rtx_release_device_memory, rtx_device_check
//   rtx_render.hip     the scene's device copy and layouts, enqueue_on / collect_on, the region render, PPM
//   rtx_bands.hip      rtx_render(_ex): the bands and their assembly
//   rtx_accum.hip      progressive passes and their previews; rtx_trace_capi.hip: ray queries; rtx_shade_capi.hip:
//                      camera rays and material scatter for a batch; rtx_guides_capi.hip: guide images and the
//                      preview filter; rtx_direct_capi.hip: light samples and shadow rays for a batch;
//                      rtx_capi.hip: scene create / destroy
//   rtx_batch.hip      what the batch entry points (trace, shade, guides, direct) share: the scene's copy on the
//                      current device, a feature's counters and events (Probe), the argument checks, the shard and
//                      walk parameters of a launch
//
// A unit that defines RTX_HOST_ONLY before including this header sees the first half only, which names no HIP type:
// it compiles with the plain host compiler and links without the runtime (tests/test_pack_layout.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rtx.h"
#include "rtx_layout.h"
#include "rtx_topology.h"

namespace rtxh {
struct DeviceCopy;  // below: a scene's tables on one device
}

struct rtx_scene {
    // The caller's tree as threaded entries in the reference's visit order (bvh.go:220-249).
    std::vector<rtx_entry> base;
    // The walk as threaded entries: layouts[0] for a scene that keeps the caller's topology; a
    // rebuilt scene (topo) has one per camera octant.  Each is planned on first use, for the
    // camera of that render: the tree's entries less the box tests the collapsed walk leaves
    // out (rtx_collapse.h; skips[k]: per node entry of the uncollapsed walk, 1 = left out).
    // Slots [8, 16) hold the near walks of a tiered scene (near_topo).
    std::vector<rtx_entry> layouts[16];
    std::vector<uint8_t> skips[16];
    std::vector<double> reads[16];  // estimated reads per entry of layouts[k] (the hot set of a big scene)
    bool planned[16] = {};
    bool rebuilt = false;
    bool tiered = false;     // near_topo built: renders whose camera lies in its near region walk in two tiers
    rtxd::Topology near_topo;
    std::vector<uint32_t> sphere_rank;  // each sphere's place in the reference walk (base): the tie rule
    bool every_box = false;  // RTX_SCENE_EVERY_BOX: no box test left out
    rtxd::Topology topo;
    std::vector<float> quadtab;  // 16 floats per quad (rtx_layout.h)
    std::vector<rtx_material> materials;
    std::vector<rtx_texture> textures;
    std::vector<uint32_t> texels;
    // by pointer: the host-only unit sees DeviceCopy incomplete (scenes are made and deleted in rtx_capi.hip alone)
    std::map<int, std::unique_ptr<rtxh::DeviceCopy>> copies;
    bool has_image = false;  // some texture is an ImageTexture: hits need UV
    bool has_noise = false;  // some texture is a Perlin NoiseTexture
    // Direct light sampling: the emitter table, built from `base` by the first call that asks for it
    // (build_lights, mu held) and never by scene creation.  lighttab: 16 floats per emitter, the device records.
    bool lights_built = false;
    std::vector<rtx_light> lights;
    std::vector<float> lighttab;
    std::vector<rtx_prim_light> primlights;  // rtx_prim_lights' lookup: sphere_rank.size() spheres, then the quads
    std::mutex mu;
};

namespace rtxh {

// ---- rtx_scene.hip (host only) -------------------------------------------------------------------------------
extern thread_local std::string g_last_error;
int fail(int code, const char* fmt, ...);
// Integer knob from the environment (read per call), clamped to [lo, hi].
uint32_t env_knob(const char* name, long dflt, long lo, long hi);

int check_acyclic(const rtx_scene_desc* d);
int emit(const rtx_scene_desc* d, int32_t root, std::vector<rtx_entry>& out);
int validate_tables(const rtx_scene_desc* d);
// The items of a World handed to the GPU BVH build: each a sphere or a quad of d's tables.
int check_world_items(const rtx_scene_desc* d, const int32_t* items, uint32_t n_items);
void quad_table(const rtx_scene_desc* d, std::vector<float>& tab);
void rank_spheres(rtx_scene* s);
void adopt_topology(rtx_scene* s, uint32_t flags, const rtx_scene_desc* d);
bool camera_in_near(const rtx_scene* s, const rtx_camera* cam);
uint32_t layout_slot(const rtx_scene* s, const rtx_camera* cam, bool near = false);
int scene_layout(rtx_scene* s, const rtx_camera* cam, const std::vector<rtx_entry>** out, bool near = false);
uint64_t walk_layout(const rtx_scene* s, const rtx_camera* cam, bool tiered);
int check_camera(const rtx_camera* cam);
int check_region(const rtx_camera* cam, const rtx_region* r);
uint32_t region_rows(const rtx_region* r);
uint32_t band_stripe(int n);
// The emitter table of a scene's entries in the reference walk's order (`base`), its quad table and its materials
// (rtx.h, "direct light sampling"): `lights` in table order and, when tab != nullptr, 16 floats per emitter for the
// device: (centre | Q, radius | 0), (u, area), (v, kind: RTX_PRIM_*), (the quad's normal, material).  prims != nullptr:
// also the per-primitive lookup of rtx_prim_lights, n_spheres entries for the caller's spheres, then one per quad.
int build_lights(const std::vector<rtx_entry>& base, const std::vector<float>& quadtab,
                 const std::vector<rtx_material>& materials, std::vector<rtx_light>& lights, std::vector<float>* tab,
                 std::vector<rtx_prim_light>* prims = nullptr, uint32_t n_spheres = 0);
// The scene's own table, built on first use (s->mu held).
int scene_lights(rtx_scene* s);

// A walk in device form (rtx_layout.h): what upload_layout copies to the device and what a render needs to know
// of it.
struct PackedLayout {
    std::vector<float> soa;  // all 'a' halves, all 'b' halves, each with the sentinel; then the quad table
    uint32_t hot = 0;        // entries stored first and cached in LDS by v3 (scenes too big for the LDS copy)
    uint32_t start = 0;      // walk position of the first entry of the walk (the root)
    uint32_t prim_end = 0;   // scenes in the LDS copy: primitives stored first, below this position
    uint32_t n_entries = 0;  // device entries before the sentinel
};
// reads: the plan's estimated reads per entry (the hot set of a big scene), or nullptr: the top levels.
// hot_cap: the most entries a big scene stores first.
PackedLayout pack_layout(const std::vector<rtx_entry>& E, const std::vector<double>* reads,
                         const std::vector<float>& quadtab, const std::vector<uint32_t>& sphere_rank,
                         uint32_t hot_cap);

}  // namespace rtxh

#ifndef RTX_HOST_ONLY
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is loaded on first use (rccl_api)

#include "rtx_device.h"
#include "rtx_devmem.h"
#include "rtx_kernel.h"
#include "rtx_walk.h"

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                        \
    } while (0)

namespace rtxh {
using rtxd::DeviceBuffer;
using rtxd::DeviceGuard;

// One threaded layout of the walk on a device (rtx_layout.h): a scene keeping the caller's
// topology has one; a rebuilt one (rtx_topology.h) one per camera octant, uploaded on first use.
struct DeviceLayout {
    DeviceBuffer entries;
    uint32_t hot = 0, start = 0, prim_end = 0, n_entries = 0;  // PackedLayout's
};

// A feature's counters and events on a scene's copy, made on first use: its own, so that a counting or timed call
// changes nobody else's stats.  Every method wants the copy's device current and returns an RTX_* code.
struct Probe {
    DeviceBuffer counters;  // `slots` x u64
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    int ensure(uint32_t slots);
    // Before the launches on `st`: count zeroes the counters, timed records ev0.
    int begin(bool count, bool timed, hipStream_t st);
    // After them (a timed call): records ev1, waits for it; *ms: from ev0 to ev1.
    int end(hipStream_t st, float* ms);
    int read(unsigned long long* h, uint32_t n);  // the first n counters, after end()
    void release();
    unsigned long long* slots() const { return counters.as<unsigned long long>(); }
};

struct DeviceCopy {
    int device = -1;
    DeviceLayout lay[16];  // [0, 8): the walk of each camera octant; [8, 16): the near walks of a tiered scene
    DeviceBuffer materials, textures, texels;
    DeviceBuffer counters;  // rtxd::COUNTER_SLOTS x u64
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t n_textures = 0;  // device textures: those materials read (checkered, image, noise)
    uint32_t placement = 0;   // the last enqueued render's rtxd::scene_placement
    // Ray queries (rtx_trace_device): layouts, counters and events of their own, so that a trace
    // never plans, replaces or disturbs anything a render uses.  trace_lay[0, 8): the uncollapsed walk of a rebuilt
    // scene's tree for each hinted octant; a scene that keeps the caller's tree has trace_lay[0] alone.
    DeviceLayout trace_lay[8];
    DeviceBuffer rank_sphere;  // rank word of a sphere entry -> the caller's sphere index (first trace)
    DeviceBuffer lights;       // direct light sampling: the emitter records (first call)
    DeviceBuffer prim_lights;  // multiple importance sampling: the per-primitive lookup, with `lights`
    // ray queries (and the guide images' timing), path building blocks, direct light sampling
    Probe trace, shade, direct;

    unsigned long long* slot(uint32_t k) const { return counters.as<unsigned long long>() + k; }
    // a counter slot's low word, for the three the kernels claim from
    uint32_t* word(uint32_t k) const { return reinterpret_cast<uint32_t*>(slot(k)); }
};

// ---- rtx_resources.hip ---------------------------------------------------------------------------------------
// Sample-colour scratch, one per device, shared by all scenes (grown on demand).  `last`
// marks its latest use, so a render on another stream waits for the previous one before
// reusing it — which also serialises every render on a device on the GPU (the per-scene
// counters and unit queue rely on that).  `scenes` counts the scene copies on the
// device: the last rtx_scene_destroy there frees the scratch (rtx_release_device_memory
// frees it at any time).
struct Scratch {
    DeviceBuffer samples;
    DeviceBuffer defer;  // the tiered walk's queue of deferred paths (64 B per record)
    DeviceBuffer drain;  // Params::drain_count: its last two words are the far and redo passes' unit-queue heads
    DeviceBuffer redo;   // the tiered walk's redo bits: one per sample of a chunk
    size_t redo_zero = 0;  // bytes at the start of `redo` known to be zero (reduce_samples keeps them so)
    hipEvent_t last = nullptr;
    int scenes = 0;
};
extern std::mutex g_scratch_mu;
extern std::map<int, Scratch> g_scratch;
void release_scratch_locked(int device);  // g_scratch_mu held
// `st` waits for every render enqueued on the device so far (Scratch::last).
int wait_for_renders(int device, hipStream_t st);

// The PPM encoder's per-device scratch (line lengths and offsets), reused across calls;
// g_ppm_mu is held for a whole (blocking) encode.
extern std::mutex g_ppm_mu;
extern std::map<int, DeviceBuffer> g_ppm;

hipError_t copy_to_host(void* dst, const void* src, size_t bytes, hipStream_t st);
// Zero device memory and return when it IS zero.  The host hipMemset only enqueues the fill on the null stream
// (measured: it returns in 5 us with the fill of 1 GiB, or the null stream's earlier work, still running), and a
// non-blocking stream does not wait for the null stream: work enqueued on one right after would meet the old
// contents, or have its own results wiped later.
hipError_t zero_now(void* ptr, size_t bytes);

uint32_t* kerr_word(int device);
int kerr_take(int device);

struct RcclApi {
    bool tried = false, ok = false;
    std::string err;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
extern std::mutex g_rccl_mu;
extern std::map<int, std::vector<ncclComm_t>> g_comms;  // devices 0..n-1 -> communicators (ncclCommInitAll)
const RcclApi* rccl_api();  // g_rccl_mu held

// rtx_render's per-device buffers (bands, the gathered bands, the assembled image), stream and
// gather events, kept between calls and freed by rtx_release_device_memory; g_render_mu is held
// for a whole rtx_render.  Keyed by (device, slot): slot d >= 0 is band d, -1 the gather, -2 the
// image, -3 / -4 the image and text of rtx_render_ppm and rtx_accum_ppm, -5 rtx_accum_resolve's variance,
// -6 rtx_accum_sample_counts' map.
// Each wants the current device = device and g_render_mu held, and returns nullptr on failure.
extern std::mutex g_render_mu;
void* render_buffer(int device, int slot, size_t bytes);
hipStream_t render_stream(int device);
hipEvent_t render_event(int device, int k);

// ---- rtx_render.hip ------------------------------------------------------------------------------------------
// Lock order everywhere: s->mu, then g_render_mu (rtx_render_ex, rtx_render_ppm), then g_scratch_mu (enqueue_on).
int ensure_device(rtx_scene* s, int device, DeviceCopy** out);
int upload_layout(const rtx_scene* s, const std::vector<rtx_entry>& E, const std::vector<double>* reads,
                  DeviceLayout& lay);
void drop_copy(DeviceCopy& c);
rtxd::Params make_params(const rtx_scene* s, const DeviceCopy* c, uint32_t oct, const rtx_camera* cam, uint64_t seed,
                         const rtx_region* r, float* d_out);
int enqueue_on(rtx_scene* s, DeviceCopy* c, const rtx_camera* cam, uint64_t seed, const rtx_region* r, float* d_out,
               hipStream_t stream, uint32_t flags, bool timed, uint32_t* chunks, bool* tiered,
               const rtxd::SampleRange* pass = nullptr, uint64_t pass_slots = 0);
int collect_on(DeviceCopy* c, bool count, uint64_t samples, uint32_t chunks, rtx_stats* st);
void add_stats(rtx_stats* acc, const rtx_stats& s);
int render_region_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, float* d_out,
                         void* hip_stream, uint32_t flags, rtx_stats* stats);
// The end of every PPM entry point.  rc: what came before (not RTX_OK: returned as it is).  `rgb` (W x H on st's
// device) encoded into the device buffer `text` (of rtx_ppm_max_bytes) and copied into the caller's out_text when it
// fits; st is synchronised either way.
int ppm_to_host(int rc, const float* rgb, uint32_t W, uint32_t H, char* text, hipStream_t st, char* out_text,
                uint64_t capacity, uint64_t* out_len);

// ---- rtx_batch.hip -------------------------------------------------------------------------------------------
int hip_fail(hipError_t e, const char* what);  // fail(RTX_ERR_OOM or RTX_ERR_HIP, "<what>: <HIP's text>")
// The scene's copy on the current device (s->mu held); *device: that device.
int current_copy(rtx_scene* s, DeviceCopy** out, int* device = nullptr);
// The checks of a batch entry that need no device: the scene, the flags against `allowed`, then, unless n == 0
// (*empty: nothing to do), the record arrays `args`: not NULL, aligned to 16 B, n * record_bytes within size_t.
struct BatchArg {
    const void* ptr;
    const char* name;
};
int check_batch(const rtx_scene* s, uint32_t flags, uint32_t allowed, const char* feature, uint64_t n, size_t record_bytes,
                std::initializer_list<BatchArg> args, bool* empty);
// Samples [first, first + count) within the RNG's 32-bit sample word.
int check_sample_range(uint32_t first, uint32_t count);
// The launch parameters of a region's shard over samples [first, first + count), and of a trace layout.
rtxd::Shard shard_of(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first, uint32_t count);
rtxd::WalkScene walk_scene(const rtx_scene* s, const DeviceLayout* lay);
// fn(offset, count) for [0, n) cut into launches of at most per_launch; stops at the first code that is not RTX_OK.
template <class F>
int for_launches(uint64_t n, uint64_t per_launch, F&& fn) {
    for (uint64_t off = 0; off < n; off += per_launch)
        if (int rc = fn(off, (uint32_t)std::min<uint64_t>(per_launch, n - off))) return rc;
    return RTX_OK;
}

// A host-pointer entry through its Staging (rtx_devmem.h): call()'s code wins, else a failed reserve or copy is
// RTX_ERR_OOM / RTX_ERR_HIP with `what` ("<entry>'s buffers").
template <class S, class F>
int run_staged(S& st, const char* what, F&& call) {
    int rc = RTX_OK;
    const hipError_t e = st.run(call, &rc);
    if (rc != RTX_OK) return rc;
    return e == hipSuccess ? RTX_OK : hip_fail(e, what);
}

// ---- rtx_trace_capi.hip --------------------------------------------------------------------------------------
// What a trace on copy c needs beside the scene (s->mu held, current device = c's), made on first use (c->trace's
// counters and events among it); *out: the trace layout for the hinted octant.
int ensure_trace(rtx_scene* s, DeviceCopy* c, uint32_t oct, const DeviceLayout** out);

// ---- rtx_guides_capi.hip -------------------------------------------------------------------------------------
// rtx_guides_device after its checks, with s->mu held (rtx_accum_preview*).
int guides_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                  uint32_t count, rtx_guide* d_guides, hipStream_t stream, rtx_guide_stats* stats);

// ---- rtx_direct_capi.hip -------------------------------------------------------------------------------------
// One fused direct-light pass into an accumulator's moments (rtx_accum_add_direct after its checks), s->mu held.
// mis: the estimator of rtx_accum_add_mis.
int direct_pass_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t tile_w_log2,
                       uint32_t first, uint32_t count, float* acc_s, float* acc_q, hipStream_t stream, rtx_stats* stats,
                       bool mis = false);

// ---- rtx_bands.hip -------------------------------------------------------------------------------------------
int render_bands_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, int n_gpus, uint32_t flags, float* out_rgb,
                        float** dev_img, hipStream_t* dev_stream, rtx_stats* stats);

}  // namespace rtxh
#endif  // RTX_HOST_ONLY
