// rtx_render.hip — a scene on a device and one render of it: the scene's device copy and walk layouts, uploaded on
// first use; enqueue_on / collect_on, which every render, band and accumulator pass goes through; the region
// render; and the PPM entry points.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "rtx_internal.h"
#include "rtx_ppm.h"

namespace rtxh {

namespace {

int upload_copy(rtx_scene* s, DeviceCopy& c) {
    // device materials: a Lambertian or DiffuseLight with a SolidColor texture carries the
    // colour itself (rtxd::RTX_DEV_TEX_INLINE), so shading reads no texture record; the other
    // textures they read are numbered anew in the device texture table, which holds only those
    // (small enough for the LDS copy: randSpheres' 488 SolidColors leave one checkered texture)
    std::vector<rtx_texture> dt;
    {
        std::vector<rtx_material> dm(s->materials);
        std::vector<int64_t> renum(s->textures.size(), -1);
        for (rtx_material& m : dm) {
            if ((m.type == RTX_MAT_LAMBERTIAN || m.type == RTX_MAT_DIFFUSE_LIGHT) &&
                s->textures[m.texture].type == RTX_TEX_SOLID) {
                std::memcpy(m.albedo, s->textures[m.texture].even, sizeof(m.albedo));
                m.texture = rtxd::RTX_DEV_TEX_INLINE;
            } else if (m.type == RTX_MAT_LAMBERTIAN || m.type == RTX_MAT_DIFFUSE_LIGHT) {
                if (renum[m.texture] < 0) {
                    renum[m.texture] = (int64_t)dt.size();
                    dt.push_back(s->textures[m.texture]);
                }
                m.texture = (uint32_t)renum[m.texture];
            }
            if (m.type == RTX_MAT_DIELECTRIC) {  // (albedo unused: attenuation is (1,1,1))
                // per-material float32 quotients of materials.go:98, 116-117, computed once here
                // (IEEE division: the same bits the kernel's correctly rounded divide gave)
                const float inv = 1.0f / m.ior;
                const float rf = (1.0f - inv) / (1.0f + inv), rb = (1.0f - m.ior) / (1.0f + m.ior);
                m.albedo[0] = inv;      // eta of a front-face hit
                m.albedo[1] = rf * rf;  // r0 for eta = 1/ior
                m.albedo[2] = rb * rb;  // r0 for eta = ior
            }
        }
        HIP_TRY(c.materials.reserve(std::max<size_t>(1, dm.size()) * sizeof(rtx_material)));
        if (!dm.empty()) HIP_TRY(hipMemcpy(c.materials.ptr, dm.data(), dm.size() * sizeof(rtx_material), hipMemcpyHostToDevice));
    }
    {  // device textures: a Checkered carries invScale = float32(1 / scale) (materials.go:128) in `pad`,
       // the IEEE quotient computed once here instead of per lookup
        for (rtx_texture& t : dt)
            if (t.type == RTX_TEX_CHECKERED) t.pad = 1.0f / t.scale;
        HIP_TRY(c.textures.reserve(std::max<size_t>(1, dt.size()) * sizeof(rtx_texture)));
        if (!dt.empty()) HIP_TRY(hipMemcpy(c.textures.ptr, dt.data(), dt.size() * sizeof(rtx_texture), hipMemcpyHostToDevice));
        c.n_textures = (uint32_t)dt.size();
    }
    HIP_TRY(c.texels.reserve(std::max<size_t>(1, s->texels.size()) * sizeof(uint32_t)));
    if (!s->texels.empty())
        HIP_TRY(hipMemcpy(c.texels.ptr, s->texels.data(), s->texels.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c.counters.reserve(rtxd::COUNTER_SLOTS * sizeof(unsigned long long)));
    HIP_TRY(hipEventCreate(&c.ev0));
    HIP_TRY(hipEventCreate(&c.ev1));
    return RTX_OK;
}

void free_copy(DeviceCopy& c) {
    DeviceGuard on(c.device);
    if (on.error() != hipSuccess) return;
    (void)hipDeviceSynchronize();  // no render of this copy still running
    for (DeviceLayout& l : c.lay) l.entries.release();
    for (DeviceLayout& l : c.trace_lay) l.entries.release();
    for (DeviceBuffer* b : {&c.rank_sphere, &c.lights, &c.prim_lights, &c.materials, &c.textures, &c.texels, &c.counters}) b->release();
    for (Probe* p : {&c.trace, &c.shade, &c.direct}) p->release();
    for (hipEvent_t ev : {c.ev0, c.ev1})
        if (ev) (void)hipEventDestroy(ev);
}

}  // namespace

// Free a scene's copy; the last copy on a device also frees the device's scratch.
void drop_copy(DeviceCopy& c) {
    free_copy(c);
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    Scratch& sc = g_scratch[c.device];
    if (sc.scenes > 0 && --sc.scenes == 0) release_scratch_locked(c.device);
}

// The scene's copy on `device` (materials, textures, texels, counters), uploaded on first
// use; a failed upload frees what it had allocated.  Every copy is counted in the device's
// Scratch::scenes.  Walk layouts are uploaded separately (ensure_layout).  The current device is left as it was.
int ensure_device(rtx_scene* s, int device, DeviceCopy** out) {
    auto it = s->copies.find(device);
    if (it != s->copies.end()) {
        *out = it->second.get();
        return RTX_OK;
    }
    std::unique_ptr<DeviceCopy> c(new (std::nothrow) DeviceCopy());
    if (!c) return fail(RTX_ERR_OOM, "host memory for a scene copy");
    c->device = device;
    DeviceGuard on(device);
    HIP_TRY(on.error());
    if (int rc = upload_copy(s, *c)) {
        free_copy(*c);
        return rc;
    }
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        ++g_scratch[device].scenes;
    }
    *out = (s->copies[device] = std::move(c)).get();
    return RTX_OK;
}

// The walk E in device form into `lay` (current device = the copy's; s->mu held).  reads: the plan's estimated reads
// per entry (the hot set of a big scene), or nullptr: the top levels.
int upload_layout(const rtx_scene* s, const std::vector<rtx_entry>& E, const std::vector<double>* reads,
                  DeviceLayout& lay) {
    const uint32_t cap = env_knob("RTX_HOT_ENTRIES", rtxd::HOT_ENTRIES_MAX, 0, rtxd::HOT_ENTRIES_MAX);
    if (!env_knob("RTX_HOT_BY_READS", 1, 0, 1)) reads = nullptr;
    const PackedLayout pk = pack_layout(E, reads, s->quadtab, s->sphere_rank, cap);
    HIP_TRY(lay.entries.reserve(pk.soa.size() * sizeof(float)));
    const hipError_t copied = hipMemcpy(lay.entries.ptr, pk.soa.data(), pk.soa.size() * sizeof(float), hipMemcpyHostToDevice);
    if (copied != hipSuccess) lay.entries.release();  // (no half-made layout is taken for an uploaded one)
    HIP_TRY(copied);
    lay.hot = pk.hot;
    lay.start = pk.start;
    lay.prim_end = pk.prim_end;
    lay.n_entries = pk.n_entries;
    return RTX_OK;
}

namespace {

int ensure_layout(rtx_scene* s, DeviceCopy* c, const rtx_camera* cam, bool near = false) {
    const uint32_t oct = layout_slot(s, cam, near);
    if (c->lay[oct].entries.ptr) return RTX_OK;
    const std::vector<rtx_entry>* E = nullptr;
    if (int rc = scene_layout(s, cam, &E, near)) return rc;
    return upload_layout(s, *E, &s->reads[oct], c->lay[oct]);
}

// Lanes of a wave that wait before it shades (v1-v3); RTX_SHADE_THRESH.  48 measured
// best for v3 at the headline config with primitive batching (44 the same, 40 +1.3 %,
// 56 +4.6 %) and for v1.
uint32_t shade_thresh() {
    static const uint32_t v = [] {
        const char* e = std::getenv("RTX_SHADE_THRESH");
        const long x = e ? std::strtol(e, nullptr, 10) : 48;
        return (uint32_t)(x < 1 ? 1 : (x > 64 ? 64 : x));
    }();
    return v;
}

// Per-wave time limit of the persistent kernel (RTX_WATCHDOG_S, default 300 s): a bug
// can never keep the GPU busy forever; the launch then fails with RTX_ERR_HIP.
uint64_t watchdog_ticks() {
    static const uint64_t v = [] {
        const char* e = std::getenv("RTX_WATCHDOG_S");
        double s = e ? std::strtod(e, nullptr) : 300.0;
        if (!(s > 0)) s = 300.0;
        return (uint64_t)(s * 1.0e8);  // s_memrealtime runs at 100 MHz
    }();
    return v;
}

}  // namespace

rtxd::Params make_params(const rtx_scene* s, const DeviceCopy* c, uint32_t oct, const rtx_camera* cam, uint64_t seed,
                         const rtx_region* r, float* d_out) {
    rtxd::Params p;
    std::memset(&p, 0, sizeof(p));
    const DeviceLayout& lay = c->lay[oct];
    p.entries = lay.entries.as<const float4>();
    p.n_entries = lay.n_entries;
    p.n_quads = (uint32_t)(s->quadtab.size() / 16);
    p.n_materials = (uint32_t)s->materials.size();
    p.materials = c->materials.as<rtx_material>();
    p.textures = c->textures.as<rtx_texture>();
    p.n_textures = c->n_textures;
    p.texels = c->texels.as<uint32_t>();
    p.cam = *cam;
    p.seed = seed;
    p.x0 = r->x0;
    p.y0 = r->y0;
    p.width = r->width;
    p.rows = region_rows(r);
    p.rank = r->rank;
    p.world = r->world;
    p.stripe_log2 = r->stripe > 1 ? (uint32_t)__builtin_ctz(r->stripe) : 0u;
    // RTX_TILE_W = 8 / 16 / 32 overrides the tile width (A/B)
    const uint32_t tw = env_knob("RTX_TILE_W", 0, 0, 32);
    p.tile_w_log2 = tw >= 32 ? 5u : (tw >= 16 ? 4u : (tw >= 8 ? 3u : rtxd::tile_w_log2_for(r->world, r->stripe)));
    p.tile_w_log2 = std::max(p.tile_w_log2, rtxd::tile_w_log2_min(p.stripe_log2));  // a tile within one stripe
    p.out = d_out;
    p.counters = c->slot(0);
    p.tile_counter = c->word(rtxd::CNT_UNIT_HEAD);
    p.error_flag = nullptr;  // the device's sticky error word (KernErr), set by enqueue_on
    p.watchdog_ticks = watchdog_ticks();
    p.shade_thresh = shade_thresh();
    p.has_uv = s->has_image ? 1u : 0u;
    p.has_noise = s->has_noise ? 1u : 0u;
    p.n_hot = lay.hot;
    p.start = lay.start;
    p.prim_end = lay.prim_end;
    return p;
}

// Enqueue one region on the current device, bracketed by HIP events on `stream`.
// *chunks receives the number of sample chunks (render kernel launches).
// *tiered: whether the render walks in two tiers.
// pass: one pass of an accumulator (its samples into its S and Q, d_out unused; pass_slots: the scratch slots its
// buffers hold) instead of the camera's samples_per_pixel averaged into d_out.
int enqueue_on(rtx_scene* s, DeviceCopy* c, const rtx_camera* cam, uint64_t seed, const rtx_region* r, float* d_out,
               hipStream_t stream, uint32_t flags, bool timed, uint32_t* chunks, bool* tiered,
               const rtxd::SampleRange* pass, uint64_t pass_slots) {
    const uint32_t n_samples = pass ? pass->count : cam->samples_per_pixel;  // of every pixel, in this call
    const uint32_t oct = layout_slot(s, cam);  // the walk's layout (rtx_topology.h, rtx_collapse.h)
    if (int rc = ensure_layout(s, c, cam)) return rc;
    rtxd::Params p = make_params(s, c, oct, cam, seed, r, d_out);
    if (!(p.error_flag = kerr_word(c->device))) return fail(RTX_ERR_OOM, "the error word on device %d", c->device);
    if (pass) {  // an adaptive pass: its open tiles (a tiered render's passes copy p below)
        p.tile_list = pass->tile_list;
        p.n_open = pass->n_open;
    }
    // the tiered walk: a camera in the near region of a sphere scene (rtx_scene_near_region's rule)
    bool tier = camera_in_near(s, cam) && !p.has_noise;
    rtxd::Params pn;
    if (tier) {
        if (int rc = ensure_layout(s, c, cam, true)) return rc;
        pn = make_params(s, c, layout_slot(s, cam, true), cam, seed, r, d_out);
        // a scene with quads walks in tiers in single-row shards, with the timed or the counting kernel
        if (p.n_quads && (r->stripe > 1 || ((flags & RTX_FLAG_TIMING) && !(flags & RTX_FLAG_COUNTERS)))) tier = false;
    }
    *tiered = false;
    const uint32_t th = (flags >> 8) & 0x7Fu;  // RTX_FLAG_SHADE_THRESH(n) override
    if (th) p.shade_thresh = th > 64 ? 64 : th;
    *chunks = 0;
    std::unique_lock<std::mutex> scr_lock(g_scratch_mu);
    Scratch* scr = &g_scratch[c->device];
    if (!scr->last) HIP_TRY(hipEventCreateWithFlags(&scr->last, hipEventDisableTiming));
    // Every render on this device waits for the previous one (the shared scratch, and the
    // scene's counters / unit queue, are reused).
    HIP_TRY(hipStreamWaitEvent(stream, scr->last, 0));
    if (p.width > 0 && p.rows > 0) {
        // Sample scratch: up to RTX_SCRATCH_MB (default 16 GiB of the 288 GB HBM) of sample
        // colours, 12 B each; the samples run in chunks that fit.
        // tile-major: every tile of 64 pixels whole (render_items / reduce_samples), 12 B per pixel
        const uint64_t per_sample =
            (uint64_t)rtxd::tiles_x_of(p.width, p.tile_w_log2) * rtxd::tiles_y_of(p.rows, p.tile_w_log2) * 64 * 12;
        // an accumulator's S and Q were sized at create: the tiles must be the same (RTX_TILE_W changed since?)
        if (pass && per_sample / 12 != pass_slots)
            return fail(RTX_ERR_INVALID_ARG, "the accumulator holds %llu pixel slots, this pass has %llu (RTX_TILE_W changed?)",
                        (unsigned long long)pass_slots, (unsigned long long)(per_sample / 12));
        const uint64_t budget = (uint64_t)env_knob("RTX_SCRATCH_MB", 16384, 1, 1 << 20) << 20;
        uint64_t chunk = budget / per_sample;
        if (chunk > n_samples) chunk = n_samples;
        // the tiered walk names a chunk's samples by 32-bit ids ((k - k0) * tiles * 64 + slot: the redo
        // list, the redo bits' index): at most 2^32 scratch slots per chunk
        if (tier) chunk = std::min<uint64_t>(chunk, 0xFFFFFFFFull / (per_sample / 12));
        if (chunk < 1) return fail(RTX_ERR_OOM, "RTX_SCRATCH_MB too small for one sample of the region");
        const size_t need = (size_t)(chunk * per_sample);
        // (a buffer of the scratch may still be in use by the previous render: wait for it before it grows)
        if (scr->samples.bytes < need) HIP_TRY(hipEventSynchronize(scr->last));
        HIP_TRY(scr->samples.reserve(need));
        p.scratch = scr->samples.as<float>();
        p.kn = (uint32_t)chunk;
        *chunks = (uint32_t)((n_samples + chunk - 1) / chunk);
        p.sub = env_knob("RTX_ITEM_SUB", 0, 0, 4096);  // 0: chosen per chunk by launch_items
        // the redo pass skips a unit by one vote over its samples' bit words, one sample per lane
        if (tier && p.sub > 64) p.sub = 64;
        p.debug_partial = env_knob("RTX_DEBUG_PARTIAL_SITE", 0, 0, 3);  // (read by librtx_dbgclaim.so only)
        p.cam_pool = env_knob("RTX_CAM_POOL", 1, 0, 1);  // the near pass's camera-ray pool (A/B: 0 = off)
        p.refill_hits = env_knob("RTX_REFILL_HITS", 0, 0, 64);  // its miss phases (untiered: off by default)
        p.item_waves = env_knob("RTX_ITEM_WAVES", 8, 4, 8) >= 8 ? 8u : 4u;
        p.grid_pct = env_knob("RTX_ITEM_GRID", 100, 1, 100);
        p.debug_launch = env_knob("RTX_DEBUG_LAUNCH", 0, 0, 1);
        p.prim_batch = env_knob("RTX_PRIM_BATCH", 16, 1, 65);  // 65: primitive tests only when no node is left
        if (tier) {
            // The queue of deferred paths, per device: an eighth of the chunk's items (measured:
            // 3.2 % of randSpheres' paths leave the near region), at least 2^21 records (the near
            // pass's waves take slots in blocks of 64), at most RTX_DEFER_MB (default 4 GiB) of
            // records; RTX_DEFER_CAP overrides (tests).  A chunk that overflows it is rendered
            // again whole by the redo pass.
            // A sample whose record does not fit is flagged in a bitmap of the chunk's samples (one bit
            // per scratch slot) and rendered again from its camera ray by the redo pass.
            const uint64_t items = chunk * (per_sample / 12);
            uint64_t cap = std::max<uint64_t>(items / 8, 1u << 21);
            if (const char* e = std::getenv("RTX_DEFER_CAP")) cap = std::strtoull(e, nullptr, 10);
            cap = std::min<uint64_t>(cap, ((uint64_t)env_knob("RTX_DEFER_MB", 4096, 1, 1 << 20) << 20) / 64);
            cap = std::min<uint64_t>(cap, 0xFFFFFFFFull / 2);
            const size_t need = (size_t)std::max<uint64_t>(cap, 1) * 64;
            if (scr->defer.bytes < need) HIP_TRY(hipEventSynchronize(scr->last));
            HIP_TRY(scr->defer.reserve(need));
            // the bits (chunk x tiles x 64 slots, 8 per byte), then as many bytes of 4-byte sample ids: the
            // redo list holds up to 1/32 of the chunk's samples (C2 defers 0.9 % of its paths)
            const size_t bits = (size_t)(items / 8);
            if (scr->redo.bytes < 2 * bits) {
                HIP_TRY(hipEventSynchronize(scr->last));
                scr->redo_zero = 0;
            }
            HIP_TRY(scr->redo.reserve(2 * bits));
            // The bits [0, bits) must be zero at the first chunk's start; reduce_samples keeps them so after
            // every chunk.  Past them this render's redo list may leave ids, so only [0, bits) stays known zero.
            if (scr->redo_zero < bits) HIP_TRY(hipMemsetAsync(scr->redo.ptr, 0, bits, stream));
            scr->redo_zero = bits;
            rtxd::Params lay = pn;  // the near pass: every setting of p, the near walk's layout
            pn = p;
            pn.entries = lay.entries;
            pn.n_entries = lay.n_entries;
            pn.n_hot = lay.n_hot;
            pn.start = lay.start;
            pn.prim_end = lay.prim_end;
            pn.tier = 1;
            p.tier = 2;
            // the near pass's walk is cheaper: it shades in larger batches and tests primitives in
            // smaller ones (C2 at 100 spp: 56 / 12 lanes 23.15 ms, 48 / 16 23.49 ms; the far pass keeps
            // the defaults), unless RTX_SHADE_THRESH / RTX_SHADE_THRESH(n) / RTX_PRIM_BATCH say otherwise
            // With the camera-ray pool and its miss phases the near pass shades at 52 waiting lanes
            // and takes a miss phase when fewer than 36 of them hit (C2: 90.9 ms against 91.8 at 56 / 36, 92.2 at
            // 52 / 40; profiles/r05_refill_sweep.jsonl)
            const bool pooled = rtxd::tier_placement(pn, p, flags) == RTX_SCENE_IN_LDS && rtxd::pool_fits(pn);
            if (!th && !std::getenv("RTX_SHADE_THRESH")) pn.shade_thresh = pooled ? 52 : 56;
            if (!std::getenv("RTX_REFILL_HITS")) pn.refill_hits = 36;
            if (!std::getenv("RTX_PRIM_BATCH")) pn.prim_batch = 12;
            pn.defer = p.defer = scr->defer.as<float4>();
            pn.redo_bits = p.redo_bits = scr->redo.as<uint32_t>();
            pn.redo_ids = p.redo_ids = scr->redo.as<uint32_t>() + bits / 4;
            uint64_t rcap = std::min<uint64_t>(bits / 4, 0xFFFFFFFFull);
            if (const char* e = std::getenv("RTX_REDO_CAP")) rcap = std::min<uint64_t>(rcap, std::strtoull(e, nullptr, 10));
            pn.redo_cap = p.redo_cap = (uint32_t)rcap;  // (RTX_REDO_CAP: tests of the bits' path)
            pn.redo_count = p.redo_count = c->word(rtxd::CNT_REDO_COUNT);
            pn.defer_cap = p.defer_cap = (uint32_t)cap;
            pn.defer_count = p.defer_count = c->word(rtxd::CNT_DEFER_COUNT);  // records
            // the drain's per-workgroup words: 2 x the near grid (launch_tiered drains only when they fit)
            HIP_TRY(scr->drain.reserve(rtxd::DRAIN_WORDS * sizeof(uint32_t)));
            pn.drain_count = p.drain_count = scr->drain.as<uint32_t>();
            pn.drain = p.drain = env_knob("RTX_DRAIN", 1, 0, 1);
            std::memcpy(pn.near_min, s->near_topo.near_box, 3 * sizeof(float));
            std::memcpy(pn.near_max, s->near_topo.near_box + 3, 3 * sizeof(float));
            *tiered = true;
        }
    }
    c->placement = *tiered ? rtxd::tier_placement(pn, p, flags) : rtxd::scene_placement(p, flags);
    // every stats slot and the unit queue head start at 0 for every render (a tiered render's first chunk_start
    // launch zeroes them: one launch fewer); the sticky error word is not among them
    if (!*tiered) HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, c->counters.bytes, stream));
    if (timed) HIP_TRY(hipEventRecord(c->ev0, stream));
    if (const hipError_t e = *tiered ? rtxd::launch_render(pn, flags, stream, &p, pass)
                                     : rtxd::launch_render(p, flags, stream, nullptr, pass)) {
        scr->redo_zero = 0;  // a chunk may have stopped between setting redo bits and clearing them
        return hip_fail(e, "render launch failed");
    }
    if (timed) HIP_TRY(hipEventRecord(c->ev1, stream));
    HIP_TRY(hipEventRecord(scr->last, stream));
    return RTX_OK;
}

namespace {
// The counter slots that are plain sums, and the rtx_stats member each is reported in (the four slots of the shade
// split follow CNT_SHADE_SPLIT; kernel_ms, sample_chunks and scene_placement are no sums).
constexpr struct {
    uint32_t slot;
    uint64_t rtx_stats::*field;
} kSummed[] = {
    {rtxd::CNT_SAMPLES, &rtx_stats::samples},
    {rtxd::CNT_SEGMENTS, &rtx_stats::segments},
    {rtxd::CNT_NODE_VISITS, &rtx_stats::node_visits},
    {rtxd::CNT_PRIM_TESTS, &rtx_stats::prim_tests},
    {rtxd::CNT_HITS, &rtx_stats::hits},
    {rtxd::CNT_TEXEL_FETCHES, &rtx_stats::texel_fetches},
    {rtxd::CNT_RNG_DRAWS, &rtx_stats::rng_draws},
    {rtxd::CNT_WAVE_ITERS, &rtx_stats::wave_iters},
    {rtxd::CNT_LANE_STEPS, &rtx_stats::lane_steps},
    {rtxd::CNT_SHADE_PHASES, &rtx_stats::shade_phases},
    {rtxd::CNT_SHADE_LANES, &rtx_stats::shade_lanes},
    {rtxd::CNT_TRAV_CYCLES, &rtx_stats::trav_cycles},
    {rtxd::CNT_SHADE_CYCLES, &rtx_stats::shade_cycles},
    {rtxd::CNT_IDLE_LANES, &rtx_stats::idle_lanes},
    {rtxd::CNT_CACHE_HITS, &rtx_stats::cache_hits},
    {rtxd::CNT_PARKED_LANES, &rtx_stats::parked_lanes},
    {rtxd::CNT_DEFERRED_LANES, &rtx_stats::deferred_lanes},
    {rtxd::CNT_DEFERRED_PATHS, &rtx_stats::deferred_paths},
    {rtxd::CNT_REDO_CHUNKS, &rtx_stats::redo_chunks},
};
}  // namespace

// Wait for an enqueue_on(timed=true) and read its time and counters.
int collect_on(DeviceCopy* c, bool count, uint64_t samples, uint32_t chunks, rtx_stats* st) {
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    unsigned long long h[rtxd::COUNTER_SLOTS] = {0};
    HIP_TRY(hipMemcpy(h, c->counters.ptr, sizeof(h), hipMemcpyDeviceToHost));
    // any render on the device since the last report (this one, or one enqueued without stats before it)
    if (int rc = kerr_take(c->device)) return rc;
    std::memset(st, 0, sizeof(*st));
    for (const auto& f : kSummed) st->*f.field = h[f.slot];
    if (!count) st->samples = samples;
    for (int q = 0; q < 4; ++q) st->shade_split_cycles[q] = h[rtxd::CNT_SHADE_SPLIT + q];
    st->sample_chunks = chunks;
    st->kernel_ms = ms;
    st->scene_placement = c->placement;
    return RTX_OK;
}

void add_stats(rtx_stats* acc, const rtx_stats& s) {
    for (const auto& f : kSummed) acc->*f.field += s.*f.field;
    for (int q = 0; q < 4; ++q) acc->shade_split_cycles[q] += s.shade_split_cycles[q];
    acc->kernel_ms = std::max(acc->kernel_ms, s.kernel_ms);
    acc->sample_chunks = std::max(acc->sample_chunks, s.sample_chunks);
    acc->scene_placement = s.scene_placement;
}

// rtx_render_region_device with s->mu held by the caller.  Lock order everywhere: s->mu, then
// g_render_mu (rtx_render_ex, rtx_render_ppm), then g_scratch_mu (enqueue_on).
int render_region_locked(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region, float* d_out,
                         void* hip_stream, uint32_t flags, rtx_stats* stats) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, cur, &c)) return rc;
    const bool count = (flags & RTX_FLAG_COUNTERS) != 0;
    uint32_t chunks = 0;
    bool tiered = false;
    if (int rc = enqueue_on(s, c, cam, seed, region, d_out, (hipStream_t)hip_stream, flags, stats != nullptr, &chunks,
                            &tiered))
        return rc;
    if (!stats) return RTX_OK;
    const int rc = collect_on(c, count, (uint64_t)region_rows(region) * region->width * cam->samples_per_pixel, chunks, stats);
    stats->walk_layout = walk_layout(s, cam, tiered);
    return rc;
}

int ppm_to_host(int rc, const float* rgb, uint32_t W, uint32_t H, char* text, hipStream_t st, char* out_text,
                uint64_t capacity, uint64_t* out_len) {
    uint64_t len = 0;
    if (rc == RTX_OK) rc = rtx_encode_ppm_device(rgb, W, H, text, rtxd::ppm_max_bytes(W, H), &len, st);
    if (rc == RTX_OK && len > capacity) rc = fail(RTX_ERR_INVALID_ARG, "capacity %llu < PPM length %llu",
                                                  (unsigned long long)capacity, (unsigned long long)len);
    if (rc == RTX_OK && copy_to_host(out_text, text, len, st) != hipSuccess)
        rc = fail(RTX_ERR_HIP, "copying the PPM text to the host");
    if (st) (void)hipStreamSynchronize(st);
    if (rc == RTX_OK) *out_len = len;
    return rc;
}

}  // namespace rtxh

using namespace rtxh;

extern "C" {

int rtx_render_region_device(rtx_scene* s, const rtx_camera* cam, uint64_t seed, const rtx_region* region,
                             float* d_out, void* hip_stream, uint32_t flags, rtx_stats* stats) {
    g_last_error.clear();
    if (!s || !d_out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_region(cam, region)) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    return render_region_locked(s, cam, seed, region, d_out, hip_stream, flags, stats);
}

uint64_t rtx_ppm_max_bytes(uint32_t width, uint32_t height) { return rtxd::ppm_max_bytes(width, height); }

int rtx_encode_ppm_device(const float* d_rgb, uint32_t width, uint32_t height, char* d_text, uint64_t capacity,
                          uint64_t* out_len, void* hip_stream) {
    g_last_error.clear();
    if (!d_text || !out_len || (!d_rgb && (uint64_t)width * height)) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    const uint64_t n = (uint64_t)width * height;
    if (n > 0x7FFFFFFFull) return fail(RTX_ERR_INVALID_ARG, "image too large for the PPM encoder");
    const uint64_t need = rtxd::ppm_max_bytes(width, height);
    if (capacity < need) return fail(RTX_ERR_INVALID_ARG, "capacity %llu < rtx_ppm_max_bytes %llu",
                                     (unsigned long long)capacity, (unsigned long long)need);
    hipStream_t st = (hipStream_t)hip_stream;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    char header[64];
    const uint64_t hl = rtxd::ppm_header(width, height, header);
    HIP_TRY(hipMemcpyAsync(d_text, header, hl, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the header's stack buffer must outlive the copy
    uint64_t total = hl;
    if (n) {
        size_t sb = 0;
        HIP_TRY(rtxd::ppm_scratch_bytes(n, &sb));
        std::lock_guard<std::mutex> lk(g_ppm_mu);  // held until the encode has finished
        DeviceBuffer& ps = g_ppm[dev];
        HIP_TRY(ps.reserve(sb));
        uint64_t last_off = 0;
        uint32_t last_len = 0;
        hipError_t e = rtxd::ppm_encode(d_rgb, width, height, d_text, ps.ptr, ps.bytes, hl, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&last_off, rtxd::ppm_last_offset(ps.ptr, n), 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&last_len, rtxd::ppm_last_length(ps.ptr, n), 4, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);  // always: the copies target this frame
        HIP_TRY(e);
        HIP_TRY(es);
        total += last_off + last_len;
    }
    *out_len = total;
    return RTX_OK;
}

int rtx_render_ppm(rtx_scene* s, const rtx_camera* cam, uint64_t seed, char* out_text, uint64_t capacity,
                   uint64_t* out_len, rtx_stats* stats) {
    g_last_error.clear();
    if (!s || !out_text || !out_len) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_camera(cam)) return rc;
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint64_t need = rtxd::ppm_max_bytes(W, H);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(s->mu);  // (lock order: the scene, then the render buffers)
    std::lock_guard<std::mutex> bl(g_render_mu);  // the cached image / text buffers and stream
    hipStream_t st = render_stream(dev);
    float* rgb = static_cast<float*>(render_buffer(dev, -3, std::max<size_t>(1, (size_t)W * H * 3 * sizeof(float))));
    char* text = static_cast<char*>(render_buffer(dev, -4, need));
    if (!st) return fail(RTX_ERR_HIP, "stream on device %d", dev);
    if (!rgb || !text) return fail(RTX_ERR_OOM, "device buffers for a %ux%u PPM", W, H);
    rtx_region reg{0, 0, W, H, 0, 1};
    rtx_stats local;
    const int rc = render_region_locked(s, cam, seed, &reg, rgb, st, 0, stats ? stats : &local);
    return ppm_to_host(rc, rgb, W, H, text, st, out_text, capacity, out_len);
}

int rtx_render_ppm_ex(rtx_scene* s, const rtx_camera* cam, uint64_t seed, int n_gpus, char* out_text, uint64_t capacity,
                      uint64_t* out_len, rtx_stats* stats) {
    g_last_error.clear();
    if (!s || !out_text || !out_len) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_camera(cam)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    if (n_gpus <= 0) n_gpus = 1;
    if (n_gpus > ndev) return fail(RTX_ERR_INVALID_ARG, "n_gpus=%d but %d devices visible", n_gpus, ndev);
    const uint32_t W = cam->image_width, H = cam->image_height;
    const uint64_t need = rtxd::ppm_max_bytes(W, H);
    DeviceGuard restore;
    HIP_TRY(restore.error());
    std::lock_guard<std::mutex> lk(s->mu);  // (lock order: the scene, then the render buffers)
    std::lock_guard<std::mutex> bl(g_render_mu);
    float* img = nullptr;
    hipStream_t st = nullptr;
    rtx_stats local;
    // the bands rendered and assembled on device 0 as rtx_render_ex does, the image left there
    int rc = render_bands_locked(s, cam, seed, n_gpus, 0u, nullptr, &img, &st, stats ? stats : &local);
    if (rc == RTX_OK && hipSetDevice(0) != hipSuccess) rc = fail(RTX_ERR_HIP, "hipSetDevice(0)");
    char* text = rc == RTX_OK ? static_cast<char*>(render_buffer(0, -4, need)) : nullptr;
    if (rc == RTX_OK && !text) rc = fail(RTX_ERR_OOM, "device-0 buffer for a %ux%u PPM", W, H);
    return ppm_to_host(rc, img, W, H, text, st, out_text, capacity, out_len);
}

}  // extern "C"
