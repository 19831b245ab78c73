/*
 * rtx.h — C-ABI of the MI355X path-tracing megakernel (librtx.so).
 *
 * This is the drop-in boundary for the hot path of TwFlem/raytracer-go:
 *
 *   func (c *Camera) Render(world Hittable, writer io.Writer) error      internal/camera.go:180
 *
 * The reference runs the per-pixel / per-sample loop on the CPU
 * (internal/camera.go:254-299 -> internal/ray.go:32-54 -> internal/bvh.go:220-249 ->
 * internal/hittables.go:96-132 -> internal/materials.go:33-193).  A drop-in host
 * (the Go package via cgo, or the C++ mirror in raytracer-go_amd/host/) walks its
 * Hittable tree once, flattens it into the POD tables below, and calls
 * rtx_scene_create() + rtx_render() instead of spawning one goroutine per pixel.
 * PPM formatting (camera.go:183-188, 212-215) stays on the host.
 *
 * Rules of the ABI
 *  - POD structs only, fixed-width types, little-endian; every array is 16-B aligned.
 *  - The caller owns every input table and the output buffer for the duration of a
 *    call.  The library copies what it needs into device memory and never retains a
 *    caller pointer (cgo rule: C must not keep Go memory).
 *  - Functions return 0 on success and a negative RTX_ERR_* code on failure; the
 *    message is available from rtx_last_error() (thread-local).  No exception or
 *    abort crosses the ABI.  This is what Render's `error` return maps to
 *    (camera.go:180, 230).
 *  - rtx_render* are blocking and not re-entrant for one rtx_scene (internal mutex).
 */
#ifndef RTX_H
#define RTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 10

/* ---- status codes ------------------------------------------------------------ */
enum {
    RTX_OK = 0,
    RTX_ERR_INVALID_ARG = -1, /* null pointer, out-of-range index, bad size          */
    RTX_ERR_HIP = -2,         /* a HIP runtime call failed                            */
    RTX_ERR_RCCL = -3,        /* an RCCL call failed (multi-GPU gather)               */
    RTX_ERR_UNSUPPORTED = -4, /* a feature outside the GPU path (e.g. Perlin noise)   */
    RTX_ERR_NO_DEVICE = -5,   /* no gfx950 device visible                             */
    RTX_ERR_OOM = -6          /* device allocation failed                             */
};

/* ---- scene tables ------------------------------------------------------------ */

/* Child / root reference.  ref >= 0: index into rtx_scene_desc.nodes.
 * ref < 0: a primitive, p = ~ref, type = p >> 28 (RTX_PRIM_*), index = p & 0x0FFFFFFF.
 * RTX_PRIM_LIST (ABI 5): a World nested in the tree (a World handed to NewBVH as a child,
 * hittables.go:39-76): index into rtx_scene_desc.lists; its items are hit in order with a
 * running closest bound, (*World).Hit hittables.go:55-72. */
#define RTX_PRIM_SPHERE 0u
#define RTX_PRIM_QUAD 1u
#define RTX_PRIM_LIST 2u
#define RTX_REF_PRIM(type, index) ((int32_t) ~((int32_t)(((uint32_t)(type) << 28) | ((uint32_t)(index)&0x0FFFFFFFu))))

/* A BVH interior node exactly as internal/bvh.go:132-185 builds it: an AABB
 * (bvh.go:36-50, from NewAabbFromBoxes) and two children.  A one-element split
 * produces left == right (bvh.go:162-165); that is kept as-is in the table.
 * Every reachable node's box is ordered, bmin[k] <= bmax[k] on each axis, as NewAabb
 * makes it (flat and infinite boxes included); a node with bmin[k] > bmax[k] or a NaN
 * bound is rejected with RTX_ERR_INVALID_ARG.                                 32 B */
typedef struct rtx_bvh_node {
    float bmin[3];
    int32_t left;
    float bmax[3];
    int32_t right;
} rtx_bvh_node;

/* internal/hittables.go:78-94 (NewSphere).                                       32 B */
typedef struct rtx_sphere {
    float center[3];
    float radius;
    uint32_t material;
    uint32_t pad[3];
} rtx_sphere;

/* internal/hittables.go:138-165 (NewQuad) — derived fields as the constructor
 * computes them (w = n / dot(n, n), normal = Unit(n), d = dot(normal, q)).      80 B */
typedef struct rtx_quad {
    float q[3];
    uint32_t material;
    float u[3];
    float d;
    float v[3];
    float pad0;
    float w[3];
    float pad1;
    float normal[3];
    float pad2;
} rtx_quad;

/* Materials, internal/materials.go:9-119, 297-313.                               */
enum {
    RTX_MAT_LAMBERTIAN = 0,    /* albedo = textures[texture]       materials.go:23-42   */
    RTX_MAT_METAL = 1,         /* albedo[3], fuzz                  materials.go:44-75   */
    RTX_MAT_DIELECTRIC = 2,    /* ior                              materials.go:77-119  */
    RTX_MAT_DIFFUSE_LIGHT = 3  /* emit = textures[texture]         materials.go:297-313 */
};
typedef struct rtx_material { /* 32 B */
    uint32_t type;
    uint32_t texture;
    float fuzz;
    float ior;
    float albedo[3];
    float pad;
} rtx_material;

/* Textures, internal/materials.go:121-193, 280-295.                              */
enum {
    RTX_TEX_SOLID = 0,     /* even[3] = colour                       materials.go:151-163 */
    RTX_TEX_CHECKERED = 1, /* scale, even[3], odd[3]                 materials.go:121-145 */
    RTX_TEX_IMAGE = 2,     /* width x height RGBA16 texels at texel_offset (row-major,
                              y down), then ONE border texel: see below materials.go:165-193 */
    RTX_TEX_NOISE = 3      /* Perlin: scale, and RTX_NOISE_TEXELS words at texel_offset:
                              256 gradient vectors (x, y, z float32 bits), then permX,
                              permY, permZ (256 indices each)        materials.go:195-295 */
};
#define RTX_NOISE_TEXELS 1536u
/* RTX_TEX_IMAGE texels are Go's `img.At(x, y).RGBA()` (materials.go:188), 16 bits per
 * channel, two uint32 words per texel: word 0 = r | g << 16, word 1 = b | a << 16.
 * The texel at index width*height (after the raster) is the colour At() returns OUTSIDE
 * the image's bounds, which GetTexture reads when int(u*Dx) == Dx or int(v*Dy) == Dy
 * (u == 1, v == 0) or a NaN coordinate (int(NaN) = MinInt64 on amd64): for the
 * *image.YCbCr that jpeg.Decode returns that is color.YCbCr{} = (0, 34678, 0)
 * (image/ycbcr.go YCbCrAt, image/color/ycbcr.go RGBA), for *image.RGBA it is 0.
 * The host fills it with At(Bounds().Max.X, Bounds().Min.Y).RGBA().  Exact for every
 * image whose Bounds().Min is (0, 0) (jpeg.Decode, image.New*); texel_offset is even
 * and n_texels counts uint32 words.  Texels are fetched as
 * float32(r16) * float32(1/65535) (materials.go:187-191).                        */
#define RTX_IMAGE_TEXEL_WORDS 2u
typedef struct rtx_texture { /* 48 B */
    uint32_t type;
    float scale;
    uint32_t width;
    uint32_t height;
    float even[3];
    uint32_t texel_offset;
    float odd[3];
    float pad;
} rtx_texture;

/* A World nested in the tree: the refs list_refs[first .. first + count), in Add order.  8 B */
typedef struct rtx_list {
    uint32_t first;
    uint32_t count;
} rtx_list;

typedef struct rtx_scene_desc {
    const rtx_bvh_node* nodes;
    uint32_t n_nodes;
    uint32_t n_roots;
    /* The world handed to Render: a BVH gives one root ref (the tree); a plain World
     * (hittables.go:39-76, linear closest-hit scan in insertion order) gives its items. */
    const int32_t* roots;
    const rtx_sphere* spheres;
    uint32_t n_spheres;
    uint32_t n_quads;
    const rtx_quad* quads;
    const rtx_material* materials;
    uint32_t n_materials;
    uint32_t n_textures;
    const rtx_texture* textures;
    const uint32_t* texels; /* image RGBA16 texels and Perlin tables (uint32 words) */
    uint64_t n_texels;
    /* ABI 5: Worlds nested in the tree (RTX_PRIM_LIST refs); zero / NULL when there are none. */
    const rtx_list* lists;
    uint32_t n_lists;
    uint32_t n_list_refs;
    const int32_t* list_refs;
} rtx_scene_desc;

/* ---- camera ------------------------------------------------------------------ */
/* The derived state of Camera.init (internal/camera.go:128-165), computed by the
 * host exactly as the reference does and uploaded as kernel constants.           */
typedef struct rtx_camera {
    uint32_t image_width;       /* int(c.imageWidth)                     camera.go:181 */
    uint32_t image_height;      /* int(c.imageHeight)                    camera.go:182 */
    uint32_t samples_per_pixel; /* c.samplesPerPixel                     camera.go:256 */
    uint32_t max_depth;         /* c.bounceDepth                         camera.go:258 */
    float center[3];
    float defocus_angle; /* radians; > 0 enables the thin lens          camera.go:279 */
    float pixel00[3];
    float pad0;
    float pixel_du[3];
    float pad1;
    float pixel_dv[3];
    float pad2;
    float defocus_disk_u[3];
    float pad3;
    float defocus_disk_v[3];
    float pad4;
    float background[3];
    float pad5;
} rtx_camera;

/* ---- render region / shard ---------------------------------------------------- */
/* Pixels x in [x0, x0+width), rows y = y0 + r for r in [0, height) whose STRIPE
 * (r / stripe, stripes of `stripe` rows; 0 or 1: single rows) is rank modulo world:
 * stripes dealt round-robin to the shards, so sky and ground are balanced across GPUs.
 * Output rows are stored compacted in shard order: shard row i is image row
 * y0 + rtx_region_row(region, i).  The RNG is keyed by the GLOBAL pixel index
 * y*image_width + x, so every pixel's value is independent of the region, the stripe
 * and the shard count.  ABI 9 added `stripe` (a power of two, at most 4096): 8-row
 * stripes keep a shard's 8x8 work tiles compact in the image (rtx_render with
 * n_gpus > 1 uses them).                                          */
typedef struct rtx_region {
    uint32_t x0, y0, width, height;
    uint32_t rank, world;
    uint32_t stripe;
} rtx_region;



/* Work counters of one render (filled when RTX_FLAG_COUNTERS is set).  These are
 * the units of SURVEY.md §8(d): segments = world.Hit calls (ray.go:36).          */
typedef struct rtx_stats {
    uint64_t samples;
    uint64_t segments;
    uint64_t node_visits;  /* AABB slab tests   (bvh.go:221)                        */
    uint64_t prim_tests;   /* ray-primitive tests (hittables.go:96), duplicates of
                              a one-element split skipped (bit-identical, §8a a5)   */
    uint64_t hits;         /* segments that hit a primitive                          */
    uint64_t texel_fetches;
    uint64_t rng_draws;
    double kernel_ms;      /* device time of the render kernels, HIP events on the render
                              stream (n_gpus > 1: the slowest device)                */
    double gather_ms;      /* rtx_render with n_gpus > 1: the RCCL gather of the bands to
                              device 0 plus the de-interleave, HIP events on device 0  */
    /* scheduling counters of the persistent kernel (RTX_FLAG_COUNTERS):             */
    uint64_t wave_iters;   /* traversal-loop iterations, summed over waves           */
    uint64_t lane_steps;   /* lanes stepping a BVH entry, summed over iterations     */
    uint64_t shade_phases; /* shading phases, summed over waves                      */
    uint64_t shade_lanes;  /* lanes shaded or claiming, summed over shading phases   */
    uint64_t trav_cycles;  /* shader cycles (s_memtime) in traversal, summed over waves */
    uint64_t shade_cycles; /* shader cycles in shading phases, summed over waves      */
    uint64_t idle_lanes;   /* lanes with no item left, summed over iterations         */
    uint64_t cache_hits;   /* scenes too big for LDS: entries (of node_visits + prim_tests and
                              the steps on the end sentinel) read from the LDS cache of the top
                              levels */
    uint64_t sample_chunks; /* launches of the render kernel: the samples of every pixel run in
                               chunks that fit the per-device colour scratch (always filled) */
    uint64_t parked_lanes;   /* lanes parked on the end sentinel (waiting to shade, or without
                                an item) per walk step, summed over steps / steps per vote   */
    uint64_t deferred_lanes; /* lanes whose entry kind (node / primitive) a batched walk step
                                did not run, likewise                                        */
    uint64_t shade_split_cycles[4]; /* shade_cycles split: scatter sampling, shading, item claims +
                                       camera rays, segment starts (1/dir)                    */
    uint64_t walk_layout;   /* ABI 6: the layout walked: 0-7 = the camera octant of a rebuilt tree
                               (rtx_scene_topology), RTX_LAYOUT_REFERENCE = the caller's tree  */
    uint64_t gather_kind;   /* ABI 6, rtx_render: how the bands were assembled (RTX_GATHER_*)    */
    uint64_t scene_placement; /* ABI 6: where the walk read the scene (RTX_SCENE_IN_LDS / ...)    */
    uint64_t deferred_paths;  /* ABI 8, tiered walk: paths the near pass handed to the far pass  */
    uint64_t redo_chunks;     /* ABI 8, tiered walk: sample chunks whose queue of deferred paths
                                 overflowed: the samples that did not fit were rendered again from
                                 their camera rays on the far tree (the rest of the chunk is not) */
} rtx_stats;
#define RTX_SCENE_IN_HBM 0u    /* entries from HBM (through L2)                                   */
#define RTX_SCENE_IN_LDS 1u    /* the whole scene and its materials copied into LDS per workgroup */
#define RTX_SCENE_LDS_CACHE 2u /* top levels cached in LDS, the rest from HBM                     */
#define RTX_LAYOUT_REFERENCE 8u
#define RTX_LAYOUT_TIERED 16u  /* ABI 8: walk_layout bit: the render walked in two tiers (RTX_SCENE_NO_TIER) */
#define RTX_GATHER_NONE 0u   /* one band: it is the image                                        */
#define RTX_GATHER_RCCL 1u   /* ncclGather of the padded bands to device 0, de-interleave kernel  */
#define RTX_GATHER_DEVICE 2u /* RTX_SIM_BANDS (tests): bands on device 0, device copies, kernel   */
#define RTX_GATHER_HOST 3u   /* RCCL unavailable or failed (or RTX_NO_RCCL=1): each band's rows
                                copied into the caller's buffer                                 */

#define RTX_FLAG_COUNTERS 1u /* count work units (separate kernel instantiation) */
#define RTX_FLAG_NO_LDS 4u   /* A/B: read the scene from global memory even if it fits LDS */
#define RTX_FLAG_TIMING (1u << 20) /* diagnostics: the timed kernel with the wave-cycle split of
                                      rtx_stats (trav_cycles, shade_cycles, shade_split_cycles) */
/* Bits 2u, 8u, 16u, 32u, 64u and RTX_FLAG_WAVE_GEOM (bits 24-26) selected the A/B schedules
 * v0/v1/v2 of ABI 3; they were removed in ABI 4 and are ignored. */
/* Tuning: lanes of a wave that must wait before it shades (1..64; 0 = default, or the
 * RTX_SHADE_THRESH environment variable). */
#define RTX_FLAG_SHADE_THRESH(n) (((uint32_t)(n)&0x7Fu) << 8)

typedef struct rtx_scene rtx_scene;

/* ---- entry points ------------------------------------------------------------- */

/* ABI version (RTX_ABI_VERSION) and a static build string. */
int rtx_version(void);
const char* rtx_build_info(void);

/* Last error message of this thread ("" if none). */
const char* rtx_last_error(void);

/* Number of visible GPUs (0 if none). */
int rtx_device_count(void);

/* Validate the tables, convert them to the device layout and upload them once to
 * the current HIP device (replicated to further devices lazily by rtx_render).
 * Replaces the tree walk the reference does on every ray (bvh.go:220).           */
int rtx_scene_create(const rtx_scene_desc* desc, rtx_scene** out);

/* ABI 6.  rtx_scene_create with build flags.  By default a scene whose world is one BVH over
 * spheres (NewBVHFromWorld of a World of spheres, main.go:287) is walked over the library's
 * own tree of the same spheres: a binned surface-area-heuristic split, each node's near child
 * (along the camera's viewing direction) first.  The closest hit bvh.go:220-249 returns is
 * the nearest sphere root among the spheres whose boxes the ray passes, whichever tree the
 * boxes come from; the reference's tree (median splits on a random axis, bvh.go:142-185)
 * costs 1.8x the box tests and 4x the sphere tests on randSpheres (DESIGN.md §12 states the
 * floating-point caveat and how the tests check it).  RTX_SCENE_REFERENCE_BVH keeps the
 * caller's tree and the reference's visit order (left, then right) as they are; so do the
 * environment variable RTX_BVH=reference and every scene with quads, nested Worlds or a
 * World root.  rtx_scene_create(d, out) = rtx_scene_create_ex(d, 0, out).              */
#define RTX_SCENE_REFERENCE_BVH 1u
/* ABI 7.  The collapsed walk: a walk leaves out the box tests of tree nodes
 * whose children are all nodes where that saves tests on sample paths from the first camera
 * rendered with each layout.  A child's box lies inside its parent's and the slab test is
 * monotone in the box, so no primitive test, hit, path or image bit changes — only
 * rtx_stats.node_visits.  RTX_SCENE_EVERY_BOX (or RTX_COLLAPSE=0 in the environment) keeps
 * every box test, as bvh.go:220-249 makes them. */
#define RTX_SCENE_EVERY_BOX 2u
/* ABI 8.  The tiered walk.  A scene of spheres under one tree whose node
 * boxes contain the boxes of the spheres below them (every NewBVH tree) also gets a NEAR tree:
 * the spheres themselves as leaves, each behind its own box grown by the float32 sphere test's
 * derived error bound for ray origins inside a NEAR REGION (the box of the scene's non-huge
 * spheres, grown by 1.5 times its largest extent — by 1 % of it for scenes the rebuild's precision
 * gate refuses, config 4).  A render whose camera lies in the region walks every segment that starts
 * there on the near tree, and accepts a near hit only when the sphere's own box passes with the
 * bound just past it; a path whose segment starts outside the region, or whose near hit fails
 * that check, is handed, once, to a second pass that continues it on the FAR tree: the guarded
 * rebuild (the reference's leaves) when the scene has one, else the caller's own tree.  The
 * closest hit of every segment is the one bvh.go:220-249 returns, ties included (DESIGN.md §15
 * states why and what the tests check).  RTX_SCENE_NO_TIER (or RTX_TIER=0 in the environment)
 * walks the far tree alone; RTX_SCENE_REFERENCE_BVH keeps the caller's tree alone. */
#define RTX_SCENE_NO_TIER 4u
int rtx_scene_create_ex(const rtx_scene_desc* desc, uint32_t flags, rtx_scene** out);

/* The tree a rebuilt scene walks for camera octant `octant` (rtx_camera_octant): *n_nodes
 * nodes with `left` the child visited first; sphere refs index the caller's sphere table;
 * *root is the root ref.  nodes is filled when cap >= *n_nodes.  A scene that keeps the
 * caller's tree reports *n_nodes = 0, *root = -1.  For tests and tools.                */
int rtx_scene_topology(const rtx_scene* scene, uint32_t octant, rtx_bvh_node* nodes, uint32_t cap, uint32_t* n_nodes,
                       int32_t* root);
/* ABI 8: octant | RTX_TREE_NEAR names the near tree of a tiered scene (rtx_scene_topology,
 * rtx_walk_tree; *n_nodes = 0, *root = -1 when the scene has none). */
#define RTX_TREE_NEAR 0x100u

/* The same without a scene or a device: the tree rtx_scene_create_ex(desc, flags) walks for
 * `octant` (*n_nodes = 0, *root = -1 when it would keep the caller's).  Host only.       */
int rtx_walk_tree(const rtx_scene_desc* desc, uint32_t flags, uint32_t octant, rtx_bvh_node* nodes, uint32_t cap,
                  uint32_t* n_nodes, int32_t* root);

/* ABI 7.  The box tests the walk for `cam` leaves out: skip[k] = 1 for the k-th node entry of
 * the uncollapsed walk (the walked tree — rtx_scene_topology's, or the caller's — in visit
 * order: a node, then its first child's subtree, then its second's).  *n = the number of node
 * entries; skip is filled when cap >= *n.  The walk for a layout is planned on that layout's
 * first render (or on this call); later cameras of the same layout reuse it.  For tests and
 * tools (the oracle walks the same skips: parity of node_visits).                        */
int rtx_scene_walk_skip(rtx_scene* scene, const rtx_camera* cam, uint8_t* skip, uint32_t cap, uint32_t* n);

/* The same without a scene or a device: the skips rtx_scene_create_ex(desc, flags) plans for
 * a first render with `cam`.  Host only.                                                   */
int rtx_walk_skip(const rtx_scene_desc* desc, uint32_t flags, const rtx_camera* cam, uint8_t* skip, uint32_t cap,
                  uint32_t* n);

/* ABI 8.  The near region of a tiered scene (box = min xyz, max xyz; a segment whose origin o
 * has box[k] <= o[k] <= box[3 + k] for every k starts in it, a NaN origin does not; box is left
 * alone when the scene has no near tree), and *active = whether renders with `cam` qualify:
 * the camera's rays start in the region, spheres only, no Perlin texture (rtx_stats.walk_layout
 * & RTX_LAYOUT_TIERED says that a render walked in two tiers).  For tests and tools. */
int rtx_scene_near_region(rtx_scene* scene, const rtx_camera* cam, float box[6], uint32_t* active);
/* ABI 8.  rtx_scene_walk_skip of the near walk for `cam` (over rtx_scene_topology's
 * octant | RTX_TREE_NEAR tree). */
int rtx_scene_near_skip(rtx_scene* scene, const rtx_camera* cam, uint8_t* skip, uint32_t cap, uint32_t* n);
/* ABI 8.  The same without a scene or a device: the near region rtx_scene_create_ex(desc,
 * flags) would walk with and *active for `cam`.  Host only. */
int rtx_walk_near_region(const rtx_scene_desc* desc, uint32_t flags, const rtx_camera* cam, float box[6],
                         uint32_t* active);

/* Octant of the camera's viewing direction (pixel00 + du W/2 + dv H/2 - center): bit k set
 * when it points to negative axis k. */
uint32_t rtx_camera_octant(const rtx_camera* cam);

/* Release device memory owned by the scene (NULL is a no-op). */
void rtx_scene_destroy(rtx_scene* scene);

/* Size of the device layout in bytes (entries + materials + textures + texels). */
uint64_t rtx_scene_device_bytes(const rtx_scene* scene);

/* The whole of Camera.Render's pixel loop (camera.go:198-222): render every pixel
 * of the image, averaged over samples_per_pixel, linear (pre-gamma) float32 RGB,
 * row-major, rows top to bottom, into caller-owned host memory out_rgb[W*H*3].
 * n_gpus > 1 row-interleaves the image over devices 0..n_gpus-1 of this process
 * (rank d renders rows y = d, d + n, ...), gathers the equal-sized bands to device 0
 * with one RCCL ncclGather over xGMI (communicators from ncclCommInitAll, cached per
 * device set; librccl is loaded on first use), de-interleaves them on device 0 and
 * copies the image to the host.  Without RCCL (not loadable, or a failing
 * CommInitAll / Gather) each band's rows are copied into out_rgb instead: slower,
 * same bits (stats->gather_kind says which).  The band, gather and image buffers are
 * kept per device between calls (rtx_release_device_memory frees them).
 * stats (optional) receives the time (kernel_ms, gather_ms), samples, sample_chunks,
 * walk_layout and gather_kind of the call; its work counters stay 0: rtx_render runs the
 * timed kernel.  rtx_render = rtx_render_ex(..., flags = 0, ...).                     */
int rtx_render(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, int n_gpus, float* out_rgb,
               rtx_stats* stats);

/* ABI 6: rtx_render with flags: RTX_FLAG_COUNTERS runs the counting kernel instead (same
 * image; every work counter of stats filled; about twice the kernel time of the timed
 * kernel on the headline config).                                                     */
int rtx_render_ex(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, int n_gpus, uint32_t flags,
                  float* out_rgb, rtx_stats* stats);

/* Free the device memory the library keeps between renders on `device` (-1: every
 * device): the per-device sample-colour scratch (up to RTX_SCRATCH_MB, 12 B per
 * sample of a chunk) and the cached RCCL communicators.  Scenes are not affected;
 * the next render allocates again.  The scratch of a device is also freed when the
 * last scene with a copy on that device is destroyed.  Blocking.                   */
int rtx_release_device_memory(int device);

/* Bytes of the per-device scratch currently held on `device` (for tests and tools). */
uint64_t rtx_device_scratch_bytes(int device);

/* ABI 10.  Wait for every render enqueued on `device` and report whether any of them failed inside the
 * kernel since the last report: RTX_OK, or RTX_ERR_HIP when a wave hit the watchdog (RTX_WATCHDOG_S) or
 * reached a wave-level claim without the whole wave (the output of that render is then invalid).  The
 * kernel's error word is sticky: no later render clears it, so renders enqueued back to back without
 * stats (rtx_render_region_device with stats == NULL) are checked by ONE call after the last of them.
 * A render that returns stats reports (and acknowledges) the same word itself.  The report is
 * acknowledged: a second call without a failed render in between returns RTX_OK.  Blocking.
 * The Go side: the error a pipelined Render loop returns once (camera.go:180, 230). */
int rtx_device_check(int device);

/* Render one region/shard on the CURRENT device into device memory d_out (float32
 * RGB, compacted shard rows, see rtx_region) on the given HIP stream (hipStream_t,
 * NULL = default stream).  Returns after enqueueing unless stats != NULL, in which
 * case it synchronises the stream and fills stats (kernel_ms from HIP events
 * recorded on that same stream).  This is the entry a one-process-per-GPU launcher
 * (torch.distributed / RCCL) uses.                                               */
int rtx_render_region_device(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, const rtx_region* region,
                             float* d_out, void* hip_stream, uint32_t flags, rtx_stats* stats);

/* Number of output rows of a region shard: the rows of the stripes rank, rank + world, ... that
 * lie in [0, height) (ceil((height - rank) / world) for single-row stripes). */
uint32_t rtx_region_rows(const rtx_region* region);
/* ABI 9.  The row (relative to y0) of shard row i of a region: row i % S of stripe (i / S) * world + rank
 * (S = max(stripe, 1)). */
uint32_t rtx_region_row(const rtx_region* region, uint32_t i);

/* ---- BVH build on the GPU ----------------------------------
 * rtx_scene_create for NewBVHFromWorld(world) (bvh.go:138-185) of a World holding only
 * spheres, with the BVH built on the current device instead of by the caller: spheres
 * in World.Add order; the k-th NewBVH call (pre-order) takes Intn(3) from word
 * bvh_draw0 + k of the global host stream of bvh_seed (the RNG contract, DESIGN.md
 * §3), which is the axis the host builder draws.  The scene equals the one
 * rtx_scene_create makes from NewBVHFromWorld's tree over this sphere table: the same
 * entries byte for byte, a sphere entry's sphere word being the index into `spheres`
 * (Add order), so rtx_hit.prim and rtx_light.prim name the caller's spheres
 * (tests/test_bvh_gpu.py against tests/bvh_ref.py).  A tree built over a reordered
 * copy of the table, as the host mirror's, differs in that word alone.  build_ms
 * (optional) receives the build's wall time.                                        */
int rtx_scene_create_spheres(const rtx_sphere* spheres, uint32_t n_spheres, const rtx_material* materials,
                             uint32_t n_materials, const rtx_texture* textures, uint32_t n_textures,
                             const uint32_t* texels, uint64_t n_texels, uint64_t bvh_seed, uint64_t bvh_draw0,
                             rtx_scene** out, double* build_ms);

/* The same for a World of spheres and quads (ABI 10, additive): rtx_scene_create for
 * NewBVHFromWorld(world), the BVH built on the current device.  items[0 .. n_items) is the
 * World's list in World.Add order, each item RTX_REF_PRIM(RTX_PRIM_SPHERE or RTX_PRIM_QUAD,
 * index into `spheres` / `quads`).  The scene equals the one rtx_scene_create makes from
 * NewBVHFromWorld's tree over these tables: the same entries byte for byte, a leaf's index word
 * being the item's index into the CALLER's table (so rtx_hit.prim and rtx_light.prim name the
 * caller's primitives).  A quad's box, which the comparators read, is NewQuad's padded one
 * (hittables.go:161, bvh.go:63-82) computed from q, u, v; its entry takes normal and d from the
 * record (rtx_quad_init derives them).  The sorts are stable, and the k-th NewBVH call (pre-order)
 * takes Intn(3) from word bvh_draw0 + k of host stream 1 of bvh_seed, as for spheres
 * (tests/test_world_bvh_gpu.py against tests/world_bvh_ref.py).
 *  - items == NULL means every sphere in table order, then every quad in table order; n_items
 *    must then equal n_spheres + n_quads.
 *  - A primitive no item names is uploaded, never hit, and is no emitter.  A primitive named
 *    twice (the same Hittable added twice) gives two entries.  (Where both items of one
 *    two-item NewBVH call name the same primitive, the node's children are two entries here, as
 *    the reference tests both; rtx_scene_create reads left == right as the one-element split and
 *    would emit one.  Hits and colours are the same, the primitive-test count is not.)
 *  - Returned as RTX_ERR_INVALID_ARG before any device is touched: a NULL out, n_items == 0
 *    (bvh.go:163 indexes h[0]), n_items > 2^25, an item that is a node ref (>= 0), a list ref, of
 *    an unknown type or with an index outside its table, and everything rtx_scene_create refuses
 *    in the primitive, material, texture and texel tables.
 *  - A box with a NaN bound (a NaN or inf - inf in q, u, v, centre or radius) is out of contract:
 *    the comparator is no order there.
 * build_ms (optional) receives the build's wall time.                                  */
int rtx_scene_create_world(const int32_t* items, uint32_t n_items, const rtx_sphere* spheres, uint32_t n_spheres,
                           const rtx_quad* quads, uint32_t n_quads, const rtx_material* materials,
                           uint32_t n_materials, const rtx_texture* textures, uint32_t n_textures,
                           const uint32_t* texels, uint64_t n_texels, uint64_t bvh_seed, uint64_t bvh_draw0,
                           rtx_scene** out, double* build_ms);

/* NewQuad (hittables.go:149-165) in float32, every operation rounded on its own: n = Cross(u, v),
 * normal = n * (1 / float32(sqrt(float64(Dot(n, n))))), d = Dot(normal, q), w = n * (1 / Dot(n, n));
 * the pads are zero.  A degenerate quad (u x v = 0) gets NaN or infinite fields, as in the
 * reference.  Host only; a NULL pointer returns RTX_ERR_INVALID_ARG.                   */
int rtx_quad_init(const float q[3], const float u[3], const float v[3], uint32_t material, rtx_quad* out);

/* Box (hittables.go:200-216): the six quads of the box spanned by the corners a and b, in the
 * reference's order (front, right, back, left, top, bottom), the negated edges being Scale(dz, -1)
 * and Scale(dx, -1) as written (their zero components are -0).  Host only.             */
int rtx_box_quads(const float a[3], const float b[3], uint32_t material, rtx_quad out[6]);

/* Copy the scene's threaded BVH entries (32 B each, rtx_layout.h order) to out when
 * cap is large enough; returns their size in bytes.  For tests and tools.            */
uint64_t rtx_scene_export(const rtx_scene* scene, void* out, uint64_t cap);

/* ---- PPM output on the GPU ---------------------------------
 * Render's output tail, camera.go:183-188 and 212-215 with vec3.go:141-166: the P3
 * header "P3\n<W> <H>\n255\n", then per pixel int(Clamp(0,1,float32(sqrt(c)))*255.999)
 * for R, G, B as "%d %d %d\n" (a NaN channel prints Go's int(NaN) = MinInt64).     */

/* Upper bound of the PPM text of a width x height image (header + 63 B per pixel). */
uint64_t rtx_ppm_max_bytes(uint32_t width, uint32_t height);

/* Encode a float32 RGB image in device memory (d_rgb, width*height*3, row-major) into
 * device memory d_text (capacity bytes) on the current device and the given stream;
 * synchronises that stream and stores the text length in *out_len.  Replaces the
 * reference's per-pixel fmt.Sprintf + channel pipeline (camera.go:198-231).          */
int rtx_encode_ppm_device(const float* d_rgb, uint32_t width, uint32_t height, char* d_text, uint64_t capacity,
                          uint64_t* out_len, void* hip_stream);

/* Render + encode on the current device and copy the PPM text to the caller's host
 * buffer: the bytes (*Camera).Render(world, writer) writes (camera.go:180).  Blocking. */
int rtx_render_ppm(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, char* out_text, uint64_t capacity,
                   uint64_t* out_len, rtx_stats* stats);

/* ABI 9.  rtx_render_ppm for n_gpus devices: the bands rendered and gathered to device 0 exactly
 * as rtx_render(n_gpus) does (one RCCL ncclGather over xGMI and the de-interleave kernel, or the
 * per-band copies without RCCL), then the PPM encoded ON device 0 (rtx_encode_ppm_device) and only
 * the text copied to the caller: the multi-GPU (*Camera).Render(world, writer) of camera.go:180-231
 * with no per-pixel formatting on the host.  Devices 0..n_gpus-1 (n_gpus <= 1: device 0, one band;
 * RTX_SIM_BANDS=k simulates k bands on device 0 as rtx_render does).  The bytes equal
 * rtx_render_ppm's for any n_gpus.  stats as rtx_render's.  Blocking. */
int rtx_render_ppm_ex(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, int n_gpus, char* out_text,
                      uint64_t capacity, uint64_t* out_len, rtx_stats* stats);

/* ---- progressive rendering (ABI 10, additive) -------------------
 * rtx_render* run samples_per_pixel samples in one blocking call (camera.go:256-261).  An
 * rtx_accum renders them in PASSES of the caller's size and can be looked at in between: after n
 * accumulated samples the resolved image is, bit for bit, what a one-shot render of the same
 * region with samples_per_pixel = n returns, for every n and any split into passes.
 *
 * An accumulator belongs to one scene, one device (the device current at create) and one
 * (camera, seed, region), all copied at create; the camera's samples_per_pixel is not used by it
 * (a host wrapper uses it as its target).  Per pixel of the region's shard it holds float32
 * S[3] and Q[3], and n, the samples done: all zero at create and after reset.  A pass adds, for
 * every pixel and channel, in k order:  S = S + c;  Q = Q + c * c  (the product rounded to
 * float32 before the add), c being the colour the one-shot render computes for sample k.
 *
 * Rules
 *  - The caller orders the passes and resolves of ONE accumulator: the same stream, or a
 *    synchronise between them.  Different accumulators are independent.
 *  - Accumulators are destroyed before their scene.
 *  - A call with another device current than the accumulator's returns RTX_ERR_INVALID_ARG.
 *  - S and Q belong to the accumulator, not to the per-device scratch: other renders on the
 *    device do not disturb them, rtx_device_scratch_bytes does not count them and
 *    rtx_release_device_memory does not touch accumulators.
 *  - Several GPUs work as for rtx_render_region_device: one accumulator per rank's shard, on
 *    that rank's device; shards are independent.
 *  - The variance is Q/n - mean^2, which cancels: its error is about n * 2^-24 of mean^2, so on
 *    a constant pixel it comes out as a small value of either sign and is clamped at 0 (323 of
 *    the 3888 channel values of randSpheres 48x27 at 8 samples, all on constant sky).          */
typedef struct rtx_accum rtx_accum;

/* Validates as rtx_render_region_device does; allocates and zeroes 24 B per pixel slot of the
 * region's shard (64-pixel tiles, ragged tiles padded) on the current device.  The zeroes are in place on return: a
 * pass may follow at once on any stream, a non-blocking one included. */
int rtx_accum_create(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, const rtx_region* region,
                     rtx_accum** out);

/* One pass: renders samples k = n .. n + count - 1 of every pixel on hip_stream and sets
 * n += count.  count == 0, or n + count past 2^32 - 1, returns RTX_ERR_INVALID_ARG.  flags as for
 * rtx_render_region_device.  Returns after enqueueing unless stats != NULL; then it synchronises
 * and fills stats for THIS pass: samples = pixels * count, sample_chunks, kernel_ms, walk_layout,
 * and with RTX_FLAG_COUNTERS the work counters of this pass alone.  The sticky error word works
 * as for any render (rtx_device_check). */
int rtx_accum_add(rtx_accum* accum, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats);

/* n, the samples accumulated per pixel (0 for NULL). */
uint32_t rtx_accum_samples(const rtx_accum* accum);

/* The image after n >= 1 samples into device memory, on hip_stream: d_rgb, and d_var when not
 * NULL, hold the region's compacted shard rows (rtx_region), row-major, 3 floats per pixel.  All
 * arithmetic is float32, each operation rounded (no fused multiply-add, no square root):
 *     inv   = 1.0f / (float)n
 *     rgb_c = S_c * inv
 *     d     = Q_c * inv - rgb_c * rgb_c
 *     v     = d > 0 ? d : 0                       (a NaN gives 0)
 *     var_c = v * inv                             the biased variance of the pixel mean
 *     sv    = (var_r + var_g) + var_b
 *     mb    = (rgb_r + rgb_g) + rgb_b
 *     t     = rel_tol * (mb > 0.01f ? mb : 0.01f)
 * and a pixel is NOISY when sv > t * t.  *noisy (when not NULL) receives the number of noisy
 * pixels, and the call then synchronises the stream; else it returns after enqueueing.  The
 * accumulator is not modified: more passes may follow. */
int rtx_accum_resolve_device(rtx_accum* accum, float* d_rgb, float* d_var, float rel_tol, void* hip_stream,
                             uint64_t* noisy);

/* The same into host memory, after every render enqueued on the device so far.  out_var and noisy
 * may be NULL; so may out_rgb when noisy is not (the count alone: a stopping rule that needs no
 * image).  Blocking. */
int rtx_accum_resolve(rtx_accum* accum, float* out_rgb, float* out_var, float rel_tol, uint64_t* noisy);

/* Resolve, rtx_encode_ppm_device, and the text copied to the caller's host buffer (capacity at
 * least rtx_ppm_max_bytes(region width, shard rows)).  For a whole-image region the bytes equal
 * rtx_render_ppm's at samples_per_pixel = n.  Blocking. */
int rtx_accum_ppm(rtx_accum* accum, char* out_text, uint64_t capacity, uint64_t* out_len);

/* Back to n = 0 with S and Q zero, after everything enqueued on the device.  Blocking: S and Q are zero on return,
 * so a pass may follow at once on any stream. */
int rtx_accum_reset(rtx_accum* accum);

/* Frees the accumulator's device memory (NULL is a no-op).  Blocking. */
void rtx_accum_destroy(rtx_accum* accum);

/* ---- adaptive sampling (ABI 10, additive) --------------------------
 * rtx_accum_add samples every pixel in every pass, so "stop when clean" means "stop when the LAST
 * pixel is clean".  An ADAPTIVE pass samples only the tiles that still hold a noisy pixel.  It is a
 * separate, opt-in entry: rtx_render* and rtx_accum_add compute what they computed before.
 *
 * State.  An accumulator holds one word per TILE of its S / Q layout: open, or closed at n.  A
 * tile is tile_width x tile_height pixels of the shard (rtx_accum_tile_shape; 64 pixels), tiles
 * start at the region's x0 and at shard row 0 (the compacted rows of rtx_region), and the tiles of
 * the right and bottom edges may be partial.  All tiles are open at create and after
 * rtx_accum_reset.  rtx_accum_samples stays the FRONTIER n: the samples offered so far.  Pixel p
 * has received n_p samples: n when its tile is open, else the n at which its tile closed.
 *
 * The contract that replaces "equal to the one-shot render at n":  a pixel with n_p samples is, bit
 * for bit, that pixel of a one-shot render of the same region at samples_per_pixel = n_p.
 *
 * rtx_accum_add_adaptive does three things in order, all enqueued on hip_stream, with no host
 * round trip in between:
 *  1. SELECT.  If n >= max(min_samples, 1): every open tile NONE of whose pixels is NOISY is closed
 *     at n.  NOISY is rtx_accum_resolve_device's test at (n, rel_tol), the same float32 operations.
 *     A NaN pixel is not noisy (its comparison is false) and keeps no tile open.  A closed tile
 *     never reopens before a reset.
 *  2. SAMPLE.  The samples k = n .. n + count - 1 of every pixel of every tile still open are
 *     rendered and folded into S and Q exactly as rtx_accum_add does.  A closed tile's S and Q are
 *     not touched.
 *  3. n += count, whether or not a tile was open: the host does not know, and does not wait to
 *     find out.
 * count == 0, n + count past 2^32 - 1, !(rel_tol >= 0) (a NaN, a negative tolerance) and a NULL
 * accumulator return RTX_ERR_INVALID_ARG before any device is touched.  So does rtx_accum_add on an
 * accumulator that has taken an adaptive pass, until it is reset: its tiles no longer share one n.
 *
 * A non-NULL stats or adapt_stats synchronises the stream.  adapt_stats: the accumulator's tiles,
 * the tiles this pass sampled and the pixels in them.  open_tiles == 0 is the caller's stop signal
 * (such a pass renders nothing, and completes).  stats as rtx_accum_add's, for the samples this
 * pass rendered: samples = open_pixels * count, kernel_ms (the selection not included), and with
 * RTX_FLAG_COUNTERS the work counters of exactly those samples.
 *
 * Everything that reads an accumulator uses n_p: rtx_accum_resolve* computes inv = 1.0f /
 * (float)n_p per pixel and counts the noisy pixels at each pixel's own n_p; rtx_accum_ppm and
 * rtx_accum_preview* resolve likewise (the preview's guides stay over [0, min(n, guide_samples)):
 * they do not depend on the accumulator's contents).  An accumulator that never took an adaptive
 * pass runs the kernels and launches it ran before.
 *
 * BIAS.  Stopping on an ESTIMATE of the noise biases the result: a tile that has not yet seen its
 * first firefly (a rare bright sample) looks clean, closes early and stays too dark; min_samples is
 * the guard.  Neighbouring tiles that stop at different n differ in noise level, so tile edges can
 * show at loose tolerances.  Not provided: per-pixel granularity, dilation of the open tiles,
 * reopening, and a gather of accumulators across GPUs (each rank's shard selects on its own).   */
typedef struct rtx_adapt_stats {
    uint64_t tiles;       /* tiles of the accumulator's shard */
    uint64_t open_tiles;  /* tiles this pass sampled */
    uint64_t open_pixels; /* the pixels of the shard in them */
} rtx_adapt_stats;

int rtx_accum_add_adaptive(rtx_accum* accum, uint32_t count, float rel_tol, uint32_t min_samples, void* hip_stream,
                           uint32_t flags, rtx_stats* stats, rtx_adapt_stats* adapt_stats);

/* The accumulator's tile: tile_width x tile_height pixels (a reference can reproduce the selection). */
int rtx_accum_tile_shape(const rtx_accum* accum, uint32_t* tile_width, uint32_t* tile_height);

/* n_p of every pixel of the region's compacted shard rows, row-major, one uint32 each: a heat map
 * of where the samples went.  Into device memory on hip_stream (enqueued), or into host memory
 * after every render enqueued on the device so far (blocking).  Before any adaptive pass every
 * value is n. */
int rtx_accum_sample_counts_device(rtx_accum* accum, uint32_t* d_counts, void* hip_stream);
int rtx_accum_sample_counts(rtx_accum* accum, uint32_t* out_counts);

/* ---- ray queries (ABI 10, additive) ------------------------------
 * The question under Render, the reference's own public interface:
 *   Hittable.Hit(r *Ray, rayT Interval) (HitInfo, bool)          hittables.go:7-20, bvh.go:220-249
 * for a batch of the CALLER's rays against the world handed to rtx_scene_create*: picking, auto-focus,
 * shadow and occlusion rays, first-hit guide images, an integrator written elsewhere.
 *
 * Closest hit.  Hit i is what world.Hit(ray_i, Interval{tmin, tmax}) returns:
 *  - the running bound starts at tmax; Interval.In is strict at both ends (bvh.go:18-20), so a root equal
 *    to tmin or tmax is no hit; Aabb.Hit gets (tmin, running bound) (bvh.go:52-61, 84-102);
 *  - equal roots are resolved as the reference's walk resolves them, whichever tree is walked (the
 *    render's rank rule): of two spheres with the same root, the one the reference's walk
 *    meets first;
 *  - tmin >= tmax is a miss, and so is a NaN tmin or tmax (every comparison with it is false);
 *  - NaN, infinite and zero origin and direction components are legal and take the IEEE forms of the Go
 *    code (1 / 0 = inf, 0 * inf = NaN fails `t0 > min`), as in a render.
 * `prim` names the caller's table index whichever tree was walked; `material` indexes
 * rtx_scene_desc.materials.  point = r.At(t) (ray.go:25-30); normal is unit and flipped against the ray,
 * front_face says whether it had to be (NewHitInfo, hittables.go:22-37).  A miss: t = +inf,
 * prim = RTX_HIT_NONE, every other field 0.
 * RTX_TRACE_ANY: each ray stops at the first primitive it accepts (a shadow ray); only
 * prim != RTX_HIT_NONE is specified, and it holds for exactly the rays whose closest hit exists (the two
 * walks take the same steps with the same bound, tmax, up to the first accepted primitive).
 * n == 0 returns RTX_OK and launches nothing.  A NULL scene, ray or hit pointer, a ray or hit pointer
 * not aligned to 16 B, flag bits other than those below, and (rtx_trace_device) a current device that
 * holds no copy of the scene return RTX_ERR_INVALID_ARG.
 * A trace takes the scene's mutex like a render.  It uses none of the per-device sample scratch
 * (rtx_device_scratch_bytes is unchanged by it, rtx_release_device_memory does not disturb it), walks
 * layouts of its own (a render's walk, and so its node_visits, is what it is without the trace) and
 * keeps its counters in memory of its own: a counting trace between two renders changes neither's stats. */
typedef struct rtx_ray { /* 32 B */
    float origin[3];
    float tmin;
    float dir[3]; /* any length: t is in units of it, as in the reference */
    float tmax;
} rtx_ray;
typedef struct rtx_hit { /* 48 B */
    float t;             /* HitInfo.t; +inf on a miss                                        */
    uint32_t prim;       /* type << 28 | index into the CALLER's sphere / quad table (RTX_PRIM_*);
                            RTX_HIT_NONE on a miss                                           */
    uint32_t material;   /* index into rtx_scene_desc.materials                              */
    uint32_t front_face; /* 1: the ray came from outside (dot(dir, outward normal) < 0)      */
    float point[3];      /* r.At(t), ray.go:25-30                                            */
    float u;
    float normal[3];     /* unit, flipped against the ray: NewHitInfo, hittables.go:22-37    */
    float v;
} rtx_hit;
#define RTX_HIT_NONE 0xFFFFFFFFu
#define RTX_TRACE_ANY 1u      /* stop at the lane's first accepted primitive; only prim != RTX_HIT_NONE is specified */
#define RTX_TRACE_UV 2u       /* fill u, v (sphere: hittables.go:122-126; quad: alpha, beta); else 0 */
#define RTX_TRACE_COUNTERS 4u /* counting instantiation: hits, node_visits, prim_tests (with stats only) */
/* hint: the direction signs (rtx_camera_octant's bits) the tree's child order should suit; a scene that
 * walks its own trees (rtx_scene_create_ex) has one per octant.  Every hint gives the same hits. */
#define RTX_TRACE_OCTANT(o) (((uint32_t)(o)&7u) << 8)
typedef struct rtx_trace_stats {
    uint64_t rays;
    uint64_t hits;            /* RTX_TRACE_COUNTERS: rays with a hit                                  */
    uint64_t node_visits;     /* RTX_TRACE_COUNTERS: AABB slab tests (bvh.go:221), as rtx_stats'      */
    uint64_t prim_tests;      /* RTX_TRACE_COUNTERS: ray-primitive tests, as rtx_stats'               */
    uint64_t walk_layout;     /* the hinted octant of a rebuilt tree, or RTX_LAYOUT_REFERENCE         */
    uint64_t scene_placement; /* RTX_SCENE_IN_LDS or RTX_SCENE_IN_HBM                                 */
    double kernel_ms;         /* device time of the launches, HIP events on the stream                */
} rtx_trace_stats;

/* Rays and hits in device memory of the CURRENT device, on the given HIP stream (hipStream_t, NULL =
 * default stream).  Returns after enqueueing unless stats != NULL; then it synchronises the stream and
 * fills stats.  The trace layout and the rank table are uploaded on the first trace that needs them
 * (blocking copies).  n beyond what one launch indexes in 32 bits is cut into several launches. */
int rtx_trace_device(rtx_scene* scene, const rtx_ray* d_rays, uint64_t n, rtx_hit* d_hits, uint32_t flags,
                     void* hip_stream, rtx_trace_stats* stats);
/* The same for rays and hits in host memory, on the current device.  Blocking. */
int rtx_trace(rtx_scene* scene, const rtx_ray* rays, uint64_t n, rtx_hit* hits, uint32_t flags,
              rtx_trace_stats* stats);

/* ---- path building blocks (ABI 10, additive) ---------------------
 * The other two public calls under Render, for a batch:
 *   Camera.GetRay                                  camera.go:265-299
 *   Material.Emit + Material.Scatter               ray.go:41-42, materials.go:23-113, 297-313
 * with the four textures and the Philox draw order of DESIGN.md §3, computed by the same device code as a
 * render.  GetRay -> Hit -> Scatter in a loop is Ray.GetColor (ray.go:32-54), so with rtx_trace they compose
 * into an integrator of the caller's own.  This loop IS a render: on a scene that keeps the caller's tree
 * (RTX_SCENE_REFERENCE_BVH) its colours equal rtx_render*'s bit for bit (float32, each operation rounded, no fused
 * multiply-add) and its segments, hits, draws and texel fetches are the render's; on the library's own trees a
 * trace may resolve a rare grazing hit differently from the render's walk:
 *
 *   rays, keys = camera_rays(region, first, count);  T = 1;  L = 0;  alive = all
 *   repeat max_depth times:
 *       hits = trace(rays, RTX_TRACE_UV);  b = shade(rays, hits, keys)
 *       miss & alive:  L += T * background;  alive = false
 *       hit  & alive:  if EMITS: L += T * emitted
 *                      if SCATTERED: T *= attenuation;  rays = b.ray;  keys.event += 1   else alive = false
 *   colour(pixel) = (sum of L over k, in k order) * (1 / spp)
 *
 * An ended path needs no compaction: its bounce ray is all zero, tmin >= tmax is a miss in rtx_trace, and a miss
 * shades to an all-zero bounce again. */
typedef struct rtx_path_key { /* 16 B: the Philox counter of DESIGN.md §3 without the attempt */
    uint32_t pixel;           /* GLOBAL pixel index y * image_width + x                          */
    uint32_t sample;          /* k                                                               */
    uint32_t event;           /* 0 = GetRay; s + 1 = the scatter after segment s                 */
    uint32_t draws;           /* written by rtx_camera_rays*: rand.Float32() calls GetRay made;
                                 ignored on input                                                */
} rtx_path_key;

typedef struct rtx_bounce { /* 64 B */
    float attenuation[3];   /* ScatterInfo.attenuation; 0 when not scattered                       */
    uint32_t flags;         /* RTX_BOUNCE_SCATTERED | RTX_BOUNCE_EMITS                             */
    float emitted[3];       /* material.Emit(u, v, point): the texture of a DiffuseLight, else 0   */
    uint32_t rng_draws;     /* rand.Float32() calls Scatter made (3 per unit-sphere attempt,
                               1 for a Dielectric that can refract)                                */
    rtx_ray ray;            /* ScatterInfo.ray with GetColor's interval: origin = hit.point,
                               dir, tmin = 0.001f, tmax = +inf; all zero when not scattered        */
} rtx_bounce;
#define RTX_BOUNCE_SCATTERED 1u
#define RTX_BOUNCE_EMITS 2u /* the material is a DiffuseLight */
#define RTX_SHADE_COUNTERS 1u /* counting instantiation: hits, scattered, rng_draws, texel_fetches (with stats only) */
typedef struct rtx_shade_stats {
    uint64_t n;             /* records                                                             */
    uint64_t hits;          /* RTX_SHADE_COUNTERS: records with a hit                              */
    uint64_t scattered;     /* RTX_SHADE_COUNTERS: records with RTX_BOUNCE_SCATTERED               */
    uint64_t rng_draws;     /* RTX_SHADE_COUNTERS: the sum of rtx_bounce.rng_draws                 */
    uint64_t texel_fetches; /* RTX_SHADE_COUNTERS: image-texture lookups, as rtx_stats'            */
    double kernel_ms;       /* device time of the launches, HIP events on the stream               */
} rtx_shade_stats;

/* GetRay for samples k = first_sample .. first_sample + count - 1 of every pixel of the region's shard, into
 * device memory of the CURRENT device on the given HIP stream; returns after enqueueing.  Needs no scene.  The
 * camera and the region are validated as by rtx_render_region_device.  With rows = rtx_region_rows(region) and
 * P = rows * region->width, ray (k - first_sample) * P + i * width + (x - x0) belongs to pixel
 * (x, y0 + rtx_region_row(region, i)) and sample k: sample-major, so 64 consecutive rays are neighbouring pixels
 * of one sample.  Draws (event 0): block (0, 0) gives dx, dy and the first defocus-disk pair;
 * attempt a >= 1 of the disk uses words 0 and 1 of block (0, a).  The disk's rejection loop runs whether or not
 * defocus_angle > 0, as in the reference, so `draws` is the reference's count.  Every ray has tmin = 0.001f and
 * tmax = +inf (GetColor's interval, ray.go:36).  d_keys (may be NULL) receives (y * image_width + x, k, 1, draws):
 * event 1 is the key of the first scatter.  count == 0 or an empty shard returns RTX_OK and launches nothing.
 * first_sample + count past 2^32 - 1, a NULL cam, region or d_rays, and a pointer not aligned to 16 B return
 * RTX_ERR_INVALID_ARG.  More rays than one launch takes are cut into several launches. */
int rtx_camera_rays_device(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                           uint32_t count, rtx_ray* d_rays, rtx_path_key* d_keys, void* hip_stream);
/* The same into host memory, on the current device.  Blocking. */
int rtx_camera_rays(const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
                    uint32_t count, rtx_ray* rays, rtx_path_key* keys);

/* Emit and Scatter for n records in lock step, device memory of the CURRENT device on the given HIP stream:
 *  - d_rays[i] is the ray that was traced (Metal and Dielectric need Unit(r.dir));
 *  - d_hits[i] is its CLOSEST hit as rtx_trace* wrote it: point, normal, front_face, material, u and v are
 *    HitInfo's.  A scene with image textures must be traced with RTX_TRACE_UV (u and v are 0 without it).  Hits of
 *    RTX_TRACE_ANY are not valid input: only their prim is specified;
 *  - d_keys[i] names the Philox block: attempt a of the unit-sphere loop (vec3.go:182-190) is words 0-2 of
 *    (pixel, sample, event, a); the Dielectric's uniform (materials.go:103) is word 0 of (pixel, sample, event, 0),
 *    drawn only when refraction is possible;
 *  - seed is the render's seed.
 * d_hits[i].prim == RTX_HIT_NONE (a miss, or the all-zero bounce ray of an ended path traced again) gives an
 * all-zero bounce, and so does a material index outside the scene's table.  A Metal that absorbs (materials.go:70)
 * gives flags = 0, attenuation 0 and an all-zero ray; its rng_draws still counts the draws made.
 * Input and output buffers must not overlap.  n == 0 returns RTX_OK.  A NULL scene, a NULL pointer with n > 0, a
 * pointer not aligned to 16 B, flag bits other than RTX_SHADE_COUNTERS (all checked before any device is touched)
 * and a current device that holds no copy of the scene return RTX_ERR_INVALID_ARG.
 * Returns after enqueueing unless stats != NULL; then it synchronises the stream and fills stats.  A shade takes
 * the scene's mutex like a trace, uses none of the per-device sample scratch and keeps counters and events of its
 * own: a counting shade between two renders changes neither's stats.  n beyond what one launch indexes in 32 bits
 * is cut into several launches. */
int rtx_shade_device(rtx_scene* scene, uint64_t seed, const rtx_ray* d_rays, const rtx_hit* d_hits,
                     const rtx_path_key* d_keys, uint64_t n, rtx_bounce* d_out, uint32_t flags, void* hip_stream,
                     rtx_shade_stats* stats);
/* The same for records in host memory, on the current device.  Blocking. */
int rtx_shade(rtx_scene* scene, uint64_t seed, const rtx_ray* rays, const rtx_hit* hits, const rtx_path_key* keys,
              uint64_t n, rtx_bounce* out, uint32_t flags, rtx_shade_stats* stats);

/* ---- denoised previews (ABI 10, additive) -------------------------
 * The first resolved image of a progressive render is noise.  A preview is that image passed through a
 * variance-guided, edge-avoiding a-trous filter steered by first-hit guide images.  It is a SEPARATE output: no
 * render, no resolve and no image the oracle checks changes.
 *
 * Guide images.  One rtx_guide per pixel of the region's shard, row-major in the compacted shard rows
 * rtx_render_region_device writes (rtx_region): the mean, over samples k = first_sample .. first_sample + count - 1,
 * of the first hit of the render's own camera ray for (pixel, k): event 0 of DESIGN.md §3, the ray rtx_camera_rays
 * produces for that pixel and sample, lens included.  Per sample:
 *   a miss:  a = (1, 1, 1), n = 0, no depth;
 *   a hit:   n = HitInfo.normal (unit, flipped against the ray), t = HitInfo.t (the camera's rays end on the focus
 *            plane, so t is planar depth in units of the focus distance), and a = the Lambertian's texture value at
 *            (u, v, point) (all four texture kinds), the Metal's albedo, (1, 1, 1) for Dielectric and DiffuseLight.
 * The fold is float32 in k order, each operation rounded, no fused multiply-add:
 *   A = A + a;  N = N + n;  on a hit  Z = Z + t;  c = c + 1
 *   inv = 1.0f / (float)count;  albedo = A * inv;  normal = N * inv;  cover = (float)c * inv
 *   depth = c ? Z / (float)c : 0
 * So a guide equals rtx_camera_rays -> rtx_trace(RTX_TRACE_UV) -> rtx_shade folded this way, bit for bit on a scene
 * that keeps the caller's tree (on the library's own trees up to the grazing hits of DESIGN.md §12), without the
 * 32 + 48 + 64 B per sample those calls move through memory. */
typedef struct rtx_guide { /* 32 B */
    float albedo[3];
    float cover;    /* the share of the samples that hit something */
    float normal[3];
    float depth;    /* mean t of the samples that hit; 0 when none did */
} rtx_guide;
typedef struct rtx_guide_stats {
    uint64_t rays;    /* pixels * count */
    double kernel_ms; /* device time of the launch, HIP events on the stream */
} rtx_guide_stats;

/* Guides of the region's shard into device memory of the CURRENT device, on the given HIP stream.  Returns after
 * enqueueing unless stats != NULL; then it synchronises the stream and fills stats.  count == 0 (a mean over
 * nothing), first_sample + count past 2^32 - 1, a NULL scene, cam, region or d_guides, a d_guides not aligned to
 * 16 B (all checked before any device is touched) and a current device that holds no copy of the scene return
 * RTX_ERR_INVALID_ARG; the camera and the region are validated as by rtx_render_region_device.  An empty shard
 * returns RTX_OK and launches nothing.  The call takes the scene's mutex and walks the ray queries' layouts (hinted
 * with rtx_camera_octant(cam)); it uses none of the sample scratch and no render's counters, so a call between two
 * renders changes neither. */
int rtx_guides_device(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, const rtx_region* region,
                      uint32_t first_sample, uint32_t count, rtx_guide* d_guides, void* hip_stream,
                      rtx_guide_stats* stats);
/* The same into host memory, on the current device.  Blocking. */
int rtx_guides(rtx_scene* scene, const rtx_camera* cam, uint64_t seed, const rtx_region* region, uint32_t first_sample,
               uint32_t count, rtx_guide* guides, rtx_guide_stats* stats);

/* The filter.  d_rgb and d_var are the images rtx_accum_resolve_device writes (width x rows, 3 floats per pixel;
 * d_var the variance of the mean, required), d_guides the guides of the same pixels, d_out the filtered image
 * (3 floats per pixel).  Stateless: no scene, no lock, like rtx_encode_ppm_device.  The arithmetic is the contract:
 * float32, every operation rounded on its own, no fused multiply-add, no square root, no exp.
 *
 *   prepare, per pixel:   a_c = albedo_c > 0.01f ? albedo_c : 0.01f;   c_c = rgb_c / a_c
 *                         v = (var_r / (a_r * a_r) + var_g / (a_g * a_g)) + var_b / (a_b * a_b)
 *   level i = 0 .. iterations - 1, s = 1 << i, (c, v) -> (c', v'), n = guide.normal, z = guide.depth:
 *     vb = SV / SK, both sums starting at 0 over the taps p + (a, b) inside the image, b = -1..1 outer, a = -1..1
 *          inner:  k = k3[b + 1] * k3[a + 1], k3 = (1, 2, 1);  SV = SV + k * v;  SK = SK + k
 *     l_p = (c_r + c_g) + c_b;    dl = (sigma_luminance * sigma_luminance) * vb + 1e-6f
 *     W = C_c = V = 0;  for dy = -2..2, for dx = -2..2, q = p + s * (dx, dy), taps outside the image skipped:
 *         dn = n_p - n_q;  xn = ((dn_x * dn_x + dn_y * dn_y) + dn_z * dn_z) / (sigma_normal * sigma_normal)
 *         m = (float)(s * max(|dx|, |dy|));  zm = z_p > z_q ? z_p : z_q;  tz = (sigma_depth * m) * zm
 *         dz = z_p - z_q;  xz = (dz * dz) / (tz * tz + 1e-6f)
 *         d = l_p - l_q;   xl = (d * d) / dl
 *         w = (((k5[dy + 2] * k5[dx + 2]) * f(xn)) * f(xz)) * f(xl),  k5 = (1/16, 1/4, 3/8, 1/4, 1/16),
 *                                                                    f(x) = 1 - x > 0 ? 1 - x : 0
 *         if (w > 0) { W = W + w;  C_c = C_c + w * c_q;  V = V + (w * w) * v_q }
 *     c' = C / W;   v' = V / (W * W)
 *   finish:  out_c = c_c * a_c
 *
 * Sky next to sky has dn = 0 and dz = 0: weight k5 * k5; sky next to geometry has |dn|^2 = 1 > sigma_normal^2:
 * weight 0.  A NaN colour (resolve gives it variance 0) weighs 0 in every neighbour's sum and comes out NaN itself;
 * from the second level on its variance is NaN too, which the 3 x 3 variance sum hands to the pixels around it, so
 * after i levels the pixels within i - 1 of it are NaN.
 * sigma_depth is the relative depth slope tolerated per pixel of distance, so it scales with the resolution: a
 * surface seen at twice the pixel count changes half as much per pixel.
 * iterations is 1 to 6; sigma_normal > 0, sigma_depth >= 0, sigma_luminance >= 0.  Every pointer is aligned to
 * 16 B; d_work holds at least rtx_denoise_workspace_bytes(width, rows); d_out overlaps neither an input nor d_work,
 * and d_work no input.  A violation of any of these, or a NULL pointer, returns RTX_ERR_INVALID_ARG before any
 * device is touched.  width * rows == 0 returns RTX_OK and launches nothing.  Returns after enqueueing
 * iterations + 1 kernels on the stream. */
typedef struct rtx_denoise_params {
    uint32_t iterations;
    float sigma_normal;
    float sigma_depth;
    float sigma_luminance;
} rtx_denoise_params;
/* 5, 0.45f, 0.05f, 8.0f */
void rtx_denoise_defaults(rtx_denoise_params* params);
/* Two float4 images: 32 B per pixel. */
uint64_t rtx_denoise_workspace_bytes(uint32_t width, uint32_t rows);
int rtx_denoise_device(const float* d_rgb, const float* d_var, const rtx_guide* d_guides, uint32_t width, uint32_t rows,
                       const rtx_denoise_params* params, float* d_out, void* d_work, uint64_t work_bytes,
                       void* hip_stream);
/* The same for images in host memory (no alignment rule, no workspace), on the current device.  Blocking. */
int rtx_denoise(const float* rgb, const float* var, const rtx_guide* guides, uint32_t width, uint32_t rows,
                const rtx_denoise_params* params, float* out_rgb);

/* A preview of an accumulator after n >= 1 samples, into device memory d_out (the region's compacted shard rows,
 * 3 floats per pixel, aligned to 16 B) on hip_stream:  rtx_accum_resolve_device, rtx_guides_device over samples
 * [0, min(n, guide_samples)), rtx_denoise_device; its bytes are those of the three calls composed.  params NULL:
 * rtx_denoise_defaults.  guide_samples == 0 returns RTX_ERR_INVALID_ARG.  The resolved image, its variance, the
 * guides and the filter's workspace (88 B per pixel) belong to the accumulator: allocated by its first preview
 * (a blocking allocation), freed with it, not part of the per-device scratch and not counted by
 * rtx_device_scratch_bytes.  S, Q and n are not modified: more passes may follow.  Returns after enqueueing. */
int rtx_accum_preview_device(rtx_accum* accum, uint32_t guide_samples, const rtx_denoise_params* params, float* d_out,
                             void* hip_stream);
/* The same into host memory, after every render enqueued on the device so far.  Blocking. */
int rtx_accum_preview(rtx_accum* accum, uint32_t guide_samples, const rtx_denoise_params* params, float* out_rgb);
/* The preview encoded as rtx_accum_ppm encodes the resolved image.  Blocking. */
int rtx_accum_preview_ppm(rtx_accum* accum, uint32_t guide_samples, const rtx_denoise_params* params, char* out_text,
                          uint64_t capacity, uint64_t* out_len);

/* ---- direct light sampling (ABI 10, additive) ----------------------
 * Ray.GetColor finds a DiffuseLight only when a bounce happens to hit it (ray.go:41-47).  Next-event estimation
 * samples a point on an emitter at a diffuse hit and casts a shadow ray to it.  This section gives the emitter table
 * and the BLOCK that does both for a batch of hits; it composes with rtx_trace* and rtx_shade* (wavefront.py's
 * render(direct=True) is the estimator).  Every render, pass and image of the other sections is what it was.
 *
 * The emitter table.  The emitters are the spheres and quads the world references (roots, nodes, lists) whose
 * material is RTX_MAT_DIFFUSE_LIGHT: spheres in sphere-table order, then quads in quad-table order, each once.  A
 * primitive the tree never references is not an emitter; nor is a sphere with radius <= 0, nor an emitter whose area
 * is not finite and > 0.  Areas are float32:
 *   sphere:  area = (4 * PiF32) * (r * r)          (PiF32 = float32(math.Pi), math.go:48)
 *   quad:    area = Len(Cross(u, v))               (vec3.go:119-135; the square root goes through float64, as Len's)
 * L is the count; a scene with L > 2^24 is refused (RTX_ERR_INVALID_ARG): (float)L must be exact.  The table is built
 * on the host and uploaded by the first call that needs it, as the trace layout is. */
typedef struct rtx_light { /* 8 B */
    uint32_t prim; /* type << 28 | index into the CALLER's sphere / quad table, as rtx_hit.prim */
    float area;
} rtx_light;
/* The table of a scene description (validated as rtx_scene_create does), without a scene or a device, or of a scene:
 * *n = L; out is filled when cap >= L (out may be NULL to ask for the count).  Host only. */
int rtx_lights(const rtx_scene_desc* desc, rtx_light* out, uint32_t cap, uint32_t* n);
int rtx_scene_lights(const rtx_scene* scene, rtx_light* out, uint32_t cap, uint32_t* n);

/* The block.  Record i takes d_hits[i], the CLOSEST hit rtx_trace* wrote with RTX_TRACE_UV, the rtx_path_key of the
 * scatter at that hit (d_keys[i]) and the render's seed, and gives one light sample and its shadow ray's answer.
 * One kernel does both halves: the sample by the render's own device functions (the four textures, the sphere UV,
 * the unit-sphere loop), the shadow walk over the ray queries' layouts.  The arithmetic is the contract: float32,
 * every operation rounded on its own, no fused multiply-add; Dot, Len, Cross as vec3.go states them.
 *
 *   only when hit.prim != RTX_HIT_NONE, hit.material indexes a Lambertian and L > 0; otherwise the record is all zero
 *   p = hit.point   n = hit.normal   a = the Lambertian's texture at (hit.u, hit.v, p)
 *   B0 = Philox block (pixel, sample, 0x40000000 | event, 0)     (the light events of DESIGN.md §3; unit(w) =
 *                                                                 (float)(w >> 8) * 2^-24, rand.Float32's)
 *   j  = min((uint32)(unit(B0.x) * (float)L), L - 1)
 *   quad j:    x1 = unit(B0.y), x2 = unit(B0.z);  q = (Q + x1 * u) + x2 * v;  nl = the quad's normal;  (lu, lv) = (x1, x2)
 *   sphere j:  d = the loop of vec3.go:182-190, attempt a = 1, 2, .. taking words 0-2 of block (.., 0x40000000 | event, a)
 *              q = c + r * d;  nl = d;  (lu, lv) = the sphere UV of d (hittables.go:122-126)
 *   w = q - p;  d2 = Dot(w, w);  dist = Len(w);  cs = Dot(n, w) / dist;  cl = |Dot(nl, w)| / dist
 *   SAMPLED = d2 > 0 && cs > 0 && cl > 0           (a NaN fails; DiffuseLight.Emit ignores the face: both sides emit)
 *   g  = (((cs * cl) * area_j) * (float)L) / (PiF32 * d2)
 *   Le = the emitter's texture at (lu, lv, q), all four texture kinds
 *   radiance_c = (a_c * Le_c) * g
 *   ray = { origin p, tmin 0.001f, dir w, tmax 0.999f }
 *   VISIBLE = SAMPLED && no primitive accepted on ray   (exactly rtx_trace(ray, RTX_TRACE_ANY).prim == RTX_HIT_NONE)
 *
 * g is the Lambertian BRDF (a / pi) times the geometry term cs * cl / d2 over the density 1 / (L * area_j) of the
 * point q.  radiance does NOT include the visibility: the caller adds it when RTX_DIRECT_VISIBLE is set.  A record
 * that is not SAMPLED has `light` and `rng_draws` filled and every other field zero.
 * The sphere case samples its whole area uniformly: half of the points face away from p, and the shadow ray then
 * finds the sphere's own near side (tmax 0.999 ends before q, tmin 0.001 starts past p).  That is unbiased and
 * wasteful.  Not provided: cone sampling of spheres, power-proportional light selection.  (Multiple importance
 * sampling with the bounce: the section after this one.)
 * Argument checks (before any device is touched), alignment, n == 0, the scene's mutex, the 32-bit launch cut, the
 * counters and events of its own and the untouched sample scratch are rtx_shade_device's.  Input and output buffers
 * must not overlap. */
typedef struct rtx_direct_sample { /* 64 B */
    float radiance[3];  /* (a * Le) * g, visibility NOT applied; 0 when not SAMPLED                  */
    uint32_t flags;     /* RTX_DIRECT_SAMPLED | RTX_DIRECT_VISIBLE                                   */
    rtx_ray ray;        /* the shadow ray; all zero when not SAMPLED                                  */
    uint32_t light;     /* j, the index into the emitter table                                        */
    uint32_t rng_draws; /* rand.Float32() calls: 1 + 2 for a quad, 1 + 3 per attempt for a sphere      */
    float geom;         /* g                                                                          */
    uint32_t reserved;  /* 0                                                                          */
} rtx_direct_sample;
#define RTX_DIRECT_SAMPLED 1u
#define RTX_DIRECT_VISIBLE 2u
#define RTX_DIRECT_COUNTERS 1u /* counting instantiation: sampled, visible, rng_draws (with stats only) */
typedef struct rtx_direct_stats {
    uint64_t n;         /* records                                                    */
    uint64_t sampled;   /* RTX_DIRECT_COUNTERS: records with RTX_DIRECT_SAMPLED       */
    uint64_t visible;   /* RTX_DIRECT_COUNTERS: records with RTX_DIRECT_VISIBLE       */
    uint64_t rng_draws; /* RTX_DIRECT_COUNTERS: the sum of rtx_direct_sample.rng_draws       */
    double kernel_ms;   /* device time of the launches, HIP events on the stream      */
} rtx_direct_stats;

/* Records in device memory of the CURRENT device, on the given HIP stream.  Returns after enqueueing unless
 * stats != NULL; then it synchronises the stream and fills stats.  The emitter table and the trace layout are
 * uploaded by the first call that needs them (blocking copies). */
int rtx_direct_device(rtx_scene* scene, uint64_t seed, const rtx_hit* d_hits, const rtx_path_key* d_keys, uint64_t n,
                      rtx_direct_sample* d_out, uint32_t flags, void* hip_stream, rtx_direct_stats* stats);
/* The same for records in host memory, on the current device.  Blocking. */
int rtx_direct(rtx_scene* scene, uint64_t seed, const rtx_hit* hits, const rtx_path_key* keys, uint64_t n,
               rtx_direct_sample* out, uint32_t flags, rtx_direct_stats* stats);

/* The estimator and the fused pass.  Ray.GetColor (ray.go:32-54) with one change: radiance a Lambertian bounce would
 * have found by hitting an emitter is taken from the block instead.  Per sample L = 0, T = 1, diffuse = false; for
 * segment s = 0 .. max_depth - 1, in this order, every * and + rounded on its own:
 *
 *   miss:  L += T * background; end
 *   hit:   if EMITS and !diffuse:                       L += T * emitted
 *          lam = SCATTERED and the material is Lambertian
 *          if lam and s + 1 < max_depth and L_lights > 0:
 *              d = direct(hit, key(event s + 1));  if d.VISIBLE:  L += T * d.radiance
 *          if !SCATTERED: end
 *          T *= attenuation;  diffuse = lam and L_lights > 0;  continue with the bounce ray
 *
 * s + 1 < max_depth keeps the set of path lengths the reference's depth cap allows, so the expectation is the plain
 * render's; with no emitter nothing is added and nothing suppressed, and the pass computes the plain render, bit for
 * bit.  CAVEAT of the rule: `diffuse` also drops the emission of a DiffuseLight primitive the emitter table excludes
 * (zero area, radius <= 0) when the scene has other emitters: biased for such a primitive, which the reference renders.
 *
 * rtx_accum_add_direct renders samples n .. n + count - 1 of every pixel this way in one kernel (no ray, hit, bounce
 * or path state goes through memory) and folds S += c; Q += c * c in k order, as rtx_accum_add does; its image equals
 * rtx_camera_rays -> (rtx_trace(RTX_TRACE_UV) -> rtx_shade -> rtx_direct) x max_depth composed as above, bit for bit on
 * a scene that keeps the caller's tree (on the library's own trees up to the grazing hits of DESIGN.md §12).
 * An accumulator is plain, adaptive or direct from its first pass until rtx_accum_reset: rtx_accum_add or
 * rtx_accum_add_adaptive after a direct pass, and rtx_accum_add_direct after either of them, return
 * RTX_ERR_INVALID_ARG, as do a NULL accumulator, count == 0, n + count past 2^32 - 1 and flags != 0, all before any
 * device is touched.  Returns after enqueueing unless stats != NULL; then it synchronises and fills samples,
 * sample_chunks, kernel_ms and walk_layout of this pass.  Resolve, ppm, preview and sample_counts read a direct
 * accumulator as they read a plain one.  The pass uses none of the sample scratch.
 * Tuning knobs, read from the environment per call, none of which changes a bit of any output: RTX_DIRECT_RANGE
 * (records per wave of the block, 256), RTX_DIRECT_REFILL (parked lanes at which a wave of the pass runs its fold step,
 * 32), RTX_DIRECT_PRIM_BATCH (lanes a primitive test waits for, 16), RTX_DIRECT_LAUNCH_RECORDS (records per launch of
 * the block: tests of the cut). */
int rtx_accum_add_direct(rtx_accum* accum, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats);

/* ---- multiple importance sampling of the direct light (ABI 10, additive) ----------------------
 * The estimator above takes an emitter's radiance after a Lambertian hit from the light sample alone, and a light
 * sample's g has no bound (a light close to a surface: 1 / d2).  This section weights the two strategies that reach
 * an emitter point q from a Lambertian hit p, the light sample and the bounce, by the power heuristic (beta = 2).
 * Nothing of the sections above changes: rtx_direct*, rtx_accum_add_direct and their images are what they were.
 *
 * Weighting.  Both densities on the area measure at q: the light sample's is 1 / (L * A_j); the bounce's, whose
 * direction normal + unit is cosine-distributed, is cs * cl / (PiF32 * d2).  Their ratio, bounce over light, is exactly
 * the block's g, so the heuristic needs nothing else:
 *   light sample:                 wl = 1 / (1 + g * g)        g = rtx_direct_sample.geom
 *   bounce that finds an emitter: wb = 1 - 1 / (1 + g * g)    g evaluated at the point the bounce hit
 * float32, every operation rounded on its own, no fused multiply-add; a g * g of +inf gives wb = 1 exactly.  The
 * bounce's g, for a bounce that left the Lambertian hit `from` and found `hit` on a DiffuseLight primitive:
 *   A    = the emitter table's area of hit.prim, 0 if the table excludes it     L = the table's count
 *   w    = hit.point - from.point;  d2 = Dot(w, w);  dist = Len(w)
 *   cs   = Dot(from.normal, w) / dist;  cl = |Dot(hit.normal, w)| / dist
 *   g    = (((cs * cl) * A) * (float)L) / (PiF32 * d2)
 * A == 0, d2 == 0 or a NaN g give wb = 1 (and a record's geom = 0): the reference's emission is kept whole.  So an
 * emitter the table excludes (radius <= 0, zero area) is NOT dropped, which removes the CAVEAT above for this mode.
 * wl + wb = 1 wherever both strategies can produce q; a light sample adds at most a * Le / 2 (g / (1 + g * g) <= 1/2),
 * a weighted bounce at most a * Le.  No random number is drawn and no new Philox event range is used.
 *
 * The per-primitive lookup the weight reads: entry k < n_spheres is the caller's sphere k, entry n_spheres + k the
 * caller's quad k; area and light are the emitter table's (bit-equal), 0 and RTX_LIGHT_NONE for every primitive that
 * is not in it.  Host only, validated as rtx_lights; *n = n_spheres + n_quads, out filled when cap >= *n. */
typedef struct rtx_prim_light { /* 8 B */
    float area;
    uint32_t light; /* index into the emitter table, or RTX_LIGHT_NONE */
} rtx_prim_light;
#define RTX_LIGHT_NONE 0xFFFFFFFFu
int rtx_prim_lights(const rtx_scene_desc* desc, rtx_prim_light* out, uint32_t cap, uint32_t* n_spheres, uint32_t* n);

/* The block.  Record i takes d_from[i], the hit a bounce left, and d_hits[i], the closest hit that bounce found
 * (both as rtx_trace* wrote them), and gives the bounce's weight.  A record is NOT WEIGHTED (weight = 1, geom = 0,
 * light = RTX_LIGHT_NONE, flags = 0) when hit is a miss, hit.material is outside the table or no DiffuseLight,
 * from is a miss, or from.material is outside the table or not Lambertian.  Otherwise light is hit.prim's table index
 * (RTX_LIGHT_NONE when the table excludes it, or hit.prim names no primitive of the scene) and, when A > 0, d2 > 0
 * and g is no NaN, RTX_EMITTER_WEIGHTED is set, geom = g and weight = wb; else weight = 1, geom = 0.
 * Argument checks, alignment, n == 0, the scene's mutex, the launch cut, counters and events are rtx_direct_device's
 * (RTX_EMITTER_LAUNCH_RECORDS: records per launch, tests of the cut).  No walk, no texture, no random number. */
typedef struct rtx_emitter_weight_record { /* 16 B */
    float weight;   /* wb */
    float geom;     /* g; 0 when not WEIGHTED */
    uint32_t light; /* table index of hit.prim, or RTX_LIGHT_NONE */
    uint32_t flags; /* RTX_EMITTER_WEIGHTED */
} rtx_emitter_weight_record;
#define RTX_EMITTER_WEIGHTED 1u
#define RTX_EMITTER_COUNTERS 1u /* counting instantiation: weighted (with stats only) */
typedef struct rtx_emitter_stats {
    uint64_t n;        /* records                                                 */
    uint64_t weighted; /* RTX_EMITTER_COUNTERS: records with RTX_EMITTER_WEIGHTED */
    double kernel_ms;  /* device time of the launches, HIP events on the stream   */
} rtx_emitter_stats;
int rtx_emitter_weight_device(rtx_scene* scene, const rtx_hit* d_from, const rtx_hit* d_hits, uint64_t n,
                              rtx_emitter_weight_record* d_out, uint32_t flags, void* hip_stream,
                              rtx_emitter_stats* stats);
/* The same for records in host memory, on the current device.  Blocking. */
int rtx_emitter_weight(rtx_scene* scene, const rtx_hit* from, const rtx_hit* hits, uint64_t n,
                       rtx_emitter_weight_record* out, uint32_t flags, rtx_emitter_stats* stats);

/* The estimator and the fused pass: the rule of rtx_accum_add_direct with two lines changed (`diffuse` as there):
 *
 *   hit:   if EMITS:  L += T * (diffuse ? emitted * wb : emitted)        wb of (the previous hit, this hit)
 *          ...        if d.VISIBLE:  L += T * (d.radiance * wl)          wl of d.geom
 *
 * The sample-taking condition and so the set of path lengths are unchanged; wb applies whenever diffuse is set,
 * whether or not the light sample at the previous hit was SAMPLED.  With no emitter, or at max_depth 1, the result is
 * the plain render bit for bit.  Unbiased: at every emitter point visible from p the two weights sum to 1, and where
 * one strategy cannot produce q (a sphere's far side, cs <= 0) neither adds anything.
 * rtx_accum_add_mis is rtx_accum_add_direct for this estimator, one kernel, equal bit for bit to the composition
 * rtx_trace -> rtx_shade -> rtx_emitter_weight -> rtx_direct (wavefront.py's render(direct=True, mis=True)) as stated
 * there.  An accumulator has a fourth mode: rtx_accum_add_mis after a plain, adaptive or direct pass, and any of those
 * after it, return RTX_ERR_INVALID_ARG until rtx_accum_reset, as do a NULL accumulator, count == 0, n + count past
 * 2^32 - 1 and flags != 0, all before any device is touched.  Stats, readers and knobs are rtx_accum_add_direct's. */
int rtx_accum_add_mis(rtx_accum* accum, uint32_t count, void* hip_stream, uint32_t flags, rtx_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* RTX_H */
