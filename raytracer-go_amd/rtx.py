"""ctypes binding of librtx.so (include/rtx.h) and librtxhost.so (include/rtx_host.h).

This is plumbing for the Python test driver and bench.py — the drop-in boundary
itself is the C-ABI (a Go host binds it via cgo).  Loading fails
loudly if the native libraries are missing: there is no CPU fallback for the product
path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_uint32, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))

RTX_OK = 0
RTX_ERR_INVALID_ARG = -1
RTX_ERR_HIP = -2
RTX_ERR_RCCL = -3
RTX_ERR_UNSUPPORTED = -4
RTX_ERR_NO_DEVICE = -5
RTX_ERR_OOM = -6

RTX_PRIM_SPHERE = 0
RTX_PRIM_QUAD = 1
RTX_PRIM_LIST = 2  # a World nested in the tree (ABI 5)
RTX_MAT_LAMBERTIAN, RTX_MAT_METAL, RTX_MAT_DIELECTRIC, RTX_MAT_DIFFUSE_LIGHT = 0, 1, 2, 3
RTX_TEX_SOLID, RTX_TEX_CHECKERED, RTX_TEX_IMAGE, RTX_TEX_NOISE = 0, 1, 2, 3
RTX_FLAG_COUNTERS = 1
RTX_FLAG_NO_LDS = 4
RTX_FLAG_TIMING = 1 << 20  # diagnostics: timed kernel + wave-cycle split
RTX_SCENE_REFERENCE_BVH = 1  # rtx_scene_create_ex: keep the caller's tree and the reference's visit order
RTX_SCENE_EVERY_BOX = 2  # rtx_scene_create_ex: the walk leaves no box test out (ABI 7, rtx_collapse.h)
RTX_SCENE_NO_TIER = 4  # rtx_scene_create_ex: no tiered walk (ABI 8)
RTX_LAYOUT_REFERENCE = 8  # Stats.walk_layout of a scene walking the caller's tree
RTX_LAYOUT_TIERED = 16  # Stats.walk_layout bit: the render walked in two tiers (ABI 8)
RTX_TREE_NEAR = 0x100  # rtx_scene_topology / rtx_walk_tree octant bit: the near tree (ABI 8)
RTX_GATHER_NONE, RTX_GATHER_RCCL, RTX_GATHER_DEVICE, RTX_GATHER_HOST = 0, 1, 2, 3  # Stats.gather_kind
RTX_SCENE_IN_HBM, RTX_SCENE_IN_LDS, RTX_SCENE_LDS_CACHE = 0, 1, 2  # Stats.scene_placement
RTX_IMAGE_TEXEL_WORDS = 2  # RGBA16 image texels: two uint32 words each (rtx.h)
# ray queries (rtx_trace*, ABI 10 additive)
RTX_HIT_NONE = 0xFFFFFFFF  # Hit.prim of a miss
RTX_TRACE_ANY = 1  # stop at the first accepted primitive: only prim != RTX_HIT_NONE is specified
RTX_TRACE_UV = 2  # fill u, v
RTX_TRACE_COUNTERS = 4  # the counting instantiation (with stats)
# path building blocks (rtx_camera_rays*, rtx_shade*, ABI 10 additive)
RTX_BOUNCE_SCATTERED = 1  # Bounce.flags: Scatter returned true; attenuation and ray are ScatterInfo's
RTX_BOUNCE_EMITS = 2  # Bounce.flags: the material is a DiffuseLight; emitted is its texture
RTX_SHADE_COUNTERS = 1  # the counting instantiation (with stats)
RTX_DIRECT_SAMPLED = 1  # DirectSample.flags: a light point was sampled; radiance, ray and geom are its
RTX_DIRECT_VISIBLE = 2  # DirectSample.flags: the shadow ray met no primitive
RTX_LIGHT_NONE = 0xFFFFFFFF  # PrimLight.light / EmitterWeight.light: not in the emitter table
RTX_EMITTER_WEIGHTED = 1  # EmitterWeight.flags: the power heuristic's weight (else weight = 1, geom = 0)
RTX_EMITTER_COUNTERS = 1  # rtx_emitter_weight* flag: count the weighted records (with stats)
RTX_DIRECT_COUNTERS = 1  # the counting instantiation (with stats)


def RTX_TRACE_OCTANT(o: int) -> int:
    """Hint: the direction signs (camera_octant's bits) the walked tree's child order should suit."""
    return (o & 7) << 8


def RTX_FLAG_SHADE_THRESH(n: int) -> int:
    return (n & 0x7F) << 8


def ref_prim(ptype: int, index: int) -> int:
    """RTX_REF_PRIM: ~((type << 28) | index) as int32."""
    v = ((ptype << 28) | (index & 0x0FFFFFFF)) & 0xFFFFFFFF
    return ~v if v < 0x80000000 else ~(v - (1 << 32))


class BvhNode(ctypes.Structure):
    _fields_ = [("bmin", c_float * 3), ("left", c_int32), ("bmax", c_float * 3), ("right", c_int32)]


class Sphere(ctypes.Structure):
    _fields_ = [("center", c_float * 3), ("radius", c_float), ("material", c_uint32), ("pad", c_uint32 * 3)]


class Quad(ctypes.Structure):
    _fields_ = [("q", c_float * 3), ("material", c_uint32), ("u", c_float * 3), ("d", c_float),
                ("v", c_float * 3), ("pad0", c_float), ("w", c_float * 3), ("pad1", c_float),
                ("normal", c_float * 3), ("pad2", c_float)]


class Material(ctypes.Structure):
    _fields_ = [("type", c_uint32), ("texture", c_uint32), ("fuzz", c_float), ("ior", c_float),
                ("albedo", c_float * 3), ("pad", c_float)]


class Texture(ctypes.Structure):
    _fields_ = [("type", c_uint32), ("scale", c_float), ("width", c_uint32), ("height", c_uint32),
                ("even", c_float * 3), ("texel_offset", c_uint32), ("odd", c_float * 3), ("pad", c_float)]


class List(ctypes.Structure):  # rtx_list (ABI 5): a World nested in the tree
    _fields_ = [("first", c_uint32), ("count", c_uint32)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("nodes", POINTER(BvhNode)), ("n_nodes", c_uint32), ("n_roots", c_uint32),
                ("roots", POINTER(c_int32)), ("spheres", POINTER(Sphere)), ("n_spheres", c_uint32),
                ("n_quads", c_uint32), ("quads", POINTER(Quad)), ("materials", POINTER(Material)),
                ("n_materials", c_uint32), ("n_textures", c_uint32), ("textures", POINTER(Texture)),
                ("texels", POINTER(c_uint32)), ("n_texels", c_uint64),
                ("lists", POINTER(List)), ("n_lists", c_uint32), ("n_list_refs", c_uint32),
                ("list_refs", POINTER(c_int32))]


class Camera(ctypes.Structure):
    _fields_ = [("image_width", c_uint32), ("image_height", c_uint32), ("samples_per_pixel", c_uint32),
                ("max_depth", c_uint32), ("center", c_float * 3), ("defocus_angle", c_float),
                ("pixel00", c_float * 3), ("pad0", c_float), ("pixel_du", c_float * 3), ("pad1", c_float),
                ("pixel_dv", c_float * 3), ("pad2", c_float), ("defocus_disk_u", c_float * 3), ("pad3", c_float),
                ("defocus_disk_v", c_float * 3), ("pad4", c_float), ("background", c_float * 3), ("pad5", c_float)]


class Region(ctypes.Structure):
    """rtx_region: columns [x0, x0 + width), the rows of [y0, y0 + height) in stripes of `stripe` rows (0 / 1:
    single rows) dealt round-robin: this shard takes stripes rank, rank + world, ... (ABI 9: stripe)."""
    _fields_ = [("x0", c_uint32), ("y0", c_uint32), ("width", c_uint32), ("height", c_uint32),
                ("rank", c_uint32), ("world", c_uint32), ("stripe", c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("samples", c_uint64), ("segments", c_uint64), ("node_visits", c_uint64),
                ("prim_tests", c_uint64), ("hits", c_uint64), ("texel_fetches", c_uint64),
                ("rng_draws", c_uint64), ("kernel_ms", c_double), ("gather_ms", c_double),
                ("wave_iters", c_uint64), ("lane_steps", c_uint64), ("shade_phases", c_uint64),
                ("shade_lanes", c_uint64), ("trav_cycles", c_uint64), ("shade_cycles", c_uint64),
                ("idle_lanes", c_uint64), ("cache_hits", c_uint64), ("sample_chunks", c_uint64),
                ("parked_lanes", c_uint64), ("deferred_lanes", c_uint64), ("shade_split_cycles", c_uint64 * 4),
                ("walk_layout", c_uint64), ("gather_kind", c_uint64), ("scene_placement", c_uint64),
                ("deferred_paths", c_uint64), ("redo_chunks", c_uint64)]

    def as_dict(self) -> dict:
        return {name: (list(v) if not isinstance(v := getattr(self, name), (int, float)) else v)
                for name, _ in self._fields_}


class TraceRay(ctypes.Structure):  # rtx_ray, 32 B
    _fields_ = [("origin", c_float * 3), ("tmin", c_float), ("dir", c_float * 3), ("tmax", c_float)]


class TraceHit(ctypes.Structure):  # rtx_hit, 48 B
    _fields_ = [("t", c_float), ("prim", c_uint32), ("material", c_uint32), ("front_face", c_uint32),
                ("point", c_float * 3), ("u", c_float), ("normal", c_float * 3), ("v", c_float)]


class TraceStats(ctypes.Structure):  # rtx_trace_stats
    _fields_ = [("rays", c_uint64), ("hits", c_uint64), ("node_visits", c_uint64), ("prim_tests", c_uint64),
                ("walk_layout", c_uint64), ("scene_placement", c_uint64), ("kernel_ms", c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PathKey(ctypes.Structure):  # rtx_path_key, 16 B
    _fields_ = [("pixel", c_uint32), ("sample", c_uint32), ("event", c_uint32), ("draws", c_uint32)]


class Bounce(ctypes.Structure):  # rtx_bounce, 64 B
    _fields_ = [("attenuation", c_float * 3), ("flags", c_uint32), ("emitted", c_float * 3), ("rng_draws", c_uint32),
                ("ray", TraceRay)]


class ShadeStats(ctypes.Structure):  # rtx_shade_stats
    _fields_ = [("n", c_uint64), ("hits", c_uint64), ("scattered", c_uint64), ("rng_draws", c_uint64),
                ("texel_fetches", c_uint64), ("kernel_ms", c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class Light(ctypes.Structure):  # rtx_light, 8 B
    _fields_ = [("prim", c_uint32), ("area", c_float)]


class DirectSample(ctypes.Structure):  # rtx_direct_sample, 64 B
    _fields_ = [("radiance", c_float * 3), ("flags", c_uint32), ("ray", TraceRay), ("light", c_uint32),
                ("rng_draws", c_uint32), ("geom", c_float), ("reserved", c_uint32)]


class DirectStats(ctypes.Structure):  # rtx_direct_stats
    _fields_ = [("n", c_uint64), ("sampled", c_uint64), ("visible", c_uint64), ("rng_draws", c_uint64),
                ("kernel_ms", c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PrimLight(ctypes.Structure):  # rtx_prim_light, 8 B
    _fields_ = [("area", c_float), ("light", c_uint32)]


class EmitterWeight(ctypes.Structure):  # rtx_emitter_weight_record, 16 B
    _fields_ = [("weight", c_float), ("geom", c_float), ("light", c_uint32), ("flags", c_uint32)]


class EmitterStats(ctypes.Structure):  # rtx_emitter_stats
    _fields_ = [("n", c_uint64), ("weighted", c_uint64), ("kernel_ms", c_double)]


class Guide(ctypes.Structure):  # rtx_guide, 32 B
    _fields_ = [("albedo", c_float * 3), ("cover", c_float), ("normal", c_float * 3), ("depth", c_float)]


class GuideStats(ctypes.Structure):  # rtx_guide_stats
    _fields_ = [("rays", c_uint64), ("kernel_ms", c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class AdaptStats(ctypes.Structure):  # rtx_adapt_stats
    _fields_ = [("tiles", c_uint64), ("open_tiles", c_uint64), ("open_pixels", c_uint64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class DenoiseParams(ctypes.Structure):  # rtx_denoise_params; DenoiseParams.defaults() = rtx_denoise_defaults
    _fields_ = [("iterations", c_uint32), ("sigma_normal", c_float), ("sigma_depth", c_float),
                ("sigma_luminance", c_float)]

    @classmethod
    def defaults(cls) -> "DenoiseParams":
        p = cls()
        load().rtx_denoise_defaults(ctypes.byref(p))
        return p


def __getattr__(name: str):
    """RAY_DTYPE / HIT_DTYPE / KEY_DTYPE / BOUNCE_DTYPE / GUIDE_DTYPE / LIGHT_DTYPE / DIRECT_DTYPE / PRIM_LIGHT_DTYPE /
    EMITTER_WEIGHT_DTYPE: the numpy structured dtypes of rtx_ray, rtx_hit, rtx_path_key, rtx_bounce, rtx_guide, rtx_light,
    rtx_direct_sample, rtx_prim_light and rtx_emitter_weight_record (numpy is imported on first use, as everywhere in
    this module)."""
    if name in ("PRIM_LIGHT_DTYPE", "EMITTER_WEIGHT_DTYPE"):
        import numpy as np
        globals().update(PRIM_LIGHT_DTYPE=np.dtype([("area", "<f4"), ("light", "<u4")]),
                         EMITTER_WEIGHT_DTYPE=np.dtype([("weight", "<f4"), ("geom", "<f4"), ("light", "<u4"),
                                                        ("flags", "<u4")]))
        return globals()[name]
    if name == "GUIDE_DTYPE":
        import numpy as np
        globals().update(GUIDE_DTYPE=np.dtype([("albedo", "<f4", (3,)), ("cover", "<f4"), ("normal", "<f4", (3,)),
                                               ("depth", "<f4")]))
        return globals()[name]
    if name in ("LIGHT_DTYPE", "DIRECT_DTYPE"):
        import numpy as np
        ray = __getattr__("RAY_DTYPE")
        globals().update(LIGHT_DTYPE=np.dtype([("prim", "<u4"), ("area", "<f4")]),
                         DIRECT_DTYPE=np.dtype([("radiance", "<f4", (3,)), ("flags", "<u4"), ("ray", ray), ("light", "<u4"),
                                                ("rng_draws", "<u4"), ("geom", "<f4"), ("reserved", "<u4")]))
        return globals()[name]
    if name in ("RAY_DTYPE", "HIT_DTYPE", "KEY_DTYPE", "BOUNCE_DTYPE"):
        import numpy as np
        ray = np.dtype([("origin", "<f4", (3,)), ("tmin", "<f4"), ("dir", "<f4", (3,)), ("tmax", "<f4")])
        hit = np.dtype([("t", "<f4"), ("prim", "<u4"), ("material", "<u4"), ("front_face", "<u4"),
                        ("point", "<f4", (3,)), ("u", "<f4"), ("normal", "<f4", (3,)), ("v", "<f4")])
        key = np.dtype([("pixel", "<u4"), ("sample", "<u4"), ("event", "<u4"), ("draws", "<u4")])
        bounce = np.dtype([("attenuation", "<f4", (3,)), ("flags", "<u4"), ("emitted", "<f4", (3,)),
                           ("rng_draws", "<u4"), ("ray", ray)])
        globals().update(RAY_DTYPE=ray, HIT_DTYPE=hit, KEY_DTYPE=key, BOUNCE_DTYPE=bounce)
        return globals()[name]
    raise AttributeError(f"module 'rtx' has no attribute {name!r}")


RTX_SYMBOLS = [
    "rtx_version", "rtx_build_info", "rtx_last_error", "rtx_device_count", "rtx_scene_create",
    "rtx_scene_destroy", "rtx_scene_device_bytes", "rtx_render", "rtx_render_region_device", "rtx_region_rows",
    "rtx_ppm_max_bytes", "rtx_encode_ppm_device", "rtx_render_ppm", "rtx_scene_create_spheres", "rtx_scene_export",
    "rtx_release_device_memory", "rtx_device_scratch_bytes", "rtx_scene_create_ex", "rtx_scene_topology",
    "rtx_camera_octant", "rtx_walk_tree", "rtx_render_ex", "rtx_scene_walk_skip", "rtx_walk_skip",
    "rtx_scene_near_region", "rtx_scene_near_skip", "rtx_walk_near_region", "rtx_render_ppm_ex", "rtx_region_row",
    "rtx_device_check",
    # progressive rendering (ABI 10, additive)
    "rtx_accum_create", "rtx_accum_add", "rtx_accum_samples", "rtx_accum_resolve_device", "rtx_accum_resolve",
    "rtx_accum_ppm", "rtx_accum_reset", "rtx_accum_destroy",
    # ray queries (ABI 10, additive)
    "rtx_trace_device", "rtx_trace",
    # path building blocks (ABI 10, additive)
    "rtx_camera_rays_device", "rtx_camera_rays", "rtx_shade_device", "rtx_shade",
    # denoised previews (ABI 10, additive)
    "rtx_guides_device", "rtx_guides", "rtx_denoise_defaults", "rtx_denoise_workspace_bytes", "rtx_denoise_device",
    "rtx_denoise", "rtx_accum_preview_device", "rtx_accum_preview", "rtx_accum_preview_ppm",
    # adaptive sampling (ABI 10, additive)
    "rtx_accum_add_adaptive", "rtx_accum_tile_shape", "rtx_accum_sample_counts_device", "rtx_accum_sample_counts",
    # direct light sampling (ABI 10, additive)
    "rtx_lights", "rtx_scene_lights", "rtx_direct_device", "rtx_direct", "rtx_accum_add_direct",
    # multiple importance sampling of the direct light (ABI 10, additive)
    "rtx_prim_lights", "rtx_emitter_weight_device", "rtx_emitter_weight", "rtx_accum_add_mis",
    # GPU BVH build for a World of spheres and quads, and the quad constructors (ABI 10, additive)
    "rtx_scene_create_world", "rtx_quad_init", "rtx_box_quads",
]
RTXHOST_SYMBOLS = [
    "rtxhost_build_scene", "rtxhost_scene_free", "rtxhost_scene_desc", "rtxhost_scene_camera",
    "rtxhost_render_ppm", "rtxhost_ppm_encode", "rtxhost_last_error", "rtxhost_scene_world_spheres",
    "rtxhost_synthetic_earth_ycbcr", "rtxhost_ycbcr_rgba", "rtxhost_scene_world",
]

_lib = None
_host = None


def lib_path(name: str) -> str:
    return os.path.join(HERE, name)


def load() -> ctypes.CDLL:
    """Load librtx.so (raises OSError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RTX_LIB") or lib_path("librtx.so")  # RTX_LIB: A/B against another build
    if not os.path.exists(path):
        raise OSError(f"librtx.so not built at {path}: run __graft_entry__.build() (no CPU fallback exists)")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 (the SONAME of
    # /opt/rocm's), and whichever loads first serves both.  With librtx first, torch then bound to
    # the system runtime and reported no GPU (torch.cuda.is_available() False); torch first works.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    L.rtx_version.restype = c_int
    L.rtx_build_info.restype = c_char_p
    L.rtx_last_error.restype = c_char_p
    L.rtx_device_count.restype = c_int
    L.rtx_scene_create.argtypes = [POINTER(SceneDesc), POINTER(c_void_p)]
    L.rtx_scene_create.restype = c_int
    L.rtx_scene_create_ex.argtypes = [POINTER(SceneDesc), c_uint32, POINTER(c_void_p)]
    L.rtx_scene_create_ex.restype = c_int
    L.rtx_scene_topology.argtypes = [c_void_p, c_uint32, POINTER(BvhNode), c_uint32, POINTER(c_uint32),
                                     POINTER(c_int32)]
    L.rtx_scene_topology.restype = c_int
    L.rtx_walk_tree.argtypes = [POINTER(SceneDesc), c_uint32, c_uint32, POINTER(BvhNode), c_uint32,
                                POINTER(c_uint32), POINTER(c_int32)]
    L.rtx_walk_tree.restype = c_int
    L.rtx_scene_walk_skip.argtypes = [c_void_p, POINTER(Camera), c_void_p, c_uint32, POINTER(c_uint32)]
    L.rtx_scene_walk_skip.restype = c_int
    L.rtx_walk_skip.argtypes = [POINTER(SceneDesc), c_uint32, POINTER(Camera), c_void_p, c_uint32, POINTER(c_uint32)]
    L.rtx_walk_skip.restype = c_int
    L.rtx_scene_near_region.argtypes = [c_void_p, POINTER(Camera), POINTER(c_float), POINTER(c_uint32)]
    L.rtx_scene_near_region.restype = c_int
    L.rtx_scene_near_skip.argtypes = [c_void_p, POINTER(Camera), c_void_p, c_uint32, POINTER(c_uint32)]
    L.rtx_scene_near_skip.restype = c_int
    L.rtx_walk_near_region.argtypes = [POINTER(SceneDesc), c_uint32, POINTER(Camera), POINTER(c_float),
                                       POINTER(c_uint32)]
    L.rtx_walk_near_region.restype = c_int
    L.rtx_camera_octant.argtypes = [POINTER(Camera)]
    L.rtx_camera_octant.restype = c_uint32
    L.rtx_scene_destroy.argtypes = [c_void_p]
    L.rtx_scene_destroy.restype = None
    L.rtx_scene_device_bytes.argtypes = [c_void_p]
    L.rtx_scene_device_bytes.restype = c_uint64
    L.rtx_render.argtypes = [c_void_p, POINTER(Camera), c_uint64, c_int, c_void_p, POINTER(Stats)]
    L.rtx_render.restype = c_int
    L.rtx_render_ex.argtypes = [c_void_p, POINTER(Camera), c_uint64, c_int, c_uint32, c_void_p, POINTER(Stats)]
    L.rtx_render_ex.restype = c_int
    L.rtx_render_region_device.argtypes = [c_void_p, POINTER(Camera), c_uint64, POINTER(Region), c_void_p,
                                           c_void_p, c_uint32, POINTER(Stats)]
    L.rtx_render_region_device.restype = c_int
    L.rtx_region_rows.argtypes = [POINTER(Region)]
    L.rtx_region_rows.restype = c_uint32
    L.rtx_ppm_max_bytes.argtypes = [c_uint32, c_uint32]
    L.rtx_ppm_max_bytes.restype = c_uint64
    L.rtx_encode_ppm_device.argtypes = [c_void_p, c_uint32, c_uint32, c_void_p, c_uint64, POINTER(c_uint64), c_void_p]
    L.rtx_encode_ppm_device.restype = c_int
    L.rtx_render_ppm.argtypes = [c_void_p, POINTER(Camera), c_uint64, c_void_p, c_uint64, POINTER(c_uint64),
                                 POINTER(Stats)]
    L.rtx_render_ppm.restype = c_int
    if hasattr(L, "rtx_render_ppm_ex"):  # ABI 9 (RTX_LIB may name an older build for A/B)
        L.rtx_render_ppm_ex.argtypes = [c_void_p, POINTER(Camera), c_uint64, c_int, c_void_p, c_uint64,
                                        POINTER(c_uint64), POINTER(Stats)]
        L.rtx_render_ppm_ex.restype = c_int
    L.rtx_scene_create_spheres.argtypes = [POINTER(Sphere), c_uint32, POINTER(Material), c_uint32, POINTER(Texture),
                                           c_uint32, POINTER(c_uint32), c_uint64, c_uint64, c_uint64,
                                           POINTER(c_void_p), POINTER(c_double)]
    L.rtx_scene_create_spheres.restype = c_int
    if hasattr(L, "rtx_scene_create_world"):  # ABI 10, additive (RTX_LIB may name an older build for A/B)
        L.rtx_scene_create_world.argtypes = [POINTER(c_int32), c_uint32, POINTER(Sphere), c_uint32, POINTER(Quad),
                                             c_uint32, POINTER(Material), c_uint32, POINTER(Texture), c_uint32,
                                             POINTER(c_uint32), c_uint64, c_uint64, c_uint64, POINTER(c_void_p),
                                             POINTER(c_double)]
        L.rtx_scene_create_world.restype = c_int
        L.rtx_quad_init.argtypes = [POINTER(c_float), POINTER(c_float), POINTER(c_float), c_uint32, POINTER(Quad)]
        L.rtx_quad_init.restype = c_int
        L.rtx_box_quads.argtypes = [POINTER(c_float), POINTER(c_float), c_uint32, POINTER(Quad)]
        L.rtx_box_quads.restype = c_int
    L.rtx_scene_export.argtypes = [c_void_p, c_void_p, c_uint64]
    L.rtx_scene_export.restype = c_uint64
    L.rtx_release_device_memory.argtypes = [c_int]
    L.rtx_release_device_memory.restype = c_int
    L.rtx_device_scratch_bytes.argtypes = [c_int]
    L.rtx_device_scratch_bytes.restype = c_uint64
    if hasattr(L, "rtx_device_check"):  # ABI 10 (RTX_LIB may name an older build for A/B)
        L.rtx_device_check.argtypes = [c_int]
        L.rtx_device_check.restype = c_int
    if hasattr(L, "rtx_accum_create"):  # ABI 10, additive (RTX_LIB may name an older build for A/B)
        L.rtx_accum_create.argtypes = [c_void_p, POINTER(Camera), c_uint64, POINTER(Region), POINTER(c_void_p)]
        L.rtx_accum_create.restype = c_int
        L.rtx_accum_add.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, POINTER(Stats)]
        L.rtx_accum_add.restype = c_int
        L.rtx_accum_samples.argtypes = [c_void_p]
        L.rtx_accum_samples.restype = c_uint32
        L.rtx_accum_resolve_device.argtypes = [c_void_p, c_void_p, c_void_p, c_float, c_void_p, POINTER(c_uint64)]
        L.rtx_accum_resolve_device.restype = c_int
        L.rtx_accum_resolve.argtypes = [c_void_p, c_void_p, c_void_p, c_float, POINTER(c_uint64)]
        L.rtx_accum_resolve.restype = c_int
        L.rtx_accum_ppm.argtypes = [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]
        L.rtx_accum_ppm.restype = c_int
        L.rtx_accum_reset.argtypes = [c_void_p]
        L.rtx_accum_reset.restype = c_int
        L.rtx_accum_destroy.argtypes = [c_void_p]
        L.rtx_accum_destroy.restype = None
    if hasattr(L, "rtx_trace_device"):  # ABI 10, additive (RTX_LIB may name an older build for A/B)
        L.rtx_trace_device.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, POINTER(TraceStats)]
        L.rtx_trace_device.restype = c_int
        L.rtx_trace.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(TraceStats)]
        L.rtx_trace.restype = c_int
    if hasattr(L, "rtx_shade_device"):  # ABI 10, additive (RTX_LIB may name an older build for A/B)
        L.rtx_camera_rays_device.argtypes = [POINTER(Camera), c_uint64, POINTER(Region), c_uint32, c_uint32, c_void_p,
                                             c_void_p, c_void_p]
        L.rtx_camera_rays_device.restype = c_int
        L.rtx_camera_rays.argtypes = [POINTER(Camera), c_uint64, POINTER(Region), c_uint32, c_uint32, c_void_p, c_void_p]
        L.rtx_camera_rays.restype = c_int
        L.rtx_shade_device.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32,
                                       c_void_p, POINTER(ShadeStats)]
        L.rtx_shade_device.restype = c_int
        L.rtx_shade.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32,
                                POINTER(ShadeStats)]
        L.rtx_shade.restype = c_int
    if hasattr(L, "rtx_guides_device"):  # ABI 10, additive (RTX_LIB may name an older build for A/B)
        L.rtx_guides_device.argtypes = [c_void_p, POINTER(Camera), c_uint64, POINTER(Region), c_uint32, c_uint32, c_void_p,
                                        c_void_p, POINTER(GuideStats)]
        L.rtx_guides_device.restype = c_int
        L.rtx_guides.argtypes = [c_void_p, POINTER(Camera), c_uint64, POINTER(Region), c_uint32, c_uint32, c_void_p,
                                 POINTER(GuideStats)]
        L.rtx_guides.restype = c_int
        L.rtx_denoise_defaults.argtypes = [POINTER(DenoiseParams)]
        L.rtx_denoise_defaults.restype = None
        L.rtx_denoise_workspace_bytes.argtypes = [c_uint32, c_uint32]
        L.rtx_denoise_workspace_bytes.restype = c_uint64
        L.rtx_denoise_device.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, POINTER(DenoiseParams), c_void_p,
                                         c_void_p, c_uint64, c_void_p]
        L.rtx_denoise_device.restype = c_int
        L.rtx_denoise.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, POINTER(DenoiseParams), c_void_p]
        L.rtx_denoise.restype = c_int
        L.rtx_accum_preview_device.argtypes = [c_void_p, c_uint32, POINTER(DenoiseParams), c_void_p, c_void_p]
        L.rtx_accum_preview_device.restype = c_int
        L.rtx_accum_preview.argtypes = [c_void_p, c_uint32, POINTER(DenoiseParams), c_void_p]
        L.rtx_accum_preview.restype = c_int
        L.rtx_accum_preview_ppm.argtypes = [c_void_p, c_uint32, POINTER(DenoiseParams), c_void_p, c_uint64,
                                            POINTER(c_uint64)]
        L.rtx_accum_preview_ppm.restype = c_int
    if hasattr(L, "rtx_accum_add_adaptive"):  # adaptive sampling (ABI 10, additive)
        L.rtx_accum_add_adaptive.argtypes = [c_void_p, c_uint32, c_float, c_uint32, c_void_p, c_uint32, POINTER(Stats),
                                             POINTER(AdaptStats)]
        L.rtx_accum_add_adaptive.restype = c_int
        L.rtx_accum_tile_shape.argtypes = [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]
        L.rtx_accum_tile_shape.restype = c_int
        L.rtx_accum_sample_counts_device.argtypes = [c_void_p, c_void_p, c_void_p]
        L.rtx_accum_sample_counts_device.restype = c_int
        L.rtx_accum_sample_counts.argtypes = [c_void_p, c_void_p]
        L.rtx_accum_sample_counts.restype = c_int
    if hasattr(L, "rtx_direct_device"):  # direct light sampling (ABI 10, additive)
        L.rtx_lights.argtypes = [POINTER(SceneDesc), c_void_p, c_uint32, POINTER(c_uint32)]
        L.rtx_lights.restype = c_int
        L.rtx_scene_lights.argtypes = [c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]
        L.rtx_scene_lights.restype = c_int
        L.rtx_direct_device.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p,
                                        POINTER(DirectStats)]
        L.rtx_direct_device.restype = c_int
        L.rtx_direct.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(DirectStats)]
        L.rtx_direct.restype = c_int
        L.rtx_accum_add_direct.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, POINTER(Stats)]
        L.rtx_accum_add_direct.restype = c_int
    if hasattr(L, "rtx_accum_add_mis"):  # multiple importance sampling (ABI 10, additive)
        L.rtx_prim_lights.argtypes = [POINTER(SceneDesc), c_void_p, c_uint32, POINTER(c_uint32), POINTER(c_uint32)]
        L.rtx_prim_lights.restype = c_int
        L.rtx_emitter_weight_device.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_void_p,
                                                POINTER(EmitterStats)]
        L.rtx_emitter_weight_device.restype = c_int
        L.rtx_emitter_weight.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, POINTER(EmitterStats)]
        L.rtx_emitter_weight.restype = c_int
        L.rtx_accum_add_mis.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32, POINTER(Stats)]
        L.rtx_accum_add_mis.restype = c_int
    _lib = L
    return L


def load_host() -> ctypes.CDLL:
    global _host
    if _host is not None:
        return _host
    load()
    path = lib_path("librtxhost.so")
    if not os.path.exists(path):
        raise OSError(f"librtxhost.so not built at {path}")
    H = ctypes.CDLL(path)
    H.rtxhost_build_scene.argtypes = [c_char_p, c_uint64, POINTER(c_void_p)]
    H.rtxhost_build_scene.restype = c_int
    H.rtxhost_scene_free.argtypes = [c_void_p]
    H.rtxhost_scene_free.restype = None
    H.rtxhost_scene_desc.argtypes = [c_void_p]
    H.rtxhost_scene_desc.restype = POINTER(SceneDesc)
    H.rtxhost_scene_camera.argtypes = [c_void_p, c_int32, c_int32, c_int32, POINTER(Camera)]
    H.rtxhost_scene_camera.restype = c_int
    H.rtxhost_render_ppm.argtypes = [c_char_p, c_uint64, c_int32, c_int32, c_int32, c_uint64, c_int32, c_char_p]
    H.rtxhost_render_ppm.restype = c_int
    H.rtxhost_ppm_encode.argtypes = [c_void_p, c_uint32, c_uint32, c_void_p, c_uint64]
    H.rtxhost_ppm_encode.restype = c_uint64
    H.rtxhost_last_error.restype = c_char_p
    H.rtxhost_scene_world_spheres.argtypes = [c_void_p, POINTER(Sphere), c_uint64, POINTER(c_uint64), POINTER(c_uint64)]
    H.rtxhost_scene_world_spheres.restype = ctypes.c_int64
    H.rtxhost_scene_world.argtypes = [c_void_p, POINTER(c_int32), c_uint64, POINTER(Sphere), c_uint64, POINTER(Quad),
                                      c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64),
                                      POINTER(c_uint64)]
    H.rtxhost_scene_world.restype = ctypes.c_int64
    H.rtxhost_synthetic_earth_ycbcr.argtypes = [c_uint64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    H.rtxhost_synthetic_earth_ycbcr.restype = c_int
    H.rtxhost_ycbcr_rgba.argtypes = [ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, POINTER(c_uint32)]
    H.rtxhost_ycbcr_rgba.restype = None
    _host = H
    return H


def quad(Q, u, v, material: int) -> "Quad":
    """rtx_quad_init: NewQuad (hittables.go:149-165), the derived fields w, normal and d filled in."""
    out = Quad()
    vec = [(c_float * 3)(*[float(x) for x in a]) for a in (Q, u, v)]
    check(load().rtx_quad_init(vec[0], vec[1], vec[2], material, ctypes.byref(out)), "rtx_quad_init")
    return out


def box(a, b, material: int):
    """rtx_box_quads: the six quads of Box(a, b) (hittables.go:200-216), a ctypes array of Quad."""
    out = (Quad * 6)()
    vec = [(c_float * 3)(*[float(x) for x in p]) for p in (a, b)]
    check(load().rtx_box_quads(vec[0], vec[1], material, out), "rtx_box_quads")
    return out


class RtxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtx error {code}: {msg}")
        self.code = code


def check(rc: int, where: str = "rtx") -> None:
    if rc != RTX_OK:
        msg = load().rtx_last_error().decode()
        raise RtxError(rc, f"{where}: {msg}")


class HostScene:
    """A main.go scene built by the C++ mirror (NewBVH + flatten)."""

    def __init__(self, name: str, seed: int = 1):
        H = load_host()
        h = c_void_p()
        rc = H.rtxhost_build_scene(name.encode(), seed, ctypes.byref(h))
        if rc != RTX_OK:
            raise RtxError(rc, H.rtxhost_last_error().decode())
        self._h = h
        self.name = name
        self.seed = seed

    @property
    def desc(self):
        d = load_host().rtxhost_scene_desc(self._h)
        d._owner = self  # the tables live in this scene: keep it alive as long as the pointer
        return d

    def camera(self, width: int = 0, spp: int = 0, depth: int = 0) -> Camera:
        cam = Camera()
        rc = load_host().rtxhost_scene_camera(self._h, width, spp, depth, ctypes.byref(cam))
        if rc != RTX_OK:
            raise RtxError(rc, load_host().rtxhost_last_error().decode())
        return cam

    def world_spheres(self):
        """(Sphere array in World.Add order, BVH draw position, seed): rtx_scene_create_spheres' inputs."""
        H = load_host()
        draw0, seed = c_uint64(), c_uint64()
        n = H.rtxhost_scene_world_spheres(self._h, None, 0, None, None)
        if n < 0:
            raise RtxError(int(n), H.rtxhost_last_error().decode())
        arr = (Sphere * max(int(n), 1))()
        H.rtxhost_scene_world_spheres(self._h, arr, n, ctypes.byref(draw0), ctypes.byref(seed))
        return arr, int(n), draw0.value, seed.value

    def world(self):
        """(items, spheres, quads, BVH draw position, seed): rtx_scene_create_world's inputs.  items: int32 refs in
        World.Add order (a ctypes array); spheres, quads: ctypes arrays numbered in Add order per kind (their lengths
        are the counts), materials indexing self.desc's table."""
        H = load_host()
        ns, nq, draw0, seed = c_uint64(), c_uint64(), c_uint64(), c_uint64()
        n = H.rtxhost_scene_world(self._h, None, 0, None, 0, None, 0, ctypes.byref(ns), ctypes.byref(nq), None, None)
        if n < 0:
            raise RtxError(int(n), H.rtxhost_last_error().decode())
        items, spheres, quads = (c_int32 * int(n))(), (Sphere * ns.value)(), (Quad * nq.value)()
        H.rtxhost_scene_world(self._h, items, n, spheres, ns.value, quads, nq.value, None, None, ctypes.byref(draw0),
                              ctypes.byref(seed))
        return items, spheres, quads, draw0.value, seed.value

    def close(self) -> None:
        if self._h:
            load_host().rtxhost_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """rtx_scene_create: the tables uploaded once to the current HIP device."""

    def __init__(self, desc_ptr=None, handle=None, reference_bvh: bool = False, every_box: bool = False,
                 no_tier: bool = False):
        L = load()
        self.build_ms = None
        if handle is not None:
            self._h = handle
            return
        h = c_void_p()
        flags = ((RTX_SCENE_REFERENCE_BVH if reference_bvh else 0) | (RTX_SCENE_EVERY_BOX if every_box else 0) |
                 (RTX_SCENE_NO_TIER if no_tier else 0))
        check(L.rtx_scene_create_ex(desc_ptr, flags, ctypes.byref(h)), "rtx_scene_create_ex")
        self._h = h

    @classmethod
    def from_spheres(cls, host: "HostScene") -> "DeviceScene":
        """rtx_scene_create_spheres: the BVH of host's World built on the GPU."""
        L = load()
        arr, n, draw0, seed = host.world_spheres()
        d = host.desc.contents
        h = c_void_p()
        ms = c_double()
        check(L.rtx_scene_create_spheres(arr, n, d.materials, d.n_materials, d.textures, d.n_textures, d.texels,
                                         d.n_texels, seed, draw0, ctypes.byref(h), ctypes.byref(ms)),
              "rtx_scene_create_spheres")
        obj = cls(handle=h)
        obj.build_ms = ms.value
        return obj

    @classmethod
    def from_tables(cls, items, spheres, quads, tables, seed: int, draw0: int = 0) -> "DeviceScene":
        """rtx_scene_create_world: NewBVHFromWorld of a World of spheres and quads, built on the GPU.  items: the
        World's list in Add order, rtx.ref_prim refs (a ctypes int32 array or a sequence), or None for every sphere,
        then every quad; spheres, quads: ctypes arrays (or None); tables: a SceneDesc (or a pointer to one) whose
        material, texture and texel tables the scene takes.  Sets build_ms."""
        L = load()
        t = tables.contents if hasattr(tables, "contents") else tables
        ns, nq = (len(spheres) if spheres is not None else 0), (len(quads) if quads is not None else 0)
        if items is None:
            n_items = ns + nq
        else:
            if not isinstance(items, ctypes.Array):
                items = (c_int32 * len(items))(*[int(r) for r in items])
            n_items = len(items)
        h, ms = c_void_p(), c_double()
        check(L.rtx_scene_create_world(items, n_items, spheres if ns else None, ns, quads if nq else None, nq,
                                       t.materials, t.n_materials, t.textures, t.n_textures, t.texels, t.n_texels,
                                       seed, draw0, ctypes.byref(h), ctypes.byref(ms)), "rtx_scene_create_world")
        obj = cls(handle=h)
        obj.build_ms = ms.value
        return obj

    @classmethod
    def from_world(cls, host: "HostScene") -> "DeviceScene":
        """rtx_scene_create_world over host's World (spheres and quads): its BVH built on the GPU."""
        items, spheres, quads, draw0, seed = host.world()
        return cls.from_tables(items, spheres, quads, host.desc, seed, draw0)

    def export(self) -> bytes:
        L = load()
        n = int(L.rtx_scene_export(self._h, None, 0))
        buf = ctypes.create_string_buffer(n)
        L.rtx_scene_export(self._h, buf, n)
        return buf.raw

    @property
    def handle(self):
        return self._h

    def device_bytes(self) -> int:
        return load().rtx_scene_device_bytes(self._h)

    def topology(self, octant: int):
        """(nodes ctypes array, root) of the tree the scene walks for a camera octant, or None when
        the scene walks the caller's tree (rtx_scene_topology)."""
        L = load()
        n, root = c_uint32(), c_int32()
        check(L.rtx_scene_topology(self._h, octant, None, 0, ctypes.byref(n), ctypes.byref(root)), "rtx_scene_topology")
        if n.value == 0 and root.value == -1:
            return None
        arr = (BvhNode * max(n.value, 1))()
        check(L.rtx_scene_topology(self._h, octant, arr, n.value, ctypes.byref(n), ctypes.byref(root)),
              "rtx_scene_topology")
        return arr, int(n.value), int(root.value)

    def walk_desc(self, desc_ptr, cam: Camera):
        """The scene description of the tree the scene walks for `cam` (the caller's own when the
        scene keeps it): same spheres, materials and textures, the walk's nodes and root.  The
        oracle rendering this description takes the kernel's box and primitive tests one for one."""
        t = self.topology(camera_octant(cam))
        if t is None:
            return desc_ptr
        arr, n, root = t
        return desc_with_tree(desc_ptr, arr, n, root)

    def near_region(self, cam: Camera):
        """(box (6 floats: min xyz, max xyz) or None, active) — rtx_scene_near_region."""
        box, act = (c_float * 6)(), c_uint32()
        for i in range(6):
            box[i] = float("nan")
        check(load().rtx_scene_near_region(self._h, ctypes.byref(cam), box, ctypes.byref(act)), "rtx_scene_near_region")
        vals = [float(v) for v in box]
        return (None if vals[0] != vals[0] else vals), bool(act.value)

    def near_desc(self, desc_ptr, cam: Camera):
        """The description of the near tree the scene walks for cam (rtx_scene_topology octant | RTX_TREE_NEAR)."""
        t = self.topology(camera_octant(cam) | RTX_TREE_NEAR)
        if t is None:
            return None
        arr, n, root = t
        return desc_with_tree(desc_ptr, arr, n, root)

    def near_skip(self, cam: Camera):
        """rtx_scene_near_skip: the near walk's skips for cam (numpy uint8)."""
        return _skip_mask(lambda buf, cap, n: load().rtx_scene_near_skip(self._h, ctypes.byref(cam), buf, cap, n),
                          "rtx_scene_near_skip")

    def walk_skip(self, cam: Camera):
        """rtx_scene_walk_skip: per node entry of the uncollapsed walk for cam (visit order), 1 where
        the collapsed walk leaves its box test out (numpy uint8)."""
        return _skip_mask(lambda buf, cap, n: load().rtx_scene_walk_skip(self._h, ctypes.byref(cam), buf, cap, n),
                          "rtx_scene_walk_skip")

    def render_region(self, cam: Camera, seed: int, region: Region, out_ptr: int, stream: int = 0,
                      counters: bool = False, timed: bool = False, flags: int = 0):
        """Enqueue (and optionally wait/time) a region render into device memory at out_ptr."""
        st = Stats() if (timed or counters) else None
        rc = load().rtx_render_region_device(self._h, ctypes.byref(cam), seed, ctypes.byref(region),
                                             c_void_p(out_ptr), c_void_p(stream),
                                             flags | (RTX_FLAG_COUNTERS if counters else 0),
                                             ctypes.byref(st) if st is not None else None)
        check(rc, "rtx_render_region_device")
        return st

    def render_host(self, cam: Camera, seed: int, n_gpus: int = 1, stats: bool = False, counters: bool = False,
                    out=None):
        """rtx_render (counters=False: the timed kernel) or rtx_render_ex(RTX_FLAG_COUNTERS) into a host array
        (`out`: a C-contiguous float32 [H, W, 3] to reuse, else a new one)."""
        import numpy as np
        if out is None:
            out = np.zeros((cam.image_height, cam.image_width, 3), dtype=np.float32)
        assert out.dtype == np.float32 and out.shape == (cam.image_height, cam.image_width, 3) and out.flags.c_contiguous
        st = Stats() if (stats or counters) else None
        if counters:
            rc = load().rtx_render_ex(self._h, ctypes.byref(cam), seed, n_gpus, RTX_FLAG_COUNTERS,
                                      out.ctypes.data_as(c_void_p), ctypes.byref(st))
        else:
            rc = load().rtx_render(self._h, ctypes.byref(cam), seed, n_gpus, out.ctypes.data_as(c_void_p),
                                   ctypes.byref(st) if st is not None else None)
        check(rc, "rtx_render")
        return out, st

    def render_ppm(self, cam: Camera, seed: int) -> bytes:
        """rtx_render_ppm: the P3 bytes Render writes, rendered and encoded on the GPU."""
        import numpy as np
        L = load()
        cap = int(L.rtx_ppm_max_bytes(cam.image_width, cam.image_height))
        buf = np.empty(cap, dtype=np.uint8)  # not zero-filled: 63 B per pixel of capacity, ~12 used
        n = c_uint64()
        check(L.rtx_render_ppm(self._h, ctypes.byref(cam), seed, buf.ctypes.data_as(c_void_p), cap, ctypes.byref(n),
                               None), "rtx_render_ppm")
        return buf[: n.value].tobytes()

    def render_ppm_ex(self, cam: Camera, seed: int, n_gpus: int = 1, stats: bool = False):
        """rtx_render_ppm_ex (ABI 9): the bands of rtx_render(n_gpus) gathered to device 0, the PPM encoded
        there; returns the bytes (and the Stats when stats=True)."""
        import numpy as np
        L = load()
        cap = int(L.rtx_ppm_max_bytes(cam.image_width, cam.image_height))
        buf = np.empty(cap, dtype=np.uint8)
        n = c_uint64()
        st = Stats()
        check(L.rtx_render_ppm_ex(self._h, ctypes.byref(cam), seed, n_gpus, buf.ctypes.data_as(c_void_p), cap,
                                  ctypes.byref(n), ctypes.byref(st)), "rtx_render_ppm_ex")
        out = buf[: n.value].tobytes()
        return (out, st) if stats else out

    def trace_device(self, rays_ptr: int, n: int, hits_ptr: int, flags: int = 0, stream: int = 0, stats: bool = False):
        """rtx_trace_device: n rtx_ray at rays_ptr -> n rtx_hit at hits_ptr, device memory of the current device
        (16-B aligned: a torch tensor's data_ptr()).  Enqueues and returns None, or with stats=True waits and returns
        the TraceStats (flags | RTX_TRACE_COUNTERS fills its work counters)."""
        st = TraceStats() if stats else None
        check(load().rtx_trace_device(self._h, c_void_p(rays_ptr), n, c_void_p(hits_ptr), flags, c_void_p(stream),
                                      ctypes.byref(st) if st is not None else None), "rtx_trace_device")
        return st

    def trace(self, rays, flags: int = 0, stats: bool = False):
        """rtx_trace: a numpy array of RAY_DTYPE in, an array of HIT_DTYPE of the same shape out (and the TraceStats
        with stats=True).  Blocking."""
        import numpy as np
        ray_t, hit_t = __getattr__("RAY_DTYPE"), __getattr__("HIT_DTYPE")
        rays = np.asarray(rays)
        if rays.dtype != ray_t:
            raise TypeError(f"rays must have dtype rtx.RAY_DTYPE, not {rays.dtype}")
        n = rays.size
        # 16-B aligned copies: numpy aligns a structured array to its widest field only (4 B)
        src = _aligned_empty(n, ray_t)
        src[...] = rays.reshape(-1)
        out = _aligned_empty(n, hit_t)
        st = TraceStats() if stats else None
        check(load().rtx_trace(self._h, src.ctypes.data_as(c_void_p), n, out.ctypes.data_as(c_void_p), flags,
                               ctypes.byref(st) if st is not None else None), "rtx_trace")
        out = out.reshape(rays.shape)
        return (out, st) if stats else out

    def shade_device(self, seed: int, rays_ptr: int, hits_ptr: int, keys_ptr: int, n: int, out_ptr: int, flags: int = 0,
                     stream: int = 0, stats: bool = False):
        """rtx_shade_device: n records of rtx_ray / rtx_hit / rtx_path_key in lock step -> n rtx_bounce at out_ptr,
        device memory of the current device (16-B aligned).  Enqueues and returns None, or with stats=True waits and
        returns the ShadeStats (flags | RTX_SHADE_COUNTERS fills its work counters)."""
        st = ShadeStats() if stats else None
        check(load().rtx_shade_device(self._h, seed, c_void_p(rays_ptr), c_void_p(hits_ptr), c_void_p(keys_ptr), n,
                                      c_void_p(out_ptr), flags, c_void_p(stream),
                                      ctypes.byref(st) if st is not None else None), "rtx_shade_device")
        return st

    def shade(self, rays, hits, keys, seed: int, stats: bool = False, flags: int = 0):
        """rtx_shade: numpy arrays of RAY_DTYPE, HIT_DTYPE and KEY_DTYPE of one shape in, an array of BOUNCE_DTYPE of
        that shape out (and the ShadeStats with stats=True, counters filled with flags=RTX_SHADE_COUNTERS).
        Blocking."""
        import numpy as np
        types = [__getattr__(t) for t in ("RAY_DTYPE", "HIT_DTYPE", "KEY_DTYPE")]
        arrs = [np.asarray(a) for a in (rays, hits, keys)]
        for a, t, what in zip(arrs, types, ("rays", "hits", "keys")):
            if a.dtype != t:
                raise TypeError(f"{what} must have dtype {t}, not {a.dtype}")
            if a.shape != arrs[0].shape:
                raise ValueError("rays, hits and keys must have one shape")
        n = arrs[0].size
        src = []
        for a, t in zip(arrs, types):  # 16-B aligned copies
            b = _aligned_empty(n, t)
            b[...] = a.reshape(-1)
            src.append(b)
        out = _aligned_empty(n, __getattr__("BOUNCE_DTYPE"))
        st = ShadeStats() if stats else None
        check(load().rtx_shade(self._h, seed, *[b.ctypes.data_as(c_void_p) for b in src], n,
                               out.ctypes.data_as(c_void_p), flags, ctypes.byref(st) if st is not None else None),
              "rtx_shade")
        out = out.reshape(arrs[0].shape)
        return (out, st) if stats else out

    def guides_device(self, cam: Camera, seed: int, region: Region, first: int, count: int, guides_ptr: int,
                      stream: int = 0, stats: bool = False):
        """rtx_guides_device: the first-hit guides (rtx_guide, 32 B per pixel of the region's shard, 16-B aligned) of
        samples [first, first + count) into device memory of the current device.  Enqueues and returns None, or with
        stats=True waits and returns the GuideStats."""
        st = GuideStats() if stats else None
        check(load().rtx_guides_device(self._h, ctypes.byref(cam), seed, ctypes.byref(region), first, count,
                                       c_void_p(guides_ptr), c_void_p(stream),
                                       ctypes.byref(st) if st is not None else None), "rtx_guides_device")
        return st

    def guides(self, cam: Camera, seed: int, region: Region, first: int = 0, count=None, stats: bool = False):
        """rtx_guides: an array of GUIDE_DTYPE of shape (rows, width) (and the GuideStats with stats=True); count
        defaults to the camera's samples_per_pixel.  Blocking."""
        if count is None:
            count = cam.samples_per_pixel
        rows = region_rows(region)
        out = _aligned_empty(rows * region.width, __getattr__("GUIDE_DTYPE"))
        st = GuideStats() if stats else None
        check(load().rtx_guides(self._h, ctypes.byref(cam), seed, ctypes.byref(region), first, count,
                                out.ctypes.data_as(c_void_p), ctypes.byref(st) if st is not None else None), "rtx_guides")
        out = out.reshape(rows, region.width)
        return (out, st) if stats else out

    def lights(self):
        """rtx_scene_lights: the scene's emitter table, an array of LIGHT_DTYPE (prim coded as Hit.prim, area)."""
        L = load()
        return _light_table(lambda out, cap, n: L.rtx_scene_lights(self._h, out, cap, n), "rtx_scene_lights")

    def direct_device(self, seed: int, hits_ptr: int, keys_ptr: int, n: int, out_ptr: int, flags: int = 0, stream: int = 0,
                      stats: bool = False):
        """rtx_direct_device: n records of rtx_hit / rtx_path_key in lock step -> n rtx_direct_sample at out_ptr,
        device memory of the current device (16-B aligned).  Enqueues and returns None, or with stats=True waits and
        returns the DirectStats (flags | RTX_DIRECT_COUNTERS fills its counters)."""
        st = DirectStats() if stats else None
        check(load().rtx_direct_device(self._h, seed, c_void_p(hits_ptr), c_void_p(keys_ptr), n, c_void_p(out_ptr), flags,
                                       c_void_p(stream), ctypes.byref(st) if st is not None else None), "rtx_direct_device")
        return st

    def direct(self, hits, keys, seed: int, stats: bool = False, flags: int = 0):
        """rtx_direct: numpy arrays of HIT_DTYPE and KEY_DTYPE of one shape in, an array of DIRECT_DTYPE of that shape
        out (and the DirectStats with stats=True, counters filled with flags=RTX_DIRECT_COUNTERS).  Blocking."""
        import numpy as np
        types = [__getattr__(t) for t in ("HIT_DTYPE", "KEY_DTYPE")]
        arrs = [np.asarray(a) for a in (hits, keys)]
        for a, t, what in zip(arrs, types, ("hits", "keys")):
            if a.dtype != t:
                raise TypeError(f"{what} must have dtype {t}, not {a.dtype}")
            if a.shape != arrs[0].shape:
                raise ValueError("hits and keys must have one shape")
        n = arrs[0].size
        src = []
        for a, t in zip(arrs, types):  # 16-B aligned copies
            b = _aligned_empty(n, t)
            b[...] = a.reshape(-1)
            src.append(b)
        out = _aligned_empty(n, __getattr__("DIRECT_DTYPE"))
        st = DirectStats() if stats else None
        check(load().rtx_direct(self._h, seed, *[b.ctypes.data_as(c_void_p) for b in src], n,
                                out.ctypes.data_as(c_void_p), flags, ctypes.byref(st) if st is not None else None),
              "rtx_direct")
        out = out.reshape(arrs[0].shape)
        return (out, st) if stats else out

    def emitter_weight_device(self, from_ptr: int, hits_ptr: int, n: int, out_ptr: int, flags: int = 0, stream: int = 0,
                              stats: bool = False):
        """rtx_emitter_weight_device: n pairs of rtx_hit (the hit a bounce left, the hit it found) -> n
        rtx_emitter_weight_record at out_ptr, device memory of the current device (16-B aligned).  Enqueues and returns
        None, or with stats=True waits and returns the EmitterStats (flags | RTX_EMITTER_COUNTERS fills `weighted`)."""
        st = EmitterStats() if stats else None
        check(load().rtx_emitter_weight_device(self._h, c_void_p(from_ptr), c_void_p(hits_ptr), n, c_void_p(out_ptr), flags,
                                               c_void_p(stream), ctypes.byref(st) if st is not None else None),
              "rtx_emitter_weight_device")
        return st

    def emitter_weight(self, from_hits, hits, stats: bool = False, flags: int = 0):
        """rtx_emitter_weight: two numpy arrays of HIT_DTYPE of one shape in, an array of EMITTER_WEIGHT_DTYPE of that
        shape out (and the EmitterStats with stats=True).  Blocking."""
        import numpy as np
        t = __getattr__("HIT_DTYPE")
        arrs = [np.asarray(a) for a in (from_hits, hits)]
        for a, what in zip(arrs, ("from_hits", "hits")):
            if a.dtype != t:
                raise TypeError(f"{what} must have dtype {t}, not {a.dtype}")
            if a.shape != arrs[0].shape:
                raise ValueError("from_hits and hits must have one shape")
        n = arrs[0].size
        src = []
        for a in arrs:  # 16-B aligned copies
            b = _aligned_empty(n, t)
            b[...] = a.reshape(-1)
            src.append(b)
        out = _aligned_empty(n, __getattr__("EMITTER_WEIGHT_DTYPE"))
        st = EmitterStats() if stats else None
        check(load().rtx_emitter_weight(self._h, *[b.ctypes.data_as(c_void_p) for b in src], n,
                                        out.ctypes.data_as(c_void_p), flags, ctypes.byref(st) if st is not None else None),
              "rtx_emitter_weight")
        out = out.reshape(arrs[0].shape)
        return (out, st) if stats else out

    def accumulator(self, cam: Camera, seed: int, region: Region) -> "Accumulator":
        """rtx_accum_create on the current device: progressive passes over `region` (close it before the scene)."""
        return Accumulator(self, cam, seed, region)

    def close(self) -> None:
        if self._h:
            load().rtx_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator:
    """rtx_accum: sample passes over one (scene, device, camera, seed, region) that can be resolved in between.
    After n samples resolve() is bit-identical to a one-shot render with samples_per_pixel = n.  The caller orders
    the passes and resolves of one accumulator (the same stream, or a synchronise between)."""

    def __init__(self, scene: DeviceScene, cam: Camera, seed: int, region: Region):
        h = c_void_p()
        check(load().rtx_accum_create(scene.handle, ctypes.byref(cam), seed, ctypes.byref(region), ctypes.byref(h)),
              "rtx_accum_create")
        self._h = h
        self._scene = scene  # destroyed after the accumulator
        self.width = region.width
        self.rows = region_rows(region)

    def add(self, count: int, stream: int = 0, stats: bool = False, counters: bool = False, flags: int = 0):
        """One pass of `count` samples per pixel; returns the pass's Stats (after waiting) when asked for."""
        st = Stats() if (stats or counters) else None
        check(load().rtx_accum_add(self._h, count, c_void_p(stream), flags | (RTX_FLAG_COUNTERS if counters else 0),
                                   ctypes.byref(st) if st is not None else None), "rtx_accum_add")
        return st

    def add_direct(self, count: int, stream: int = 0, stats: bool = False, flags: int = 0):
        """rtx_accum_add_direct: `count` more samples per pixel by the direct-light estimator, one fused
        kernel.  An accumulator is plain, adaptive or direct until reset().  Returns the pass's Stats with stats=True
        (which waits), else None."""
        st = Stats() if stats else None
        check(load().rtx_accum_add_direct(self._h, count, c_void_p(stream), flags,
                                          ctypes.byref(st) if st is not None else None), "rtx_accum_add_direct")
        return st

    def add_mis(self, count: int, stream: int = 0, stats: bool = False, flags: int = 0):
        """rtx_accum_add_mis: `count` more samples per pixel by the direct-light estimator with the light sample and the
        bounce weighted by the power heuristic, one fused kernel.  An accumulator is plain, adaptive,
        direct or MIS until reset().  Returns the pass's Stats with stats=True (which waits), else None."""
        st = Stats() if stats else None
        check(load().rtx_accum_add_mis(self._h, count, c_void_p(stream), flags,
                                       ctypes.byref(st) if st is not None else None), "rtx_accum_add_mis")
        return st

    def add_adaptive(self, count: int, rel_tol: float, min_samples: int = 1, stream: int = 0, stats: bool = True,
                     counters: bool = False, flags: int = 0):
        """rtx_accum_add_adaptive: close the open tiles without a noisy pixel at rel_tol (once min_samples have been
        offered), then `count` samples for the pixels of the tiles still open.  Returns (Stats, AdaptStats) after
        waiting (AdaptStats.open_tiles == 0: nothing was sampled, stop), or (None, None) with stats=False (enqueued)."""
        want = stats or counters
        st, ad = (Stats(), AdaptStats()) if want else (None, None)
        check(load().rtx_accum_add_adaptive(self._h, count, rel_tol, min_samples, c_void_p(stream),
                                            flags | (RTX_FLAG_COUNTERS if counters else 0),
                                            ctypes.byref(st) if want else None, ctypes.byref(ad) if want else None),
              "rtx_accum_add_adaptive")
        return st, ad

    @property
    def tile_shape(self):
        """rtx_accum_tile_shape: (width, height) of the tiles an adaptive pass opens and closes."""
        w, h = c_uint32(), c_uint32()
        check(load().rtx_accum_tile_shape(self._h, ctypes.byref(w), ctypes.byref(h)), "rtx_accum_tile_shape")
        return int(w.value), int(h.value)

    def sample_counts_device(self, counts_ptr: int, stream: int = 0) -> None:
        """rtx_accum_sample_counts_device: uint32 [rows, width] into device memory, the samples each pixel received."""
        check(load().rtx_accum_sample_counts_device(self._h, c_void_p(counts_ptr), c_void_p(stream)),
              "rtx_accum_sample_counts_device")

    def sample_counts(self):
        """rtx_accum_sample_counts: uint32 [rows, width], the samples each pixel received.  Blocking."""
        import numpy as np
        out = np.zeros((self.rows, self.width), dtype=np.uint32)
        check(load().rtx_accum_sample_counts(self._h, out.ctypes.data_as(c_void_p)), "rtx_accum_sample_counts")
        return out

    @property
    def samples(self) -> int:
        return int(load().rtx_accum_samples(self._h))

    def resolve_device(self, rgb_ptr: int, var_ptr: int = 0, rel_tol: float = 0.0, stream: int = 0,
                       count_noisy: bool = False):
        """rtx_accum_resolve_device into device memory; returns the noisy-pixel count (after waiting) when
        count_noisy, else None (enqueued only)."""
        n = c_uint64()
        check(load().rtx_accum_resolve_device(self._h, c_void_p(rgb_ptr), c_void_p(var_ptr) if var_ptr else None,
                                              rel_tol, c_void_p(stream), ctypes.byref(n) if count_noisy else None),
              "rtx_accum_resolve_device")
        return int(n.value) if count_noisy else None

    def resolve(self, rel_tol: float = 0.0):
        """(rgb, var, noisy): float32 [rows, width, 3] host arrays and the noisy-pixel count at rel_tol."""
        import numpy as np
        rgb = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        var = np.zeros_like(rgb)
        n = c_uint64()
        check(load().rtx_accum_resolve(self._h, rgb.ctypes.data_as(c_void_p), var.ctypes.data_as(c_void_p), rel_tol,
                                       ctypes.byref(n)), "rtx_accum_resolve")
        return rgb, var, int(n.value)

    def ppm(self) -> bytes:
        """rtx_accum_ppm: the P3 bytes of the image so far."""
        import numpy as np
        L = load()
        cap = int(L.rtx_ppm_max_bytes(self.width, self.rows))
        buf = np.empty(cap, dtype=np.uint8)
        n = c_uint64()
        check(L.rtx_accum_ppm(self._h, buf.ctypes.data_as(c_void_p), cap, ctypes.byref(n)), "rtx_accum_ppm")
        return buf[: n.value].tobytes()

    def preview_device(self, out_ptr: int, guide_samples: int = 4, params: "DenoiseParams" = None, stream: int = 0) -> None:
        """rtx_accum_preview_device: the denoised image so far (3 floats per pixel, 16-B aligned) into device memory:
        resolve, guides over the first min(n, guide_samples) samples, filter (params None: the defaults).  Enqueues."""
        check(load().rtx_accum_preview_device(self._h, guide_samples, ctypes.byref(params) if params is not None else None,
                                              c_void_p(out_ptr), c_void_p(stream)), "rtx_accum_preview_device")

    def preview(self, guide_samples: int = 4, params: "DenoiseParams" = None):
        """rtx_accum_preview: float32 [rows, width, 3], the denoised image so far.  Blocking."""
        import numpy as np
        rgb = np.zeros((self.rows, self.width, 3), dtype=np.float32)
        check(load().rtx_accum_preview(self._h, guide_samples, ctypes.byref(params) if params is not None else None,
                                       rgb.ctypes.data_as(c_void_p)), "rtx_accum_preview")
        return rgb

    def preview_ppm(self, guide_samples: int = 4, params: "DenoiseParams" = None) -> bytes:
        """rtx_accum_preview_ppm: the P3 bytes of the denoised image so far."""
        import numpy as np
        L = load()
        cap = int(L.rtx_ppm_max_bytes(self.width, self.rows))
        buf = np.empty(cap, dtype=np.uint8)
        n = c_uint64()
        check(L.rtx_accum_preview_ppm(self._h, guide_samples, ctypes.byref(params) if params is not None else None,
                                      buf.ctypes.data_as(c_void_p), cap, ctypes.byref(n)), "rtx_accum_preview_ppm")
        return buf[: n.value].tobytes()

    def reset(self) -> None:
        check(load().rtx_accum_reset(self._h), "rtx_accum_reset")

    def close(self) -> None:
        if self._h:
            load().rtx_accum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _aligned_empty(n: int, dtype):
    """n records of a structured dtype starting on a 16-B boundary (rtx_trace's rule), uninitialised."""
    import numpy as np
    raw = np.empty(n * dtype.itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + n * dtype.itemsize].view(dtype)


def _light_table(call, where: str):
    import numpy as np
    n = c_uint32()
    check(call(None, 0, ctypes.byref(n)), where)
    out = np.zeros(n.value, __getattr__("LIGHT_DTYPE"))
    if n.value:
        check(call(out.ctypes.data_as(c_void_p), n.value, ctypes.byref(n)), where)
    return out


def lights(desc_ptr):
    """rtx_lights: the emitter table of a scene description, an array of LIGHT_DTYPE.  Host only: no scene, no device."""
    L = load()
    return _light_table(lambda out, cap, n: L.rtx_lights(desc_ptr, out, cap, n), "rtx_lights")


def prim_lights(desc_ptr):
    """rtx_prim_lights: (the per-primitive emitter lookup of a scene description, an array of PRIM_LIGHT_DTYPE: the
    caller's spheres, then its quads; the number of spheres).  Host only: no scene, no device."""
    import numpy as np
    L = load()
    ns, n = c_uint32(), c_uint32()
    check(L.rtx_prim_lights(desc_ptr, None, 0, ctypes.byref(ns), ctypes.byref(n)), "rtx_prim_lights")
    out = np.zeros(n.value, __getattr__("PRIM_LIGHT_DTYPE"))
    if n.value:
        check(L.rtx_prim_lights(desc_ptr, out.ctypes.data_as(c_void_p), n.value, ctypes.byref(ns), ctypes.byref(n)),
              "rtx_prim_lights")
    return out, ns.value


def camera_rays_device(cam: Camera, seed: int, region: Region, first: int, count: int, rays_ptr: int, keys_ptr: int = 0,
                       stream: int = 0) -> None:
    """rtx_camera_rays_device: GetRay of samples [first, first + count) of the region's shard into device memory of
    the current device, sample-major (record (k - first) * P + i * width + x - x0); keys_ptr may be 0.  Enqueues."""
    check(load().rtx_camera_rays_device(ctypes.byref(cam), seed, ctypes.byref(region), first, count, c_void_p(rays_ptr),
                                        c_void_p(keys_ptr) if keys_ptr else None, c_void_p(stream)),
          "rtx_camera_rays_device")


def camera_rays(cam: Camera, seed: int, region: Region, first: int = 0, count=None):
    """rtx_camera_rays: (rays, keys), arrays of RAY_DTYPE and KEY_DTYPE of shape (count, rows, width); count defaults
    to the camera's samples_per_pixel.  Blocking."""
    if count is None:
        count = cam.samples_per_pixel
    rows = region_rows(region)
    n = count * rows * region.width
    rays = _aligned_empty(n, __getattr__("RAY_DTYPE"))
    keys = _aligned_empty(n, __getattr__("KEY_DTYPE"))
    check(load().rtx_camera_rays(ctypes.byref(cam), seed, ctypes.byref(region), first, count,
                                 rays.ctypes.data_as(c_void_p), keys.ctypes.data_as(c_void_p)), "rtx_camera_rays")
    shape = (count, rows, region.width)
    return rays.reshape(shape), keys.reshape(shape)


def denoise_workspace_bytes(width: int, rows: int) -> int:
    """rtx_denoise_workspace_bytes: the bytes of workspace rtx_denoise_device needs for a width x rows image."""
    return int(load().rtx_denoise_workspace_bytes(width, rows))


def denoise_device(rgb_ptr: int, var_ptr: int, guides_ptr: int, width: int, rows: int, out_ptr: int, work_ptr: int,
                   work_bytes: int, params: "DenoiseParams" = None, stream: int = 0) -> None:
    """rtx_denoise_device: the edge-avoiding filter of a resolved image (rgb, var: 3 floats per pixel; guides: rtx_guide)
    into out, device memory of the current device, every pointer 16-B aligned (params None: the defaults).  Enqueues."""
    if params is None:
        params = DenoiseParams.defaults()
    check(load().rtx_denoise_device(c_void_p(rgb_ptr), c_void_p(var_ptr), c_void_p(guides_ptr), width, rows,
                                    ctypes.byref(params), c_void_p(out_ptr), c_void_p(work_ptr), work_bytes,
                                    c_void_p(stream)), "rtx_denoise_device")


def denoise(rgb, var, guides, params: "DenoiseParams" = None):
    """rtx_denoise: float32 [rows, width, 3] rgb and var and a [rows, width] array of GUIDE_DTYPE in, the filtered
    float32 [rows, width, 3] image out.  Blocking."""
    import numpy as np
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    guides = np.ascontiguousarray(guides)
    if guides.dtype != __getattr__("GUIDE_DTYPE"):
        raise TypeError(f"guides must have dtype rtx.GUIDE_DTYPE, not {guides.dtype}")
    if rgb.ndim != 3 or rgb.shape[2] != 3 or var.shape != rgb.shape or guides.shape != rgb.shape[:2]:
        raise ValueError("rgb and var must be [rows, width, 3] and guides [rows, width]")
    if params is None:
        params = DenoiseParams.defaults()
    out = np.zeros_like(rgb)
    check(load().rtx_denoise(rgb.ctypes.data_as(c_void_p), var.ctypes.data_as(c_void_p), guides.ctypes.data_as(c_void_p),
                             rgb.shape[1], rgb.shape[0], ctypes.byref(params), out.ctypes.data_as(c_void_p)), "rtx_denoise")
    return out


def release_device_memory(device: int = -1) -> None:
    """rtx_release_device_memory: free the per-device scratch (and RCCL communicators)."""
    check(load().rtx_release_device_memory(device), "rtx_release_device_memory")


def device_scratch_bytes(device: int = 0) -> int:
    return int(load().rtx_device_scratch_bytes(device))


def device_check(device: int = 0) -> None:
    """rtx_device_check (ABI 10): wait for every render enqueued on `device` and raise RtxError
    (RTX_ERR_HIP) if any of them failed in the kernel since the last report (watchdog, partial-wave claim)."""
    check(load().rtx_device_check(device), "rtx_device_check")


def synthetic_earth_ycbcr(seed: int, w: int = 2048, h: int = 1024):
    """(Y [h, w], Cb, Cr [(h+1)//2, (w+1)//2]) uint8 planes of the earth scenes' *image.YCbCr map."""
    import numpy as np
    cw, ch = (w + 1) // 2, (h + 1) // 2
    Y = np.empty((h, w), dtype=np.uint8)
    Cb = np.empty((ch, cw), dtype=np.uint8)
    Cr = np.empty((ch, cw), dtype=np.uint8)
    rc = load_host().rtxhost_synthetic_earth_ycbcr(seed, w, h, Y.ctypes.data_as(c_void_p), Cb.ctypes.data_as(c_void_p),
                                                   Cr.ctypes.data_as(c_void_p))
    if rc != RTX_OK:
        raise RtxError(rc, load_host().rtxhost_last_error().decode())
    return Y, Cb, Cr


def host_ycbcr_rgba(y: int, cb: int, cr: int):
    o = (c_uint32 * 4)()
    load_host().rtxhost_ycbcr_rgba(y, cb, cr, o)
    return tuple(o)


def desc_with_tree(desc_ptr, arr, n: int, root: int):
    """A copy of a scene description with another node table and root (same primitives and materials)."""
    d = desc_ptr.contents
    w = SceneDesc()
    for f, _ in SceneDesc._fields_:
        setattr(w, f, getattr(d, f))
    roots = (c_int32 * 1)(root)
    w.nodes = ctypes.cast(arr, POINTER(BvhNode))
    w.n_nodes = n
    w.n_roots = 1
    w.roots = ctypes.cast(roots, POINTER(c_int32))
    p = ctypes.pointer(w)
    p._keep = (arr, roots, desc_ptr)  # the arrays live as long as the pointer
    return p


def walk_near_region(desc_ptr, cam: Camera, flags: int = 0):
    """rtx_walk_near_region (host only): (box or None, active)."""
    box, act = (c_float * 6)(), c_uint32()
    for i in range(6):
        box[i] = float("nan")
    check(load().rtx_walk_near_region(desc_ptr, flags, ctypes.byref(cam), box, ctypes.byref(act)),
          "rtx_walk_near_region")
    vals = [float(v) for v in box]
    return (None if vals[0] != vals[0] else vals), bool(act.value)


def walk_near_desc(desc_ptr, cam: Camera, flags: int = 0):
    """rtx_walk_tree (host only) of the near tree for cam's octant, or None."""
    L = load()
    n, root = c_uint32(), c_int32()
    oc = camera_octant(cam) | RTX_TREE_NEAR
    check(L.rtx_walk_tree(desc_ptr, flags, oc, None, 0, ctypes.byref(n), ctypes.byref(root)), "rtx_walk_tree")
    if n.value == 0 and root.value == -1:
        return None
    arr = (BvhNode * max(n.value, 1))()
    check(L.rtx_walk_tree(desc_ptr, flags, oc, arr, n.value, ctypes.byref(n), ctypes.byref(root)), "rtx_walk_tree")
    return desc_with_tree(desc_ptr, arr, int(n.value), int(root.value))


def walk_tree_desc(desc_ptr, cam: Camera, flags: int = 0):
    """rtx_walk_tree (host only): the description of the tree a scene made from desc_ptr walks
    for cam's octant — desc_ptr itself when the scene would keep the caller's tree."""
    L = load()
    n, root = c_uint32(), c_int32()
    oc = camera_octant(cam)
    check(L.rtx_walk_tree(desc_ptr, flags, oc, None, 0, ctypes.byref(n), ctypes.byref(root)), "rtx_walk_tree")
    if n.value == 0 and root.value == -1:
        return desc_ptr
    arr = (BvhNode * max(n.value, 1))()
    check(L.rtx_walk_tree(desc_ptr, flags, oc, arr, n.value, ctypes.byref(n), ctypes.byref(root)), "rtx_walk_tree")
    return desc_with_tree(desc_ptr, arr, int(n.value), int(root.value))


def _skip_mask(call, where):
    import numpy as np
    n = c_uint32()
    check(call(None, 0, ctypes.byref(n)), where)
    m = np.zeros(max(n.value, 1), np.uint8)
    check(call(m.ctypes.data_as(c_void_p), n.value, ctypes.byref(n)), where)
    return m[: n.value]


def walk_skip(desc_ptr, cam: Camera, flags: int = 0):
    """rtx_walk_skip (host only): the skips a scene made from desc_ptr plans for a first render with cam."""
    return _skip_mask(lambda buf, cap, n: load().rtx_walk_skip(desc_ptr, flags, ctypes.byref(cam), buf, cap, n),
                      "rtx_walk_skip")


def node_skip(desc_ptr, skip):
    """Map a skip mask over node entries in visit order (emit's pre-order: a node, its left subtree,
    then its right, a one-element split's child once, a nested World's items in order) onto the
    description's node table, for the oracle's walk hooks.  A node met twice must agree."""
    import numpy as np
    d = desc_ptr.contents
    out = np.zeros(max(d.n_nodes, 1), np.uint8)
    seen = np.zeros(max(d.n_nodes, 1), np.uint8)
    k = 0
    for r in range(d.n_roots):
        stack = [d.roots[r]]
        while stack:
            ref = stack.pop()
            if ref >= 0:
                nd = d.nodes[ref]
                v = skip[k]
                k += 1
                if seen[ref] and out[ref] != v:
                    raise ValueError(f"node {ref} is walked twice with different skips")
                seen[ref], out[ref] = 1, v
                if nd.right != nd.left:
                    stack.append(nd.right)
                stack.append(nd.left)
            elif ((~ref) & 0xFFFFFFFF) >> 28 == RTX_PRIM_LIST:
                lst = d.lists[(~ref) & 0x0FFFFFFF]
                for i in reversed(range(lst.count)):
                    stack.append(d.list_refs[lst.first + i])
    if k != len(skip):
        raise ValueError(f"skip mask has {len(skip)} node entries, the walk {k}")
    return out[: d.n_nodes]


def camera_octant(cam: Camera) -> int:
    return int(load().rtx_camera_octant(ctypes.byref(cam)))


def region_rows(region: Region) -> int:
    return int(load().rtx_region_rows(ctypes.byref(region)))


def ppm_encode(rgb) -> bytes:
    import numpy as np
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = a.shape[0], a.shape[1]
    H = load_host()
    n = H.rtxhost_ppm_encode(a.ctypes.data_as(c_void_p), w, h, None, 0)
    buf = ctypes.create_string_buffer(int(n))
    H.rtxhost_ppm_encode(a.ctypes.data_as(c_void_p), w, h, buf, n)
    return buf.raw[: int(n)]


def encode_ppm_device(rgb_ptr: int, width: int, height: int, text_ptr: int, capacity: int, stream: int = 0) -> int:
    """rtx_encode_ppm_device on device buffers; returns the text length."""
    n = c_uint64()
    check(load().rtx_encode_ppm_device(rgb_ptr, width, height, text_ptr, capacity, ctypes.byref(n), stream),
          "rtx_encode_ppm_device")
    return n.value
