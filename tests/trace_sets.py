"""The scenes and ray sets of the ray-query tests (test_trace_ref.py, test_trace_gpu.py) — TEST INFRASTRUCTURE.

Small, seeded with numpy.random.RandomState, sizes fixed here.  Every set's references (trace_ref.scan in
float32 and float64, trace_ref.walk in float32) are computed once per session and never modified.

  primary     random_spheres seed 1: look-from (13, 2, 3) through a 64 x 36 grid of pixel centres, (0.001, inf)
  incoherent  same scene, 4096: origins uniform in the scene's box, uniform directions, lengths in [1e-3, 1e3]
  secondary   same scene, 2048 starting on sphere surfaces (the points of primary's hits), random hemisphere directions
  bounded     incoherent with tmax uniform in (0, 30) and tmin in {-1, 0, 0.001, 0.5}
  cornell     cornell_box, 2048 from inside the room (outside its two blocks), random directions
  quad_demo   quad_demo, 2048 from in front of the quads, random directions
  lists       test_random_scenes.build_scene(2, 40, 6) as a plain World (every primitive a root), 2048
  big         build_scene(3, 1500, 0): 2999 entries, past the 32 KB LDS copy, so the HBM path runs; 2048
  edges       a hand-made scene and hand-made rays (edge_rays)
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import oracle_binding as ob
import rtx
import trace_ref
from test_random_scenes import build_scene

F32 = np.float32
INF = np.float32(np.inf)
SETS = ("primary", "incoherent", "secondary", "bounded", "cornell", "quad_demo", "lists", "big", "edges")
SIZES = {"primary": 64 * 36, "incoherent": 4096, "secondary": 2048, "bounded": 4096, "cornell": 2048, "quad_demo": 2048,
         "lists": 2048, "big": 2048}
SEEDS = {"incoherent": 101, "secondary": 102, "bounded": 103, "cornell": 104, "quad_demo": 105, "lists": 106, "big": 107}


def make_rays(o, d, tmin, tmax) -> np.ndarray:
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = np.zeros(len(o), rtx.RAY_DTYPE)
    r["origin"], r["dir"] = o, d
    r["tmin"], r["tmax"] = np.broadcast_to(np.asarray(tmin, F32), len(o)), np.broadcast_to(np.asarray(tmax, F32), len(o))
    return r


def unit_dirs(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- scenes -----------------------------------------------------------------------------------------
class SceneCase:
    """A scene description (ctypes pointer, kept alive here) with its threaded entries and trace_ref.Scene."""

    def __init__(self, desc_ptr, keep=None):
        self.desc, self._keep = desc_ptr, keep
        self.entries = trace_ref.entries_of(desc_ptr)
        self.ref = trace_ref.Scene(self.entries, desc_ptr)


def _world_root(d: rtx.SceneDesc):
    """The same tables as a plain World: every primitive a root, spheres then quads (World.Hit's linear scan)."""
    refs = [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in range(d.n_spheres)] + \
           [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in range(d.n_quads)]
    arr = (ctypes.c_int32 * len(refs))(*refs)
    d._keep.append(arr)
    d.roots, d.n_roots = arr, len(refs)
    return d


def edges_desc():
    """Spheres 0 and 1 coincide (different materials), 3 lies inside 2, 4 stands alone; a hand-made tree whose
    walk meets them in the order 0, 1, 2, 3, 4."""
    spec = [((0, 0, 0), 1.0, 0), ((0, 0, 0), 1.0, 1), ((4, 0, 0), 2.0, 2), ((4.5, 0, 0), 0.5, 3), ((0, 5, 0), 1.0, 0)]
    spheres = (rtx.Sphere * len(spec))()
    for s, (c, r, m) in zip(spheres, spec):
        s.center[:], s.radius, s.material = c, r, m
    mats = (rtx.Material * 4)()
    tex = (rtx.Texture * 1)()
    tex[0].type = rtx.RTX_TEX_SOLID
    tex[0].even[:] = [0.5, 0.5, 0.5]
    for m in mats:
        m.type, m.texture = rtx.RTX_MAT_LAMBERTIAN, 0
    box = lambda i: (np.array(spec[i][0], F32) - F32(spec[i][1]), np.array(spec[i][0], F32) + F32(spec[i][1]))  # noqa: E731
    leaf = lambda i: (rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i),) + box(i)  # noqa: E731
    nodes = []

    def node(l, r):
        nd = rtx.BvhNode()
        lo, hi = np.minimum(l[1], r[1]), np.maximum(l[2], r[2])
        nd.bmin[:], nd.bmax[:] = [float(v) for v in lo], [float(v) for v in hi]
        nd.left, nd.right = l[0], r[0]
        nodes.append(nd)
        return (len(nodes) - 1, lo, hi)

    n01 = node(leaf(0), leaf(1))
    n23 = node(leaf(2), leaf(3))
    n0123 = node(n01, n23)
    root = node(n0123, leaf(4))
    d = rtx.SceneDesc()
    arr = (rtx.BvhNode * len(nodes))(*nodes)
    roots = (ctypes.c_int32 * 1)(root[0])
    d.nodes, d.n_nodes, d.roots, d.n_roots = arr, len(nodes), roots, 1
    d.spheres, d.n_spheres = spheres, len(spec)
    d.materials, d.n_materials, d.textures, d.n_textures = mats, 4, tex, 1
    d._keep = [arr, roots, spheres, mats, tex]
    return d


@functools.lru_cache(maxsize=None)
def scene(name: str) -> SceneCase:
    if name in ("random_spheres", "cornell_box", "quad_demo"):
        host = rtx.HostScene(name, seed=1)
        return SceneCase(host.desc, host)
    d = {"lists": lambda: _world_root(build_scene(2, 40, 6)), "big": lambda: build_scene(3, 1500, 0),
         "edges": edges_desc}[name]()
    return SceneCase(ctypes.pointer(d), d)


SCENE_OF = {"primary": "random_spheres", "incoherent": "random_spheres", "secondary": "random_spheres",
            "bounded": "random_spheres", "cornell": "cornell_box", "quad_demo": "quad_demo", "lists": "lists",
            "big": "big", "edges": "edges"}


# ---- rays -------------------------------------------------------------------------------------------
def primary_rays(width: int = 64, height: int = 36) -> np.ndarray:
    """Pixel centres of rand_spheres_camera (main.go:228-239) without lens or jitter: GetRay's
    pixel00 + du * i + dv * j - center (camera.go:266-284)."""
    cam = ob.rand_spheres_camera(width, 1, 1)
    assert cam.image_height == height
    p00, du, dv, cen = (np.array(list(v), F32) for v in (cam.pixel00, cam.pixel_du, cam.pixel_dv, cam.center))
    j, i = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pc = (p00[None] + du[None] * i.reshape(-1, 1).astype(F32)) + dv[None] * j.reshape(-1, 1).astype(F32)
    return make_rays(np.broadcast_to(cen, pc.shape), pc - cen[None], F32(0.001), INF)


def _scene_box(sc: trace_ref.Scene):
    """The box of the scene's non-huge spheres (a ground sphere of radius 1000 would make it the ground's)."""
    k = np.nonzero(sc.is_sphere & (sc.aw < 100))[0]
    return (sc.a3[k] - sc.aw[k, None]).min(axis=0), (sc.a3[k] + sc.aw[k, None]).max(axis=0)


def incoherent_rays(n: int, seed: int, sc: trace_ref.Scene) -> np.ndarray:
    rs = np.random.RandomState(seed)
    lo, hi = _scene_box(sc)
    o = rs.uniform(lo, hi, size=(n, 3))
    d = unit_dirs(rs, n) * (10.0 ** rs.uniform(-3, 3, size=(n, 1)))
    return make_rays(o, d, F32(0.001), INF)


def edge_rays(sc: trace_ref.Scene) -> np.ndarray:
    nan, inf = float("nan"), float("inf")
    R = []  # (origin, dir, tmin, tmax)
    # axis-parallel (two zero direction components): through the coincident pair, inside their slabs
    R += [((-5, 0, 0), (1, 0, 0), 0.001, inf), ((0, -5, 0), (0, 2, 0), 0.001, inf), ((0, 0, 7), (0, 0, -0.5), 0.001, inf)]
    # ... outside a slab (y = 1.5 misses the pair's box), and one zero component
    R += [((-5, 1.5, 0), (1, 0, 0), 0.001, inf), ((-5, 0.25, 0.5), (1, 0, -0.1), 0.001, inf)]
    # ... exactly on a box plane: y = 1 is the top of the pair's boxes, x = 6 the far side of sphere 2's (tangent rays)
    R += [((-5, 1, 0), (1, 0, 0), 0.001, inf), ((6, -5, 0), (0, 1, 0), 0.001, inf), ((-1, -5, 0), (0, 1, 0), 0.001, inf)]
    # a zero direction, outside and inside a sphere
    R += [((-5, 0, 0), (0, 0, 0), 0.001, inf), ((0, 0.5, 0), (0, 0, 0), 0.001, inf)]
    # NaN and infinite origin components, a NaN and an infinite direction component
    R += [((nan, 0, 0), (1, 0, 0), 0.001, inf), ((-5, nan, 0), (1, 0, 0), 0.001, inf), ((-inf, 0, 0), (1, 0, 0), 0.001, inf),
          ((0, inf, 0), (0, -1, 0), 0.001, inf), ((-5, 0, 0), (1, nan, 0), 0.001, inf), ((-5, 0, 0), (inf, 0, 0), 0.001, inf)]
    # the interval: tmin == tmax, tmin > tmax, tmax = +inf with tmin past the first root, tmin = -1 from behind
    R += [((-5, 0, 0), (1, 0, 0), 4.5, 4.5), ((-5, 0, 0), (1, 0, 0), 6.5, 4.5), ((-5, 0, 0), (1, 0, 0), 4.5, inf),
          ((5, 0, 0), (1, 0, 0), -1.0, inf), ((-5, 0, 0), (1, 0, 0), nan, inf), ((-5, 0, 0), (1, 0, 0), 0.001, nan),
          ((-5, 0, 0), (1, 0, 0), -inf, inf), ((-5, 0, 0), (1, 0, 0), 0.0, 5.0)]
    # an origin inside a sphere: inside the pair, inside 2 but outside 3, inside both 2 and 3
    R += [((0.25, 0.1, 0), (0.3, 1, 0.2), 0.001, inf), ((3, 0.5, 0), (1, 0, 0), 0.001, inf), ((4.5, 0.1, 0), (0, 1, 1), 0.001, inf)]
    # through 2 and 3 from outside, and the lone sphere 4
    R += [((10, 0.1, 0.1), (-1, 0, 0), 0.001, inf), ((0, 10, 0.2), (0, -1, 0), 0.001, inf)]
    rays = make_rays([r[0] for r in R], [r[1] for r in R], [r[2] for r in R], [r[3] for r in R])
    # tmax exactly equal to a root: the first three rays again, each stopped AT the root it finds (a miss of that
    # sphere, Interval.In is strict), and one float32 past it (the hit again)
    first = trace_ref.scan(sc, rays[:3], F32)
    assert first.mask.all()
    at = rays[:3].copy()
    at["tmax"] = first.t
    past = rays[:3].copy()
    past["tmax"] = np.nextafter(first.t, INF)
    return np.concatenate([rays, at, past])


class RaySet:
    def __init__(self, name: str, rays: np.ndarray):
        self.name, self.rays = name, rays
        self.scene = scene(SCENE_OF[name])

    @functools.cached_property
    def scan32(self):
        return trace_ref.scan(self.scene.ref, self.rays, np.float32)

    @functools.cached_property
    def scan64(self):
        return trace_ref.scan(self.scene.ref, self.rays, np.float64)

    @functools.cached_property
    def walk32(self):
        return trace_ref.walk(self.scene.ref, self.rays, np.float32)

    @functools.cached_property
    def kept(self):
        return trace_ref.kept(self.scan32, self.scan64)


@functools.lru_cache(maxsize=None)
def ray_set(name: str) -> RaySet:
    sc = scene(SCENE_OF[name])
    if name == "primary":
        return RaySet(name, primary_rays())
    if name == "edges":
        return RaySet(name, edge_rays(sc.ref))
    n, rs = SIZES[name], np.random.RandomState(SEEDS[name])
    if name == "incoherent":
        return RaySet(name, incoherent_rays(n, SEEDS[name], sc.ref))
    if name == "bounded":
        rays = incoherent_rays(n, SEEDS["incoherent"], sc.ref).copy()
        rays["tmax"] = rs.uniform(0, 30, n)
        rays["tmin"] = np.array([-1, 0, 0.001, 0.5], F32)[rs.randint(0, 4, n)]
        return RaySet(name, rays)
    if name == "secondary":
        prim = ray_set("primary")
        h = prim.scan32
        src = np.nonzero(h.mask)[0][rs.randint(0, int(h.mask.sum()), n)]
        d = unit_dirs(rs, n)
        nrm = h.normal[src].astype(np.float64)
        d = np.where((d * nrm).sum(axis=1, keepdims=True) < 0, -d, d)  # the hemisphere about the hit's normal
        return RaySet(name, make_rays(h.point[src], d, F32(0.001), INF))
    if name == "cornell":  # inside the room (0, 555)^3, outside the two blocks (scenes.cpp: Box(...))
        blocks = [((130, 0, 65), (295, 165, 230)), ((265, 0, 295), (430, 330, 460))]
        o = np.zeros((0, 3))
        while len(o) < n:
            c = rs.uniform(1, 554, size=(n, 3))
            inside = np.zeros(n, bool)
            for lo, hi in blocks:
                inside |= ((c >= np.array(lo) - 1) & (c <= np.array(hi) + 1)).all(axis=1)
            o = np.concatenate([o, c[~inside]])
        return RaySet(name, make_rays(o[:n], unit_dirs(rs, n), F32(0.001), INF))
    if name == "quad_demo":  # in front of the quads (they span z in [0, 5]; the camera stands at z = 9)
        o = rs.uniform((-2.5, -2.5, 2.0), (2.5, 2.5, 9.0), size=(n, 3))
        return RaySet(name, make_rays(o, unit_dirs(rs, n), F32(0.001), INF))
    o = rs.uniform(-8, 8, size=(n, 3))  # lists, big: build_scene's spheres lie in (-6, 6)^3 over a ground at y = -1
    return RaySet(name, make_rays(o, unit_dirs(rs, n) * (10.0 ** rs.uniform(-2, 2, size=(n, 1))), F32(0.001), INF))
