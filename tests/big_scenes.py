"""Hand-made scenes just past the LDS limit — TEST INFRASTRUCTURE (test_big_scenes.py, test_big_scenes_gpu.py).

A walk layout of more than LIMIT entries does not fit the LDS copy ((n + 1) * 16 > LDS_B, rtx_layout.h): pack_layout
stores it hot-first and the render reads it from HBM, through an LDS cache of its hot entries (at most CACHE_MAX of
them) unless the scene has a Perlin texture.  The only such scene the other tests render is stress_100k (equal spheres,
no quad, no emitter, no image, no list, no tie); these are small seeded ones with everything else in them:

  mixed        spheres (radii from 1e-3 up, over an r = 999 ground) and quads (every 7th degenerate) of every material
               kind, solid / checkered / image textures (the image with its border texel), under a median-split tree
               two of whose subtrees are nested Worlds (RTX_PRIM_LIST): one a flat list of primitives, one a list of
               two subtrees and a list
  mixed_noise  mixed with a Perlin-textured Lambertian and a Perlin emitter on every 6th primitive.  (Their scales are
               small: a reflection off a sphere of radius 1e-3 magnifies a float32 rounding of the hit point a thousand
               times, the noise texture is continuous in the next hit point, and ref64's case may spread 1e-5 at most.)
  mixed_world  mixed's primitives as a plain World: every primitive a root, no nodes
  big_ties     test_ties.py's scene grown past the limit: a grid of small spheres, three big ones and exact copies of
               the three with other materials, under a NewBVH-shaped tree
  split_tier   a sphere grid under a tree whose every leaf is a one-element split: the guarded tree keeps the caller's
               leaf nodes (3 n - 1 entries), the near tree has none (2 n - 1), so the one fits the LDS copy and the
               other does not

The sizes.  mixed_world must itself be past the limit, and a World has one entry per primitive, so mixed holds
N_SPHERES + N_QUADS = 2060 primitives (2048 is the least; the few more keep the counts round).  Its tree then has
4085 entries (about 3770 in the collapsed walk): more than the cache holds, so a default render reads both from the cache and from HBM.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import oracle_binding as ob
import ref64_cases as rc
import rtx
import test_random_scenes as trs
import test_ties

F = np.float32
LIMIT = 2047  # the most entries of a layout in the LDS copy: (n + 1) * 16 <= LDS_B = 32768 (rtx_layout.h)
CACHE_MAX = 2560  # HOT_ENTRIES_MAX (rtx_device.h): the most entries of the LDS cache
N_SPHERES, N_QUADS = 2030, 30
CAM_W, CAM_H = 40, 24
WINDOW = (2, 1, 37, 22)  # ragged against the 8 x 8 tile on both sides
SEED = 4  # of the mixed scenes
R_EXP = (-3.0, -0.3)  # radii 10^U: from 1e-3 to 0.5, small enough that the quads and the far side show through
NOISE_SCALE = 2.0 ** -11  # Perlin scales this small keep ref64's float32 and float64 colours within 1e-5 (see REF64)
NOISE_EVERY = 6  # mixed_noise: every 6th primitive takes a Perlin material


class Big:
    """desc: the scene description (a ctypes pointer that keeps its tables alive); nested: the Hit.prim codes
    ((type << 28) | index) of the primitives below a nested World."""

    def __init__(self, name, desc, nested=()):
        self.name, self.desc, self.nested = name, desc, np.array(sorted(nested), np.uint32)


def _prim_code(ref: int) -> int:
    return (~ref) & 0xFFFFFFFF


def _tables(seed: int, noise: bool):
    """The primitive, material and texture tables of the mixed scenes and each primitive's (ref, bmin, bmax)."""
    rng = np.random.default_rng(seed)
    t = rc.Tables()
    solid = t.solid((0.7, 0.3, 0.2))
    checker = t.checker(0.37, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9))
    image = t.image(9, 5, 65535 // 8 // 4 * 4, 65535 // 4 // 4 * 4, rc.BORDER)
    of_kind = [solid, checker, image]
    for k in range(16):  # every kind four times; the textured kinds go through solid, checkered and image
        kind = [rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_METAL, rtx.RTX_MAT_DIELECTRIC, rtx.RTX_MAT_DIFFUSE_LIGHT][k % 4]
        tex = of_kind[(k // 4 + (k % 4 == 3)) % 3] if kind in (rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT) else 0
        t.material(kind, tex, albedo=rng.uniform(0.1, 1.0, 3), fuzz=rng.uniform(0, 1), ior=rng.uniform(1.0, 2.5))
    ground = t.material(rtx.RTX_MAT_LAMBERTIAN, checker)
    prims = []
    for i in range(N_SPHERES):
        c = rng.uniform(-6, 6, 3).astype(F)
        r = F(10.0 ** rng.uniform(*R_EXP))
        m = int(rng.integers(0, 16))
        if i == 0:
            c, r, m = np.array([0, -1000, 0], F), F(999.0), ground  # a ground the camera may stand on
        t.sphere(c, r, m)
        prims.append((rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i), c - r, c + r))
    for i in range(N_QUADS):
        Q = rng.uniform(-5, 5, 3).astype(F)
        u = rng.uniform(-3, 3, 3).astype(F)
        v = rng.uniform(-3, 3, 3).astype(F) if i % 7 else u * F(2)  # every 7th degenerate (u || v)
        t.quad(Q, u, v, int(rng.integers(0, 16)))
        assert bool(np.isnan(t.quads[-1].normal[0])) == (i % 7 == 0)
        pts = np.array([Q, Q + u, Q + v, Q + u + v], F)
        prims.append((rtx.ref_prim(rtx.RTX_PRIM_QUAD, i), pts.min(0) - F(1e-3), pts.max(0) + F(1e-3)))
    if noise:  # after every draw of the geometry: mixed_noise has mixed's primitives
        lam = t.material(rtx.RTX_MAT_LAMBERTIAN, t.noise(NOISE_SCALE, 41))
        lit = t.light(t.noise(NOISE_SCALE / 2, 42))
        for k, (ref, _, _) in enumerate(prims[1:]):
            if k % NOISE_EVERY == 0:
                code = _prim_code(ref)
                table = t.quads if code >> 28 == rtx.RTX_PRIM_QUAD else t.spheres
                table[code & 0x0FFFFFFF].material = lam if (k // NOISE_EVERY) % 2 else lit
    return t, prims, rng


def _desc(t: rc.Tables, nodes, roots, lists=(), list_refs=()):
    d = rtx.SceneDesc()
    keep = []

    def arr(ctype, items):
        a = (ctype * max(1, len(items)))(*items)
        keep.append(a)
        return a

    d.nodes, d.n_nodes = arr(rtx.BvhNode, nodes), len(nodes)
    d.roots, d.n_roots = arr(ctypes.c_int32, roots), len(roots)
    d.spheres, d.n_spheres = arr(rtx.Sphere, t.spheres), len(t.spheres)
    d.quads, d.n_quads = arr(rtx.Quad, t.quads), len(t.quads)
    d.materials, d.n_materials = arr(rtx.Material, t.mats), len(t.mats)
    d.textures, d.n_textures = arr(rtx.Texture, t.texs), len(t.texs)
    texels = list(t.texels) + [0] * (len(t.texels) % 2)
    d.texels, d.n_texels = arr(ctypes.c_uint32, texels), len(texels)
    d.lists, d.n_lists = arr(rtx.List, [rtx.List(a, b) for a, b in lists]), len(lists)
    d.list_refs, d.n_list_refs = arr(ctypes.c_int32, list(list_refs)), len(list_refs)
    p = ctypes.pointer(d)
    p._keep = (d, keep)
    return p


FLAT_AT, DEEP_AT = (1, 0, 1, 0, 1, 0), (0, 1)  # the two subtrees that become Worlds: paths from the root (0 = left)


def _mixed(name: str, noise: bool, world: bool) -> Big:
    t, prims, rng = _tables(SEED, noise)
    if world:
        return Big(name, _desc(t, [], [ref for ref, _, _ in prims]))
    nodes, lists, list_refs, nested = [], [], [], set()

    def new_list(items):
        lists.append((len(list_refs), len(items)))
        list_refs.extend(items)
        return rtx.ref_prim(rtx.RTX_PRIM_LIST, len(lists) - 1)

    def build(items, path):
        if len(items) == 1:
            return items[0]
        axis = int(rng.integers(0, 3))
        items = sorted(items, key=lambda it: float(it[1][axis]))
        mid = len(items) // 2
        lo, hi = np.min([it[1] for it in items], axis=0), np.max([it[2] for it in items], axis=0)
        if path == FLAT_AT:  # a World of this subtree's primitives, scanned one after another
            nested.update(_prim_code(it[0]) for it in items)
            return new_list([it[0] for it in items]), lo, hi
        if path == DEEP_AT:  # a World of the two halves' subtrees and a World of two primitives
            nested.update(_prim_code(it[0]) for it in items)
            inner = new_list([it[0] for it in items[:2]])
            a, b = build(items[2:mid], path + (0,)), build(items[mid:], path + (1,))
            return new_list([a[0], inner, b[0]]), lo, hi
        me = len(nodes)
        nodes.append(None)
        (lref, lmin, lmax), (rref, rmin, rmax) = build(items[:mid], path + (0,)), build(items[mid:], path + (1,))
        nd = rtx.BvhNode()
        nd.bmin[:], nd.bmax[:] = rc.f3(np.minimum(lmin, rmin)), rc.f3(np.maximum(lmax, rmax))
        nd.left, nd.right = lref, rref
        nodes[me] = nd
        return me, np.minimum(lmin, rmin), np.maximum(lmax, rmax)

    root, _, _ = build(prims, ())
    assert len(lists) == 3
    return Big(name, _desc(t, nodes, [root], lists, list_refs), nested)


def grid_spheres(n_side: int, spacing: float, radius: float, seed: int, n_mats: int):
    """randSpheres' shape (main.go:187-226) at another size: a ground sphere, a jittered grid of small spheres and
    three big ones — [(centre, radius, material)]."""
    rng = np.random.default_rng(seed)
    out = [((0.0, -1000.0, 0.0), 1000.0, 0)]
    half = n_side // 2
    for a in range(-half, n_side - half):
        for b in range(-half, n_side - half):
            c = (float(F(a * spacing + 0.6 * spacing * rng.random())), float(F(radius)),
                 float(F(b * spacing + 0.6 * spacing * rng.random())))
            out.append((c, float(F(radius)), 1 + int(rng.integers(0, n_mats - 1))))
    return out


def _host():
    return rtx.HostScene("random_spheres", 1)


def _big_ties() -> Big:
    """A grid of 40 x 40 small spheres less those under randSpheres' three big ones, the three, and each of them again
    with the next one's material: 1570 spheres."""
    host = _host()
    d = host.desc.contents
    own = [(tuple(d.spheres[i].center), d.spheres[i].radius, d.spheres[i].material) for i in range(d.n_spheres)]
    big = [s for s in own if abs(s[1] - 1.0) < 1e-6]
    assert len(big) == 3
    spheres = [s for s in grid_spheres(40, 0.6, 0.125, 3, d.n_materials)
               if all(np.hypot(s[0][0] - b[0][0], s[0][2] - b[0][2]) > 1.2 for b in big) or s[1] > 1]
    spheres += big + [(b[0], b[1], big[(k + 1) % 3][2]) for k, b in enumerate(big)]
    # sorted from the reversed index order: of two exact copies the reference walk meets the HIGHER index first, so a
    # walk that broke ties by sphere index instead of by rank word would keep the other material
    b = Big("big_ties", test_ties.newbvh_desc(spheres, None, host.desc, order=reversed(range(len(spheres)))))
    b.host = host
    return b


def _split_tier() -> Big:
    host = _host()
    spheres = grid_spheres(SPLIT_SIDE, 0.9, 0.2, 5, SPLIT_MATS)
    spheres += [((0.0, 1.0, 0.0), 1.0, 1), ((-4.0, 1.0, 0.0), 1.0, 2), ((4.0, 1.0, 0.0), 1.0, 3)]
    b = Big("split_tier", test_ties.newbvh_desc(spheres, None, host.desc, leaf=1))
    b.desc.contents.n_materials = SPLIT_MATS  # the first few of randSpheres' table: it goes into the LDS copy's gap
    b.host = host
    return b


SPLIT_SIDE = 31  # 961 + 4 spheres: a near tree of 2 n - 1 = 1929 entries, a guarded tree of 3 n - 1 = 2894
SPLIT_MATS = 16

MAKERS = {"mixed": lambda: _mixed("mixed", False, False), "mixed_noise": lambda: _mixed("mixed_noise", True, False),
          "mixed_world": lambda: _mixed("mixed_world", False, True), "big_ties": _big_ties, "split_tier": _split_tier}
NAMES = list(MAKERS)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Big:
    """Built once, shared, never modified."""
    return MAKERS[name]()


def camera(name: str, axis_aligned: bool = False, spp: int = 4, w: int = CAM_W, h: int = CAM_H):
    """test_random_scenes.camera (a random place, or the axis-aligned one whose centre rays have zero direction
    components) for the mixed scenes; main.go's randSpheres camera for big_ties and one looking
    from above to the horizon for split_tier, both inside the near region."""
    if name.startswith("mixed"):
        return trs.camera(CAM_SEED, w, h, spp, axis_aligned)
    if name == "split_tier":  # from above, towards the horizon: the far ground lies outside the near region
        cam = ob.camera(F(16.0) / F(9.0), w, samples_per_pixel=spp, max_depth=12, look_from=(13, 14, 3),
                        look_at=(-30, -4, -6), fov_degrees=50, defocus_degrees=0.6, focus_dist=10, background=(0.7, 0.8, 1.0))
    else:
        cam = scene(name).host.camera(width=w, spp=spp, depth=12)
    assert cam.image_height <= h
    return cam


CAM_SEED = 8  # even: no defocus on the random camera (ref64 keeps more); the axis-aligned one is seedless


def window(name: str):
    """(x0, y0, width, height) the GPU tests render of camera(name)."""
    if name.startswith("mixed"):
        return WINDOW
    cam = camera(name)
    return (1, 0, cam.image_width - 3, cam.image_height)  # 16:9 at 40 wide: 22 rows


def window_rays(cam, win) -> np.ndarray:
    """The window's pixel-centre rays without lens or jitter (GetRay's pixel00 + du * i + dv * j - center)."""
    x0, y0, w, h = win
    p00, du, dv, cen = (np.array(list(v), F) for v in (cam.pixel00, cam.pixel_du, cam.pixel_dv, cam.center))
    j, i = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    pc = (p00[None] + du[None] * i.reshape(-1, 1).astype(F)) + dv[None] * j.reshape(-1, 1).astype(F)
    rays = np.zeros(len(pc), rtx.RAY_DTYPE)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = cen[None], pc - cen[None], F(0.001), F(np.inf)
    return rays


def first_hit_kinds(b: Big, hits) -> dict:
    """Per kind, the mask of rays whose first hit (trace_ref.Hits) is of that kind."""
    d = b.desc.contents
    hit = hits.mask
    mat = np.where(hit, hits.material, 0)
    mtype = np.array([d.materials[i].type for i in range(d.n_materials)])[mat]
    textured = np.isin(mtype, (rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT))
    ttype = np.array([d.textures[d.materials[i].texture].type for i in range(d.n_materials)])[mat]
    return {"sphere": hit & (hits.prim >> 28 == rtx.RTX_PRIM_SPHERE), "quad": hit & (hits.prim >> 28 == rtx.RTX_PRIM_QUAD),
            "emitter": hit & (mtype == rtx.RTX_MAT_DIFFUSE_LIGHT), "image": hit & textured & (ttype == rtx.RTX_TEX_IMAGE),
            "noise": hit & textured & (ttype == rtx.RTX_TEX_NOISE), "nested": hit & np.isin(hits.prim, b.nested)}


# The two cases of ref64_cases.CASES: (scene, axis-aligned camera, max_depth) at ref64_cases' 36 x 20, 1 spp.
REF64 = {"big_mixed": ("mixed", False, 6), "big_mixed_noise": ("mixed_noise", True, 6)}


def ref64_scene(case: str):
    name, axis_aligned, depth = REF64[case]
    cam = camera(name, axis_aligned, spp=1, w=rc.W, h=rc.H)
    cam.max_depth = depth
    return scene(name).desc, cam
