"""One small scene per dispatch class of the block kernels — TEST INFRASTRUCTURE (test_block_census.py).

trace_rays, guide_images, direct_lights and direct_paths are compiled per QUADS x FIXED x NOISE (the scene holds quads;
its layout fits the workgroup's LDS copy; it has a Perlin texture).  block_scene(quads, big, noise) is the smallest scene
of a class that still has emitters (direct_lights and direct_paths have nothing to do without), blocked and free shadow
rays, and misses:

  always   an emitting sphere
  quads    a Lambertian floor quad and an emitting quad, as test_direct_gpu.memory_scene has them; without quads a
           ground sphere takes their place (radius 100: its horizon lies inside the window, so camera rays still miss)
  the grid g x g small Lambertian spheres under a median-split tree of its own, floating between the floor and the
           lights.  g = 8: about 130 entries, the LDS copy.  g = 32: 1024 spheres + 1023 nodes and the roots, the fewest
           of a square grid past big_scenes.LIMIT = 2047 entries, read from HBM.
  noise    the floor (the ground sphere) and one light (the quad; without quads the sphere) carry simple_light_demo's
           Perlin texture and tables, taken as test_direct_gpu.test_noise_textured_emitter_and_albedo takes them

The camera is direct_scenes.five()'s, the window 24 x 13: 312 records, a partial last wave."""
from __future__ import annotations

import functools
import itertools

import numpy as np

import direct_scenes as ds
import rtx

F32 = np.float32
WINDOW = (20, 12, 24, 13)  # x0, y0, width, height of the 64 x 36 image: 312 records
SPP, DEPTH = 3, 8
EXTENT = 6.2  # the grid's side, centre to centre (memory_scene: 32 spheres 0.2 apart)
GRID_Y = 0.9
CLASSES = list(itertools.product((False, True), repeat=3))  # (quads, big, noise)


def label(quads: bool, big: bool, noise: bool) -> str:
    return ("quads" if quads else "spheres") + ("-hbm" if big else "-lds") + ("-noise" if noise else "")


class BlockScene:
    """desc: the description (keeps its tables alive); cam: the camera (a copy per scene); grid: the sphere-table indices
    of the grid; noise_mats: the materials whose texture is the Perlin one."""

    def __init__(self, name, quads, big, noise, desc, cam, grid, noise_mats, keep):
        self.name, self.quads, self.big, self.noise = name, quads, big, noise
        self.desc, self.cam, self.grid, self.noise_mats, self.keep = desc, cam, grid, noise_mats, keep

    def region(self) -> rtx.Region:
        return rtx.Region(*WINDOW, 0, 1)

    def camera(self, spp: int = SPP, depth: int = DEPTH):
        cam = rtx.Camera.from_buffer_copy(self.cam)
        cam.samples_per_pixel, cam.max_depth = spp, depth
        return cam


@functools.lru_cache(maxsize=None)
def block_scene(quads: bool, big: bool, noise: bool) -> BlockScene:
    """Built once, shared, never modified."""
    g = 32 if big else 8
    step = F32(EXTENT / (g - 1))
    radius = F32(step / 4)  # g = 32: 0.05, memory_scene's
    texs = [ds.solid(0.8, 0.7, 0.6), ds.solid(6, 5, 4), ds.solid(3, 4, 5), ds.solid(0.2, 0.5, 0.3)]
    FLOOR, QUAD_LIGHT, SPHERE_LIGHT, GRID = 0, 1, 2, 3  # materials
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1), ds.material(ds.LIGHT, 2), ds.material(ds.LAMB, 3)]
    keep, noise_mats = None, ()
    if noise:
        keep = rtx.HostScene("simple_light_demo", 1)
        hd = keep.desc.contents
        src = next(hd.textures[i] for i in range(hd.n_textures) if hd.textures[i].type == rtx.RTX_TEX_NOISE)
        tex = rtx.Texture()
        tex.type, tex.scale, tex.texel_offset = src.type, src.scale, src.texel_offset
        texs.append(tex)
        noise_mats = (FLOOR, QUAD_LIGHT if quads else SPHERE_LIGHT)
        for m in noise_mats:
            mats[m].texture = len(texs) - 1
    spheres = [ds.sphere((2, 1.6, 0), 0.5, SPHERE_LIGHT)]
    qs = []
    if quads:
        qs = [ds.quad((-4, 0, -4), (0, 0, 8), (8, 0, 0), FLOOR),        # floor, normal +y
              ds.quad((-1, 3, -1), (2, 0, 0), (0, 0, 2), QUAD_LIGHT)]   # light, normal -y
    else:
        spheres.append(ds.sphere((0, -100, 0), 100.0, FLOOR))
    first = len(spheres)
    xz = (np.arange(g, dtype=F32) - F32((g - 1) / 2)) * step
    centres = np.stack([np.repeat(xz, g), np.full(g * g, GRID_Y, F32), np.tile(xz, g)], axis=1).astype(F32)
    spheres += [ds.sphere([float(v) for v in c], float(radius), GRID) for c in centres]
    nodes = []

    def build(idx, axis):  # a median split, x and z in turn; the grid's sphere k is sphere first + k of the table
        if len(idx) == 1:
            return rtx.ref_prim(rtx.RTX_PRIM_SPHERE, first + int(idx[0]))
        me = len(nodes)
        nodes.append(rtx.BvhNode())
        idx = idx[np.argsort(centres[idx, axis], kind="stable")]
        left, right = build(idx[: len(idx) // 2], 2 - axis), build(idx[len(idx) // 2:], 2 - axis)
        n = nodes[me]
        n.bmin[:] = [float(v) for v in centres[idx].min(axis=0) - radius]
        n.bmax[:] = [float(v) for v in centres[idx].max(axis=0) + radius]
        n.left, n.right = left, right
        return me

    root = build(np.arange(g * g), 0)
    roots = [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in range(len(qs))] + \
            [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in range(first)] + [root]
    desc = ds.world(spheres, qs, mats, texs, roots=roots)
    desc._keep["nodes"] = (rtx.BvhNode * len(nodes))(*nodes)
    desc.contents.n_nodes, desc.contents.nodes = len(nodes), desc._keep["nodes"]
    if noise:
        desc.contents.texels, desc.contents.n_texels = hd.texels, hd.n_texels
    cam = ds.five()[1]
    cam.samples_per_pixel, cam.max_depth = SPP, DEPTH
    return BlockScene(label(quads, big, noise), quads, big, noise, desc, cam, np.arange(first, first + g * g), noise_mats, keep)


def window_rays(cam, win=WINDOW) -> np.ndarray:
    """The window's pixel-centre camera rays (big_scenes.window_rays)."""
    import big_scenes

    return big_scenes.window_rays(cam, win)


def first_hit_kinds(s: BlockScene, prim, material) -> dict:
    """Per kind, the mask of the hit records (prim, material words; RTX_HIT_NONE: a miss) of that kind."""
    prim, material = np.asarray(prim, np.uint32), np.asarray(material, np.uint32)
    hit = prim != rtx.RTX_HIT_NONE
    sphere = hit & (prim >> 28 == rtx.RTX_PRIM_SPHERE)
    return {"miss": ~hit, "grid": sphere & np.isin(prim & 0x0FFFFFFF, s.grid), "sphere": sphere,
            "quad": hit & (prim >> 28 == rtx.RTX_PRIM_QUAD), "noise": hit & np.isin(material, s.noise_mats),
            "noise_lambertian": hit & np.isin(material, s.noise_mats[:1])}
