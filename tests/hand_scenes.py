"""Hand-made sphere scenes and cameras for the render tests (test infrastructure): a scene description of spheres under
a median-split tree, a material list, a camera given by its pixel grid, and a ring of Lambertian, Metal and glass spheres
around the camera that can be scaled and moved as a whole."""
import ctypes

import numpy as np

import rtx

F = np.float32


def f3(a):
    return [float(F(x)) for x in a]


class Materials(list):
    def add(self, kind, albedo=(1.0, 1.0, 1.0), fuzz=0.0, ior=1.0):
        m = rtx.Material()
        m.type, m.texture, m.fuzz, m.ior = kind, 0, float(F(fuzz)), float(F(ior))
        m.albedo[:] = f3(albedo)
        self.append(m)
        return len(self) - 1


def sphere_desc(balls, mats):
    """A scene description of the spheres (centre, radius, material index) under a median-split tree."""
    tex = rtx.Texture()
    tex.type = rtx.RTX_TEX_SOLID
    tex.even[:] = [0.5, 0.5, 0.5]
    spheres, prims = [], []
    for i, (c, r, mat) in enumerate(balls):
        s = rtx.Sphere()
        c, r = np.array(c, F), F(r)
        s.center[:] = f3(c)
        s.radius = float(r)
        s.material = mat
        spheres.append(s)
        prims.append((rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i), c - r, c + r))
    nodes = []

    def build(items, depth):
        if len(items) == 1:
            return items[0]
        items = sorted(items, key=lambda it: float(it[1][(0, 2, 1)[depth % 3]]))
        mid = len(items) // 2
        me = len(nodes)
        nodes.append(None)
        lref, lmin, lmax = build(items[:mid], depth + 1)
        rref, rmin, rmax = build(items[mid:], depth + 1)
        bmin, bmax = np.minimum(lmin, rmin), np.maximum(lmax, rmax)
        nd = rtx.BvhNode()
        nd.bmin[:] = f3(bmin)
        nd.bmax[:] = f3(bmax)
        nd.left, nd.right = lref, rref
        nodes[me] = nd
        return me, bmin, bmax

    root, _, _ = build(prims, 0)
    d = rtx.SceneDesc()
    keep = []

    def arr(ctype, items):
        a = (ctype * max(1, len(items)))(*items)
        keep.append(a)
        return a

    d.nodes, d.n_nodes = arr(rtx.BvhNode, nodes), len(nodes)
    d.roots, d.n_roots = arr(ctypes.c_int32, [root]), 1
    d.spheres, d.n_spheres = arr(rtx.Sphere, spheres), len(spheres)
    d.quads, d.n_quads = arr(rtx.Quad, []), 0
    d.materials, d.n_materials = arr(rtx.Material, mats), len(mats)
    d.textures, d.n_textures = arr(rtx.Texture, [tex]), 1
    d._keep = keep
    return d


def plain_camera(w, h, spp, depth, origin, p00, du, dv):
    cam = rtx.Camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, spp, depth
    cam.center[:] = f3(origin)
    cam.pixel00[:] = f3(p00)
    cam.pixel_du[:] = f3(du)
    cam.pixel_dv[:] = f3(dv)
    cam.background[:] = [0.6, 0.7, 0.9]
    return cam


def ring_materials():
    mats = Materials()
    kinds = [mats.add(rtx.RTX_MAT_LAMBERTIAN, (0.7, 0.4, 0.3)), mats.add(rtx.RTX_MAT_METAL, (0.8, 0.8, 0.7), fuzz=0.2),
             mats.add(rtx.RTX_MAT_DIELECTRIC, ior=1.5)]
    return mats, kinds


def ring_balls(kinds, scale=1.0, centre=(0.0, 0.0, 0.0)):
    """Eight spheres of radius 1.6 on a circle of radius 5 in the plane y = 0 (every third a little above or below),
    Lambertian, Metal and glass in turn; all of it times `scale` about `centre`."""
    c0 = np.array(centre, np.float64)
    return [(c0 + scale * np.array([5.0 * np.cos(a), 0.25 * (i % 3 - 1), 5.0 * np.sin(a)]), 1.6 * scale, kinds[i % 3])
            for i, a in enumerate(np.arange(8) * (np.pi / 4) + 0.2)]


def ring_camera(w, h, spp, depth, scale=1.0, centre=(0.0, 0.0, 0.0), dist=4.0, step=0.25):
    """A camera at `centre` looking down -z at a pixel grid `dist` away with pixels `step` apart (times `scale`): at
    32 x 18 its rays fan +-45 degrees sideways and +-29 up and down, onto the ring's spheres."""
    c0 = np.array(centre, np.float64)
    p00 = c0 + scale * np.array([-step * (w // 2), step * (h // 2), -dist])
    return plain_camera(w, h, spp, depth, c0, p00, (scale * step, 0, 0), (0, -scale * step, 0))
