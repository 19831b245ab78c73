"""Hand-made scene descriptions for the direct-light tests — TEST INFRASTRUCTURE.

A World of a few spheres and quads (a World root: the caller's order is the walk's), built with NewQuad's float32
arithmetic (hittables.go:149-165), and the analytic scenes whose pixels have closed forms: a Lambertian floor under
one or two quad lights or a sphere light, seen by a pinhole straight above it."""
from __future__ import annotations

import ctypes
import math

import numpy as np

import oracle_binding as ob
import rtx

F32, F64 = np.float32, np.float64


def _cross(l, r):  # vec3.go:129-135, float32
    return np.array([l[1] * r[2] - l[2] * r[1], l[2] * r[0] - l[0] * r[2], l[0] * r[1] - l[1] * r[0]], F32)


def _dot(l, r):  # vec3.go:137-139
    return F32(F32(F32(l[0] * r[0]) + F32(l[1] * r[1])) + F32(l[2] * r[2]))


def quad(Q, u, v, material: int) -> rtx.Quad:
    """NewQuad (hittables.go:149-165) in float32."""
    Q, u, v = (np.array(x, F32) for x in (Q, u, v))
    q = rtx.Quad()
    old = np.seterr(all="ignore")
    try:
        n = _cross(u, v)
        inv_len = F32(F32(1) / F32(np.sqrt(F64(_dot(n, n)))))
        norm = np.array([n[0] * inv_len, n[1] * inv_len, n[2] * inv_len], F32)
        inv = F32(F32(1) / _dot(n, n))
        q.q[:], q.u[:], q.v[:] = list(Q), list(u), list(v)
        q.w[:] = [float(n[0] * inv), float(n[1] * inv), float(n[2] * inv)]
        q.normal[:] = [float(x) for x in norm]
        q.d = float(_dot(norm, Q))
    finally:
        np.seterr(**old)
    q.material = material
    return q


def sphere(center, radius: float, material: int) -> rtx.Sphere:
    s = rtx.Sphere()
    s.center[:] = list(center)
    s.radius = radius
    s.material = material
    return s


def solid(r, g, b) -> rtx.Texture:
    t = rtx.Texture()
    t.type = rtx.RTX_TEX_SOLID
    t.even[:] = [r, g, b]
    return t


def checker(scale, even, odd) -> rtx.Texture:
    t = rtx.Texture()
    t.type, t.scale = rtx.RTX_TEX_CHECKERED, scale
    t.even[:], t.odd[:] = list(even), list(odd)
    return t


def material(kind: int, texture: int = 0, albedo=(0, 0, 0), fuzz: float = 0.0, ior: float = 0.0) -> rtx.Material:
    m = rtx.Material()
    m.type, m.texture, m.fuzz, m.ior = kind, texture, fuzz, ior
    m.albedo[:] = list(albedo)
    return m


def world(spheres, quads, materials, textures, roots=None):
    """(pointer to the description, the tables it points into).  roots: refs, default every primitive: spheres, then
    quads (a World root)."""
    if roots is None:
        roots = [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in range(len(spheres))] + \
                [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in range(len(quads))]
    keep = dict(spheres=(rtx.Sphere * max(1, len(spheres)))(*spheres), quads=(rtx.Quad * max(1, len(quads)))(*quads),
                mats=(rtx.Material * len(materials))(*materials), texs=(rtx.Texture * len(textures))(*textures),
                roots=(ctypes.c_int32 * len(roots))(*roots))
    d = rtx.SceneDesc()
    d.n_roots, d.roots = len(roots), keep["roots"]
    d.n_spheres, d.spheres = len(spheres), keep["spheres"]
    d.n_quads, d.quads = len(quads), keep["quads"]
    d.n_materials, d.materials = len(materials), keep["mats"]
    d.n_textures, d.textures = len(textures), keep["texs"]
    p = ctypes.pointer(d)
    p._keep = keep
    return p


LAMB, METAL, LIGHT = rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_METAL, rtx.RTX_MAT_DIFFUSE_LIGHT


def five():
    """Five primitives: a sphere light, a Metal sphere, a checkered floor, a quad light facing down and a red occluder
    quad between the quad light and the floor.  Emitter table: the sphere (light 0), then the quad (light 1)."""
    texs = [checker(0.7, (0.8, 0.8, 0.7), (0.2, 0.3, 0.4)), solid(5, 4, 3), solid(2, 3, 4), solid(0.7, 0.1, 0.1)]
    mats = [material(LAMB, 0), material(LIGHT, 1), material(LIGHT, 2), material(LAMB, 3),
            material(METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.1)]
    spheres = [sphere((2, 1, 0), 0.5, 2), sphere((-2, 0.7, 0), 0.7, 4)]
    quads = [quad((-4, 0, -4), (0, 0, 8), (8, 0, 0), 0),          # floor, normal +y
             quad((-1, 3, -1), (2, 0, 0), (0, 0, 2), 1),          # light, normal -y
             quad((-0.5, 1.5, -0.5), (1, 0, 0), (0, 0, 1), 3)]    # occluder
    desc = world(spheres, quads, mats, texs)
    cam = ob.camera(F32(16.0 / 9.0), 64, samples_per_pixel=1, max_depth=8, look_from=(0, 2.5, 7), look_at=(0, 0.6, 0),
                    fov_degrees=50, defocus_degrees=0, background=(0, 0, 0))
    return desc, cam


# ---- the analytic scenes ---------------------------------------------------------------------------------------
ALBEDO = (0.75, 0.5, 0.25)
EMIT = (4.0, 6.0, 8.0)
CAM_HEIGHT = 1.0


def floor_scene(kind: str):
    """A Lambertian floor y = 0 (albedo ALBEDO), black background, and
       'a': one 1 x 1 quad light at height 2;  'b': 'a' plus a 2 x 0.5 quad light at height 3;
       'c': one sphere light, radius 0.4, centre (0.3, 2.5, -0.2).
    Returns (description, camera 16 x 16, depth 2, straight down from height CAM_HEIGHT, lights) with lights a list
    of ('quad', x0, x1, z0, z1, h) / ('sphere', centre, r)."""
    texs, mats = [solid(*ALBEDO), solid(*EMIT)], [material(LAMB, 0), material(LIGHT, 1)]
    quads = [quad((-3, 0, -3), (0, 0, 6), (6, 0, 0), 0)]
    spheres, lights = [], []
    if kind in ("a", "b"):
        quads.append(quad((-0.5, 2, -0.5), (1, 0, 0), (0, 0, 1), 1))
        lights.append(("quad", -0.5, 0.5, -0.5, 0.5, 2.0))
    if kind == "b":
        quads.append(quad((-0.25, 3, -1.5), (2, 0, 0), (0, 0, 0.5), 1))
        lights.append(("quad", -0.25, 1.75, -1.5, -1.0, 3.0))
    if kind == "c":
        spheres.append(sphere((0.3, 2.5, -0.2), 0.4, 1))
        lights.append(("sphere", (0.3, 2.5, -0.2), 0.4))
    desc = world(spheres, quads, mats, texs)
    cam = ob.camera(F32(1.0), 16, samples_per_pixel=1, max_depth=2, look_from=(0, CAM_HEIGHT, 0), look_at=(0, 0, 0),
                    vup=(0, 0, -1), fov_degrees=40, defocus_degrees=0, background=(0, 0, 0))
    return desc, cam, lights


def footprints(cam):
    """The floor rectangle of every pixel of the pinhole camera above y = 0: arrays x0, x1, z0, z1 [H, W] (float64).
    The pixel's jitter is uniform over its square (camera.go:289-299) and the image plane is parallel to the floor, so
    a sample's floor point is uniform over the rectangle."""
    W, H = cam.image_width, cam.image_height
    c, p00 = np.array(list(cam.center), F64), np.array(list(cam.pixel00), F64)
    du, dv = np.array(list(cam.pixel_du), F64), np.array(list(cam.pixel_dv), F64)
    out = np.zeros((4, H, W))
    for y in range(H):
        for x in range(W):
            pts = []
            for ox, oy in ((-0.5, -0.5), (0.5, 0.5)):
                d = p00 + du * (x + ox) + dv * (y + oy) - c
                pts.append(c + d * (-c[1] / d[1]))
            out[:, y, x] = (min(pts[0][0], pts[1][0]), max(pts[0][0], pts[1][0]), min(pts[0][2], pts[1][2]),
                            max(pts[0][2], pts[1][2]))
    return out


def _corner_factor(a, b, c):
    """Form factor from a differential element to a parallel a x b rectangle at distance c whose corner lies on the
    element's normal (the standard configuration factor; a, b >= 0)."""
    A, B = a / c, b / c
    return (A / np.sqrt(1 + A * A) * np.arctan(B / np.sqrt(1 + A * A)) +
            B / np.sqrt(1 + B * B) * np.arctan(A / np.sqrt(1 + B * B))) / (2 * math.pi)


def form_factor(light, x, z):
    """F of the floor point(s) (x, 0, z) to the light, closed form (float64): the share of a cosine-distributed
    bounce that reaches it = integral of cos cos' / (pi d^2) over its visible area."""
    x, z = np.asarray(x, F64), np.asarray(z, F64)
    if light[0] == "quad":
        _, x0, x1, z0, z1, h = light
        f = 0.0
        for xe, sx in ((x1, 1.0), (x0, -1.0)):  # signed corner rectangles
            for ze, sz in ((z1, 1.0), (z0, -1.0)):
                a, b = xe - x, ze - z
                f = f + sx * sz * np.sign(a) * np.sign(b) * _corner_factor(np.abs(a), np.abs(b), h)
        return f
    _, c, r = light
    dx, dy, dz = c[0] - x, c[1], c[2] - z
    d2 = dx * dx + dy * dy + dz * dz
    return (r * r / d2) * (dy / np.sqrt(d2))  # (r / d)^2 cos(theta): the sphere lies wholly above the floor's horizon


def quadrature(light, x, z, n: int = 400):
    """The same integral by a midpoint rule over the light's surface, float64, for one floor point."""
    if light[0] == "quad":
        _, x0, x1, z0, z1, h = light
        xs = x0 + (np.arange(n) + 0.5) * (x1 - x0) / n
        zs = z0 + (np.arange(n) + 0.5) * (z1 - z0) / n
        X, Z = np.meshgrid(xs, zs)
        d2 = (X - x) ** 2 + h * h + (Z - z) ** 2
        return float(np.sum(h * h / (math.pi * d2 * d2)) * (x1 - x0) * (z1 - z0) / (n * n))
    _, c, r = light
    th = (np.arange(n) + 0.5) * math.pi / n
    ph = (np.arange(2 * n) + 0.5) * math.pi / n
    T, P = np.meshgrid(th, ph)
    nl = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], -1)
    q = np.array(c) + r * nl
    w = q - np.array([x, 0.0, z])
    d2 = np.sum(w * w, -1)
    cs = w[..., 1] / np.sqrt(d2)
    cl = -np.sum(nl * w, -1) / np.sqrt(d2)  # only the side facing the point is seen
    dA = r * r * np.sin(T) * (math.pi / n) ** 2
    return float(np.sum(np.where((cl > 0) & (cs > 0), cs * cl / (math.pi * d2), 0.0) * dA))


def expected_image(cam, lights, grid: int = 8):
    """Per pixel, the mean over its footprint (grid x grid midpoints) of sum over lights of F, times ALBEDO * EMIT:
    [H, W, 3] float64, and the plain F image [H, W]."""
    x0, x1, z0, z1 = footprints(cam)
    f = np.zeros(x0.shape)
    for i in range(grid):
        for j in range(grid):
            x = x0 + (i + 0.5) * (x1 - x0) / grid
            z = z0 + (j + 0.5) * (z1 - z0) / grid
            for l in lights:
                f += form_factor(l, x, z)
    f /= grid * grid
    return f[..., None] * (np.array(ALBEDO) * np.array(EMIT))[None, None, :], f


def g_max(cam, lights):
    """Per pixel, an upper bound from the geometry alone of the block's g over the footprint and every light:
    g = cs * cl * area * L / (pi d^2) with cs, cl <= 1; over a parallel quad at height h, cs = cl = h / d, so
    g <= h^2 * area * L / (pi d_min^4), d_min^2 = h^2 + the squared horizontal distance from the footprint to the
    rectangle; for a sphere d >= D_min - r, D_min the least distance from the footprint to the centre."""
    x0, x1, z0, z1 = footprints(cam)
    L = len(lights)
    out = np.zeros(x0.shape)
    gap = lambda lo, hi, a, b: np.maximum(0.0, np.maximum(a - hi, lo - b))  # noqa: E731  between [lo, hi] and [a, b]
    for l in lights:
        if l[0] == "quad":
            _, a0, a1, b0, b1, h = l
            rho2 = gap(x0, x1, a0, a1) ** 2 + gap(z0, z1, b0, b1) ** 2
            g = h * h * (a1 - a0) * (b1 - b0) * L / (math.pi * (h * h + rho2) ** 2)
        else:
            _, c, r = l
            rho2 = gap(x0, x1, c[0], c[0]) ** 2 + gap(z0, z1, c[2], c[2]) ** 2
            D = np.sqrt(c[1] ** 2 + rho2)
            g = 4 * math.pi * r * r * L / (math.pi * (D - r) ** 2)
        out = np.maximum(out, g)
    return out
