"""The cases both test_ref64.py (oracle, CPU) and test_ref64_gpu.py (kernel) hold to tests/ref64.py.

TEST INFRASTRUCTURE.  Small shapes where the code can be wrong, not the workload's: images ragged
against the 8x8 tile, hand-made camera tables (one kind with defocus, one without), hand-made
scene tables with a World-list root (spheres first, then quads: the index order ref64 scans), and the two
mixed scenes of tests/big_scenes.py, whose layouts are past the LDS limit (a tree with nested Worlds).

A case is (name, desc pointer, camera, seed, window, spp, cap): `cap` is the share of samples
that may be left out — 1 % on the probes (one primitive, or one scatterer in an emissive sphere),
3 % on the multi-bounce scenes.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import ref64
import rtx

F = np.float32
CAP_PROBE, CAP_SCENE = 0.01, 0.03
W, H = 36, 20  # ragged against the 8 x 8 tile


def f3(a):
    return [float(F(x)) for x in a]


# ---- hand-made tables -------------------------------------------------------------------------
class Tables:
    def __init__(self):
        self.spheres, self.quads, self.mats, self.texs, self.texels = [], [], [], [], []

    def solid(self, rgb):
        t = rtx.Texture()
        t.type = rtx.RTX_TEX_SOLID
        t.even[:] = f3(rgb)
        self.texs.append(t)
        return len(self.texs) - 1

    def checker(self, scale, even, odd):
        t = rtx.Texture()
        t.type, t.scale = rtx.RTX_TEX_CHECKERED, float(F(scale))
        t.even[:], t.odd[:] = f3(even), f3(odd)
        self.texs.append(t)
        return len(self.texs) - 1

    def image(self, w, h, step_r, step_g, border):
        """Texel (i, j) = (i * step_r, j * step_g, a mix) / 65535: neighbours differ by >= 1e-3."""
        assert min(step_r, step_g) / 65535.0 >= 1e-3 and (w - 1) * step_r <= 65535 and (h - 1) * step_g <= 65535
        t = rtx.Texture()
        t.type, t.width, t.height, t.texel_offset = rtx.RTX_TEX_IMAGE, w, h, len(self.texels)
        for j in range(h):
            for i in range(w):
                self.texels += [(i * step_r) | ((j * step_g) << 16), ((i * 977 + j * 3571) % 65536) | (0xFFFF << 16)]
        self.texels += [border[0] | (border[1] << 16), border[2] | (0xFFFF << 16)]
        self.texs.append(t)
        return len(self.texs) - 1

    def noise(self, scale, seed):
        """A Perlin table built here: 256 gradients in [-1, 1), three permutations (rtx.h RTX_TEX_NOISE)."""
        rng = np.random.default_rng(seed)
        t = rtx.Texture()
        t.type, t.scale, t.texel_offset = rtx.RTX_TEX_NOISE, float(F(scale)), len(self.texels)
        self.texels += rng.uniform(-1, 1, 768).astype(F).view(np.uint32).tolist()
        for _ in range(3):
            self.texels += rng.permutation(256).astype(np.uint32).tolist()
        self.texs.append(t)
        return len(self.texs) - 1

    def material(self, kind, texture=0, albedo=(0, 0, 0), fuzz=0.0, ior=0.0):
        m = rtx.Material()
        m.type, m.texture, m.fuzz, m.ior = kind, texture, float(F(fuzz)), float(F(ior))
        m.albedo[:] = f3(albedo)
        self.mats.append(m)
        return len(self.mats) - 1

    def light(self, texture):
        return self.material(rtx.RTX_MAT_DIFFUSE_LIGHT, texture)

    def sphere(self, center, radius, mat):
        s = rtx.Sphere()
        s.center[:], s.radius, s.material = f3(center), float(F(radius)), mat
        self.spheres.append(s)

    def quad(self, Q, u, v, mat):
        """NewQuad (hittables.go:149-165) in float32: normal = Unit(u x v), d = normal . Q, w = n / (n . n)."""
        Q, u, v = (np.array(a, F) for a in (Q, u, v))
        with np.errstate(all="ignore"):
            n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F)
            nn = F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            normal = n * F(F(1) / np.sqrt(nn))
            d = F(F(normal[0] * Q[0] + normal[1] * Q[1]) + normal[2] * Q[2])
            w = n * F(F(1) / nn)
        q = rtx.Quad()
        q.q[:], q.u[:], q.v[:], q.w[:], q.normal[:] = f3(Q), f3(u), f3(v), f3(w), f3(normal)
        q.d, q.material = float(d), mat
        self.quads.append(q)

    def degenerate_quad(self, mat):
        """u || v: a NaN normal, which no ray may hit (hittables.go:170-178)."""
        self.quad((-0.3, -0.2, 0.4), (0.5, 0.25, -0.125), (1.0, 0.5, -0.25), mat)
        assert np.isnan(self.quads[-1].normal[0])

    def desc(self):
        d = rtx.SceneDesc()
        keep = []

        def arr(ctype, items):
            a = (ctype * max(1, len(items)))(*items)
            keep.append(a)
            return a

        roots = [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in range(len(self.spheres))]
        roots += [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in range(len(self.quads))]
        d.nodes, d.n_nodes = arr(rtx.BvhNode, []), 0
        d.roots, d.n_roots = arr(ctypes.c_int32, roots), len(roots)
        d.spheres, d.n_spheres = arr(rtx.Sphere, self.spheres), len(self.spheres)
        d.quads, d.n_quads = arr(rtx.Quad, self.quads), len(self.quads)
        d.materials, d.n_materials = arr(rtx.Material, self.mats), len(self.mats)
        d.textures, d.n_textures = arr(rtx.Texture, self.texs), len(self.texs)
        if len(self.texels) % 2:
            self.texels.append(0)
        d.texels, d.n_texels = arr(ctypes.c_uint32, self.texels), len(self.texels)
        p = ctypes.pointer(d)
        p._keep = (d, keep)
        return p


def look(origin, target, span, depth, w=W, h=H, focus=1.0, defocus=0.0, spp=1, up=(0, 1, 0)):
    """A camera table made by hand: pixel spacing span / w at distance `focus` along the view."""
    o, t = np.array(origin, np.float64), np.array(target, np.float64)
    fwd = (t - o) / np.linalg.norm(t - o)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    du, dv = right * (span / w), -upv * (span / w)
    p00 = o + fwd * focus - right * (span / 2) + upv * (span * h / w / 2) + 0.5 * (du + dv)
    cam = rtx.Camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, spp, depth
    cam.center[:], cam.pixel00[:], cam.pixel_du[:], cam.pixel_dv[:] = f3(o), f3(p00), f3(du), f3(dv)
    cam.background[:] = [0.25, 0.5, 0.75]
    if defocus > 0:
        cam.defocus_angle = 0.02
        cam.defocus_disk_u[:], cam.defocus_disk_v[:] = f3(right * defocus), f3(upv * defocus)
    return cam


BORDER = (65535, 1111, 60000)  # the border texel's own colour


def image_light(t, w=37, h=19):
    return t.light(t.image(w, h, 65535 // (w - 1) // 4 * 4, 65535 // (h - 1) // 4 * 4, BORDER))


# ---- primary-hit probes: max_depth 1, the pixel is the texture at the first hit -----------------
def sphere_image(radius, center, origin, target, span, defocus=0.0, focus=1.0):
    t = Tables()
    t.sphere(center, radius, image_light(t))
    return t.desc(), look(origin, target, span, 1, defocus=defocus, focus=focus)


def quad_scene(light_of, origin, target, span, defocus=0.0):
    """A non-rectangular parallelogram (u . v != 0, |u| != |v|) and a degenerate quad in front of it."""
    t = Tables()
    m = light_of(t)
    t.degenerate_quad(m)
    t.quad((-1.5, -0.8, 0.3), (2.6, 0.4, -0.7), (0.9, 1.7, 0.5), m)
    return t.desc(), look(origin, target, span, 1, defocus=defocus)


def checker_light(t):
    return t.light(t.checker(0.37, (0.125, 0.5, 0.875), (0.75, 0.25, 0.0625)))


def checker_ground():
    t = Tables()
    t.sphere((0, -1000, 0), 1000.0, checker_light(t))
    return t.desc(), look((0.3, 1.2, 0.4), (-3.0, 0.0, -2.0), 1.6, 1)


NOISE_SIZE = 0.05  # the noise probes' size: see noise_scene


def noise_scene(scale_sphere, scale_quad, offset, tables=None):
    """A sphere and, in front of its left part, a quad, each with its own noise texture.  Turb sums
    seven octaves of the hit point times `scale` and GetTexture takes sin(z + 10 * turb), so a
    float32 rounding of the hit point reaches the colour about 10 * 7 * scale / 2 times larger.
    The window therefore shows the middle of the sphere only (no grazing hits, whose roots cancel)
    and the probe is NOISE_SIZE across with its camera as close: that keeps the reference's own
    spread below the 1e-5 a case may have.
    tables: (texels, scale) of a Perlin table to use instead of one made here."""
    t = Tables()
    k = NOISE_SIZE
    if tables is None:
        ts, tq = t.noise(scale_sphere, 11), t.noise(scale_quad, 12)
    else:
        words, scale = tables
        ts = t.noise(scale, 0)
        t.texels[t.texs[ts].texel_offset: t.texs[ts].texel_offset + 1536] = [int(x) for x in words]
        tq = ts
    off = np.array(offset, np.float64)
    t.sphere(off, 0.8 * k, t.light(ts))
    t.quad(np.array([-0.037, -0.045, 1.579]) * k + off, np.array([0.25, 0.03, -0.08]) * k,
           np.array([-0.03, 0.5, 0.06]) * k, t.light(tq))
    return t.desc(), look(np.array([0.5, 0.4, 3.0]) * k + off, off, 0.3 * k, 1, focus=k)


def host_noise_scene():
    """The Perlin table the host mirror lays out for simple_light_demo (256 gradients, permX, permY,
    permZ: rtx.h) and its scale, read from the desc, on the noise probe's geometry."""
    s = rtx.HostScene("simple_light_demo", 1)
    d = s.desc.contents
    tex = [d.textures[i] for i in range(d.n_textures) if d.textures[i].type == rtx.RTX_TEX_NOISE][0]
    words = np.ctypeslib.as_array(d.texels, shape=(d.n_texels,))[tex.texel_offset: tex.texel_offset + 1536].copy()
    return noise_scene(0, 0, (0.011, -0.007, 0.004), tables=(words, float(tex.scale)))


def closest_hit_scene():
    """Six overlapping spheres and quads, each its own solid emitter, and a small patch coincident
    with one quad (its pixels tie and are left out)."""
    t = Tables()
    lights = [t.light(t.solid(c)) for c in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1),
                                            (0.5, 0.5, 0.5))]
    t.sphere((0.0, 0.0, 0.0), 0.7, lights[0])
    t.sphere((0.5, 0.2, 0.3), 0.6, lights[1])
    t.sphere((-0.4, -0.1, 0.5), 0.5, lights[2])
    t.quad((-1.2, -0.9, 0.2), (2.4, 0.3, 0.2), (0.2, 1.8, -0.3), lights[3])
    t.quad((-1.0, -0.2, 1.0), (2.0, 0.0, -1.6), (0.0, 0.9, 0.1), lights[4])
    t.quad((-0.9, 0.6, -0.5), (1.9, -0.2, 1.5), (0.1, -1.3, 0.4), lights[5])
    # the coincident patch: a small part of the first quad, in exactly its plane (a pixel or two wide)
    Q, u, v = (np.array(a, np.float64) for a in ((-1.2, -0.9, 0.2), (2.4, 0.3, 0.2), (0.2, 1.8, -0.3)))
    t.quad(Q + 0.22 * u + 0.9 * v, u / 16, v / 20, lights[6])
    first, patch = t.quads[0], t.quads[3]
    patch.normal[:], patch.d = list(first.normal), first.d
    return t.desc(), look((0.3, 0.4, 3.0), (-0.1, 0.1, 0), 1.0, 1)


# ---- one- and two-bounce probes: a scatterer inside an r = 50 emissive image sphere ------------
def env(t):
    t.sphere((0.0, 0.0, 0.0), 50.0, image_light(t, 64, 32))


def metal_scene():
    t = Tables()
    env(t)
    t.sphere((-0.9, 0.1, 0.0), 0.6, t.material(rtx.RTX_MAT_METAL, albedo=(0.8, 0.6, 0.9), fuzz=0.0))
    t.sphere((0.9, 0.1, 0.0), 0.6, t.material(rtx.RTX_MAT_METAL, albedo=(0.7, 0.9, 0.5), fuzz=0.6))
    t.quad((-1.6, -0.9, -0.8), (1.5, 0.0, 0.5), (0.2, 0.6, -0.1), t.material(rtx.RTX_MAT_METAL, albedo=(0.9, 0.8, 0.7)))
    t.quad((0.2, -0.9, -0.3), (1.5, 0.1, -0.5), (-0.2, 0.6, -0.1),
           t.material(rtx.RTX_MAT_METAL, albedo=(0.6, 0.7, 0.8), fuzz=0.6))
    return t.desc(), look((0.1, 0.3, 3.0), (0, -0.2, 0), 1.2, 3)


def glass_sphere_scene():
    t = Tables()
    env(t)
    t.sphere((0.0, 0.0, 0.0), 1.0, t.material(rtx.RTX_MAT_DIELECTRIC, ior=1.5))
    return t.desc(), look((0.2, 0.3, 2.6), (0, 0, 0), 2.2, 4, defocus=0.02, focus=2.6)


def glass_inside_scene():
    """The camera inside the glass, off centre: back-face hits only, total internal reflection past
    41.8 degrees (a ray that entered a sphere from outside never meets it), exits below."""
    t = Tables()
    env(t)
    t.sphere((0.0, 0.0, 0.0), 1.0, t.material(rtx.RTX_MAT_DIELECTRIC, ior=1.5))
    return t.desc(), look((0.8, 0.3, 0.2), (-1.0, 0.2, 0.9), 2.4, 4)


def glass_sheet_scene(front: bool):
    t = Tables()
    env(t)
    t.quad((-1.5, -1.0, 0.2), (3.0, 0.3, -0.5), (0.3, 2.0, 0.4), t.material(rtx.RTX_MAT_DIELECTRIC, ior=2.4))
    return t.desc(), look((0.4, 0.2, 3.0) if front else (-0.3, 0.1, -3.0), (0, 0, 0), 1.1, 3)


def glass_critical_scene():
    """The sheet's back face seen at its critical angle (sin = 1 / 2.4) through a window a few
    float32 ulps wide: rays that can still refract in both precisions while the float32
    1 - |perp|^2 of refract (vec3.go:219) comes out below zero, where only math.Abs keeps the
    square root real."""
    t = Tables()
    env(t)
    t.quad((-1.5, -1.0, 0.2), (3.0, 0.3, -0.5), (0.3, 2.0, 0.4), t.material(rtx.RTX_MAT_DIELECTRIC, ior=2.4))
    q = t.quads[0]
    n = np.array(list(q.normal), np.float64)
    tangent = np.cross(n, [0.0, 1.0, 0.0])
    tangent /= np.linalg.norm(tangent)
    sin_c = 1.0 / float(F(2.4))
    d = np.sqrt(1.0 - sin_c * sin_c) * n + sin_c * tangent  # along the outward normal: a back-face hit
    hit = np.array([-1.5, -1.0, 0.2]) + 0.5 * np.array([3.0, 0.3, -0.5]) + 0.5 * np.array([0.3, 2.0, 0.4])
    return t.desc(), look(hit - 2.0 * d, hit, CRITICAL_SPAN, 3)


CRITICAL_SPAN = 5e-5  # the window at one unit of distance: about 200 float32 ulps of the direction


def lambert_scene():
    t = Tables()
    env(t)
    tex = t.checker(0.37, (0.9, 0.6, 0.3), (0.2, 0.4, 0.8))
    t.sphere((-0.7, 0.0, 0.0), 0.7, t.material(rtx.RTX_MAT_LAMBERTIAN, tex))
    t.quad((0.1, -0.8, -0.4), (1.5, 0.2, 0.6), (-0.1, 1.5, 0.3), t.material(rtx.RTX_MAT_LAMBERTIAN, tex))
    return t.desc(), look((0.2, 0.2, 3.0), (0, 0, 0), 0.9, 3)


# ---- scenes ------------------------------------------------------------------------------------
def random_scene(seed, n_spheres, n_quads, axis_aligned):
    import test_random_scenes as trs

    d = trs.build_scene(seed, n_spheres, n_quads)
    p = ctypes.pointer(d)
    p._keep = d
    return p, trs.camera(seed, 64, 36, 1, axis_aligned)


def host_scene(name, width, depth, spp=1):
    s = rtx.HostScene(name, 1)
    return s.desc, s.camera(width=width, spp=spp, depth=depth)


def big_scene(case):
    """The mixed scenes past the LDS limit (tests/big_scenes.py): the kernels that read the scene from HBM."""
    import big_scenes

    return big_scenes.ref64_scene(case)


def _case(name, scene, seed, window=None, spp=1, cap=CAP_PROBE):
    return name, scene, seed, window, spp, cap


CASES = [
    # primary-hit probes
    _case("sphere_image_outside", lambda: sphere_image(1.0, (0, 0, 0), (1.4, 1.1, 2.4), (0, 0, 0), 0.9, focus=1.0), 11),
    _case("sphere_image_inside", lambda: sphere_image(1.0, (0, 0, 0), (0.2, 0.1, -0.3), (0.5, 0.2, 1), 2.5,
                                                      defocus=0.05), 12),
    _case("sphere_image_tmin_r0.01", lambda: sphere_image(0.01, (0, 0, 0), f3(np.array([0.6, 0.48, 0.64]) * 0.0105),
                                                          (0, 0, 0), 2.0), 13),
    _case("sphere_image_tmin_r1000", lambda: sphere_image(1000.0, (0, -1000, 0), (0.0, 5e-4, 0.0), (0.6, -0.45, 0.7),
                                                          2.0), 14),
    _case("quad_image_front", lambda: quad_scene(image_light, (0.3, 0.5, 3.0), (0, 0.2, 0), 1.3), 15),
    _case("quad_image_back", lambda: quad_scene(image_light, (-0.4, 0.2, -3.0), (0, 0.2, 0), 1.3, defocus=0.04), 16),
    _case("quad_image_grazing", lambda: quad_scene(image_light, (2.9, 0.55, -0.62), (0.2, 0.3, 0.15), 0.9), 17),
    _case("checker_sphere_r1000", lambda: checker_ground(), 18),
    _case("checker_quad", lambda: quad_scene(checker_light, (0.3, 0.5, 3.0), (0, 0.2, 0), 1.3), 19),
    _case("noise_sphere4_quad0.5", lambda: noise_scene(4.0, 0.5, (0.0, 0.0, 0.0)), 20),
    _case("noise_negative_sphere0.5_quad4", lambda: noise_scene(0.5, 4.0, (-0.26, -0.17, -0.39)), 21),
    _case("noise_host_tables", host_noise_scene, 23),
    _case("closest_hit_order", closest_hit_scene, 22),
    # bounce probes
    _case("metal_sphere_quad_fuzz", metal_scene, 31),
    _case("dielectric_sphere", glass_sphere_scene, 32),
    _case("dielectric_sphere_inside", glass_inside_scene, 36),
    _case("dielectric_sheet_front", lambda: glass_sheet_scene(True), 33),
    _case("dielectric_sheet_back", lambda: glass_sheet_scene(False), 34),
    _case("dielectric_critical_angle", glass_critical_scene, 38),
    _case("lambertian_checker", lambert_scene, 35),
    # scenes
    _case("random_scene_2", lambda: random_scene(2, 40, 14, False), 2, cap=CAP_SCENE),
    _case("random_scene_3_axis", lambda: random_scene(3, 36, 18, True), 3, cap=CAP_SCENE),
    _case("random_scene_5", lambda: random_scene(5, 1, 21, False), 5, cap=CAP_SCENE),
    _case("random_spheres_64x36", lambda: host_scene("random_spheres", 64, 50), 2, cap=CAP_SCENE),
    _case("random_spheres_24x13x4", lambda: host_scene("random_spheres", 24, 50, spp=4), 2, spp=4, cap=CAP_SCENE),
    _case("cornell_box_window", lambda: host_scene("cornell_box", 600, 50), 41, window=(300, 340, 24, 12),
          cap=CAP_SCENE),
    _case("earth_window", lambda: host_scene("earth", 400, 50), 43, window=(188, 106, 24, 12), cap=CAP_SCENE),
    # scenes past the LDS limit (tests/big_scenes.py): a tree with nested Worlds, read from HBM
    _case("big_mixed", lambda: big_scene("big_mixed"), 5, cap=CAP_SCENE),
    _case("big_mixed_noise", lambda: big_scene("big_mixed_noise"), 5, cap=CAP_SCENE),
]
NAMES = [c[0] for c in CASES]
NO_LDS_CASES = ("dielectric_sphere", "random_scene_2")  # the two cases the GPU file also runs from global memory


class Built:
    def __init__(self, name):
        _, make, self.seed, window, self.spp, self.cap = CASES[NAMES.index(name)]
        self.name = name
        self.desc, self.cam = make()
        self.window = window or (0, 0, self.cam.image_width, self.cam.image_height)
        self.region = rtx.Region(*self.window, 0, 1)
        self.ref = ref64.Case(self.desc, self.cam, self.seed, self.window, self.spp)

    def report(self) -> str:
        r = self.ref
        return (f"{self.name}: left out {100 * r.left_out:.2f} % (cap {100 * self.cap:.0f} %), "
                f"spread {r.spread:.3g}, tol {r.tol:.3g}")


@functools.lru_cache(maxsize=None)
def built(name) -> Built:
    """The scene, the camera and ref64's two runs of a case: computed once, shared, never modified."""
    return Built(name)
