"""The shading phase of the render kernels: the own-box test, coop_scatter, shade, defer_far, the claim
loop, the pool fill and trav_begin as the timed and the counting kernel run them.

Every case goes through parity.check_scene: both kernels' frames bit-identical to the oracle's, and the counting
kernel's counters — hits and rng_draws among them — equal to the oracle's.  The cases:
  - the random spheres at 64 x 36 x 8 through the tiered kernels; the launch line shows that the drain ran,
  - a window of that camera that leaves 3 valid lanes per wave, and shard 1 of 3 of another window,
  - the Cornell box at 32 x 32 x 8 (quads; nearly every lane of a phase hit something),
  - a hand-made scene of mostly glass spheres at 48 x 27 x 16, depth 50: batches with many Dielectric lanes.  Three of
    the glass spheres hold a Lambertian core, whose scattered rays reach the glass from inside at any angle.  The
    oracle shows on the CPU that the seed produces total internal reflection (hence back-face hits: only a back face has
    eta > 1) and the drawn reflectance test: a sample's draws and hits at max_depth d minus those at d - 1 are the
    draws of its d-th segment's hit, which are 0 for a Dielectric that reflects totally, 1 for one that draws its
    reflectance test and at least 3 for a Lambertian or a Metal (the scene has no light).
  - the general side of the two merged votes: camera rays with a direction component of exactly 0 (trav_begin's four
    divisions), and a scene so small that every camera ray's squared length is below 2^-96 (unit()'s sqrt and division).
"""
import ctypes

import numpy as np
import pytest

import oracle_binding as ob
import rtx
from hand_scenes import Materials, plain_camera, sphere_desc
from parity import check_scene, gpu_region

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 1
DEPTH = 8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def spheres(built):
    return rtx.HostScene("random_spheres", seed=1)


@pytest.fixture(scope="module")
def dev_spheres(spheres, torch_cuda):
    return rtx.DeviceScene(spheres.desc)


def check_counters(st, cnt):
    assert st.rng_draws == cnt["rng_draws"] and st.rng_draws > 0
    assert st.hits == cnt["hits"] and st.hits > 0


def test_random_spheres_drain(torch_cuda, spheres, dev_spheres, monkeypatch, capfd):
    cam = spheres.camera(width=64, spp=8, depth=DEPTH)
    assert (cam.image_width, cam.image_height) == (64, 36)
    reg = rtx.Region(0, 0, 64, 36, 0, 1)
    monkeypatch.setenv("RTX_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    _, st0 = gpu_region(torch_cuda, dev_spheres, cam, SEED, reg, counters=False)
    launch = capfd.readouterr().err
    assert "drain 1" in launch, launch
    assert st0.walk_layout & rtx.RTX_LAYOUT_TIERED
    monkeypatch.delenv("RTX_DEBUG_LAUNCH")
    _, st, cnt = check_scene(torch_cuda, dev_spheres, spheres.desc, cam, SEED, reg)
    check_counters(st, cnt)


@pytest.mark.parametrize("case", [("few-lanes-3x9", 5, 3, 3, 9, 0, 1), ("rank1of3", 7, 2, 24, 20, 1, 3)],
                         ids=lambda c: c[0])
def test_random_spheres_windows(torch_cuda, spheres, dev_spheres, case):
    _, x0, y0, w, h, rank, world = case
    cam = spheres.camera(width=64, spp=8, depth=DEPTH)
    reg = rtx.Region(x0, y0, w, h, rank, world)
    assert rtx.region_rows(reg) > 0
    _, st, cnt = check_scene(torch_cuda, dev_spheres, spheres.desc, cam, SEED, reg)
    check_counters(st, cnt)


def test_cornell_box(torch_cuda, built):
    s = rtx.HostScene("cornell_box", 1)
    dev = rtx.DeviceScene(s.desc)
    cam = s.camera(width=32, spp=8, depth=DEPTH)
    assert (cam.image_width, cam.image_height) == (32, 32)
    _, st, cnt = check_scene(torch_cuda, dev, s.desc, cam, SEED, rtx.Region(0, 0, 32, 32, 0, 1))
    check_counters(st, cnt)


# ---- the glass scene ------------------------------------------------------------------------------------------------
def glass_scene():
    """A Lambertian ground, a 5 x 3 field of glass spheres (ior 1.5, every fourth 2.4), three larger glass spheres with
    a Lambertian core off their centre, one Metal sphere."""
    mats = Materials()
    ground = mats.add(rtx.RTX_MAT_LAMBERTIAN, (0.5, 0.5, 0.5))
    glass15 = mats.add(rtx.RTX_MAT_DIELECTRIC, ior=1.5)
    glass24 = mats.add(rtx.RTX_MAT_DIELECTRIC, ior=2.4)
    core = mats.add(rtx.RTX_MAT_LAMBERTIAN, (0.8, 0.3, 0.2))
    metal = mats.add(rtx.RTX_MAT_METAL, (0.7, 0.6, 0.5), fuzz=0.1)
    balls = [((0.0, -1000.0, 0.0), 1000.0, ground)]
    k = 0
    for ix in range(5):
        for iz in range(3):
            balls.append(((-2.4 + 1.2 * ix, 0.45, -1.2 + 1.2 * iz + 0.3 * (ix & 1)), 0.45, glass24 if k % 4 == 3 else glass15))
            k += 1
    for j, (x, z, mat) in enumerate([(-1.6, 2.2, glass15), (0.0, 2.6, glass24), (1.6, 2.2, glass15)]):
        balls.append(((x, 0.7, z), 0.7, mat))
        balls.append(((x + 0.15, 0.6 + 0.1 * j, z - 0.1), 0.3, core))
    balls.append(((3.2, 0.6, 1.0), 0.6, metal))
    return sphere_desc(balls, mats)


def glass_camera(depth):
    return ob.camera(F(16.0) / F(9.0), 48, samples_per_pixel=16, max_depth=depth, look_from=(0.5, 2.2, 7.5),
                     look_at=(0.0, 0.5, 0.8), fov_degrees=40, defocus_degrees=0.4, focus_dist=7.0,
                     background=(0.7, 0.8, 1.0))


def test_glass_scene(torch_cuda, built):
    d = glass_scene()
    pd = ctypes.pointer(d)
    cam = glass_camera(50)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (48, 27, 16)
    seed = 11
    # what the seed exercises, from the oracle: per sample of rows 12..17, the draws of each segment's hit
    n_tir = n_drawn = n_scatter = 0
    for py in range(12, 18):
        for px in range(48):
            for k in range(16):
                prev = None
                for depth in range(0, 9):
                    _, c = ob.sample(pd, glass_camera(depth), seed, px, py, k, ob.ORDER_ITERATIVE)
                    if prev is not None and c["hits"] - prev["hits"] == 1:
                        dd = c["rng_draws"] - prev["rng_draws"]
                        n_tir += dd == 0
                        n_drawn += dd == 1
                        n_scatter += dd >= 3
                        assert dd != 2, (px, py, k, depth)
                    prev = c
    print(f"glass scene, rows 12..17, segments 1..8: total internal reflections {n_tir}, reflectance tests drawn "
          f"{n_drawn}, Lambertian / Metal scatters {n_scatter}")
    assert n_tir > 20, n_tir  # back-face hits with sin_t * eta > 1
    assert n_drawn > 1000 and n_tir + n_drawn > n_scatter, (n_tir, n_drawn, n_scatter)  # mostly glass
    dev = rtx.DeviceScene(pd)
    _, st, cnt = check_scene(torch_cuda, dev, pd, cam, seed, rtx.Region(0, 0, 48, 27, 0, 1))
    check_counters(st, cnt)


# ---- the general side of the two merged votes -----------------------------------------------------------------------
def test_trav_begin_division_side(torch_cuda, built):
    """Every camera ray lies in the plane z = 0 (the pixel grid's plane holds the camera): direction.z is exactly 0,
    outside rcp_newton's domain, so every wave that begins camera segments takes trav_begin's vote to the division
    side for all four reciprocals, 1 / a included (1 / 0 = inf: the rays are not `safe`).  A ring of Lambertian, Metal
    and glass spheres around the camera; the bounced rays take the fast side again."""
    mats = Materials()
    kinds = [mats.add(rtx.RTX_MAT_LAMBERTIAN, (0.7, 0.4, 0.3)), mats.add(rtx.RTX_MAT_METAL, (0.8, 0.8, 0.7), fuzz=0.2),
             mats.add(rtx.RTX_MAT_DIELECTRIC, ior=1.5)]
    balls = [((5.0 * np.cos(a), 5.0 * np.sin(a), 0.25 * (i % 3 - 1)), 1.6, kinds[i % 3])
             for i, a in enumerate(np.arange(8) * (np.pi / 4))]
    d = sphere_desc(balls, mats)
    w, h = 32, 18
    cam = plain_camera(w, h, 4, 8, (0, 0, 0), (-0.25 * (w // 2), 0.25 * (h // 2), 0.0), (0.25, 0, 0), (0, -0.25, 0))
    assert cam.pixel00[2] == cam.center[2] and cam.pixel_du[2] == 0.0 and cam.pixel_dv[2] == 0.0  # direction.z == 0
    pd = ctypes.pointer(d)
    _, st, cnt = check_scene(torch_cuda, rtx.DeviceScene(pd), pd, cam, 5, rtx.Region(0, 0, w, h, 0, 1))
    check_counters(st, cnt)
    assert cnt["hits"] > cnt["samples"] // 2  # most camera rays meet the ring


def test_unit_general_side(torch_cuda, built):
    """A scene of the size 1e-15: every camera ray's squared length is below 2^-96, so Unit(direction) of the first
    hit's Metal and Dielectric lanes takes unit()'s vote to the compiler's sqrt and division (the 2^32 pre-scaled root);
    the reflected and refracted rays have length 1 and take the fast side."""
    mats = Materials()
    metal = mats.add(rtx.RTX_MAT_METAL, (0.8, 0.8, 0.7), fuzz=0.1)
    glass = mats.add(rtx.RTX_MAT_DIELECTRIC, ior=1.5)
    lam = mats.add(rtx.RTX_MAT_LAMBERTIAN, (0.7, 0.4, 0.3))
    balls = [((0.0, 0.0, -1.2e-15), 2.2e-16, metal), ((-4.6e-16, 0.0, -1.2e-15), 2.0e-16, glass),
             ((4.6e-16, 0.0, -1.2e-15), 2.0e-16, lam), ((0.0, -3.2e-16, -1.0e-15), 1.0e-16, glass)]
    d = sphere_desc(balls, mats)
    w, h, u = 32, 18, 1e-17
    cam = plain_camera(w, h, 4, 8, (0, 0, 0), (-u * (w // 2), u * (h // 2), -40 * u), (u, 0, 0), (0, -u, 0))
    far = np.array([u * (w // 2 + 1), u * (h // 2 + 1), 40 * u], np.float64)  # no pixel sample lies further out
    assert float(far @ far) < 2.0 ** -96
    pd = ctypes.pointer(d)
    _, st, cnt = check_scene(torch_cuda, rtx.DeviceScene(pd), pd, cam, 5, rtx.Region(0, 0, w, h, 0, 1))
    check_counters(st, cnt)
    assert cnt["hits"] > cnt["samples"] // 4  # the spheres fill a good part of the view
