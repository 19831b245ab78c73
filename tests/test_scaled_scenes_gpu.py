"""One scene scaled across each guard of the walk's fast float32 forms, through both render kernels.

The assembly walk restates the slab, root and sqrt forms of csrc/rtx_device.h by hand, its cold path for
|disc| < 2^-96 included, and can only be reached through a render.  Every case is hand_scenes' ring of Lambertian,
Metal and glass spheres at 32 x 18 x 4, depth 8, scaled together with its camera so that one frame has rays on both
sides of a guard, and goes through parity.check_scene: the timed and the counting kernel bit-identical to the oracle,
the counters equal.  For every case a test without a GPU shows, from float64 bounds that include the pixel jitter or
from the float32 run of the independent tracer (ref64), that at least a quarter of the pixels, first hits or segments
lie on each side, and that more than a quarter of the samples hit.

  a-low, a-high   camera rays whose a = lensq(direction) straddles 2^-60 and 2^60 (Trav::safe's a_ok).
  tiny            a scene of the size 2^-48, as small as a scene can be: a camera ray that is to pass tmin = 0.001
                  there has |d| < 2^-36, so it is not safe, hb^2 < 2^-164 underflows and disc is +-0: every sample
                  "hits".  Its bounce rays never reach a square root (measured below: no disc >= 0), so the straddle
                  of 2^-96 is `cold-sqrt`'s.
  cold-sqrt       a scene of the size 2^-18.6 seen by camera rays with a just above 2^-60: the rays are safe and the
                  first hits' disc = a (r^2 - p^2) lies on both sides of 2^-96 — the assembly walk's cold path, with
                  roots that pass tmin.
  subnormal-disc  the same with a r^2 about 2^-127: a camera ray that misses a sphere narrowly has a negative SUBNORMAL
                  disc, which v_sqrt_f32 flushes to -0 — the walk's vote is on |disc| < 2^-96 for that reason (the
                  parent's assembly walk took -hb / a for a root there and rendered hits the reference does not have).
  x-2^32          the ring reaches up to the plane x = 2^32 and the camera looks at it from beyond that plane.  A scene
                  walks in two tiers only if every near box lies within 2^32 (rtx_topology), so no hit point can lie
                  beyond the plane: what straddles near_fma_ok is the segments — every camera segment starts beyond
                  2^32 (the reference's slab form, ray by ray), every bounce segment within it (the FMA form), and the
                  pool mixes both in its waves.  The case asserts that the scene is tiered.
"""
import ctypes

import numpy as np
import pytest

import hand_scenes as H
import ref64
import rtx
from parity import check_scene, tier_of

F = np.float32
W, HT, SPP, DEPTH, SEED = 32, 18, 4, 8, 5


def x_camera(scale, cx, dist=4.0, step=0.25):
    """A camera at (cx, 0, 0) looking down -x at a pixel grid `dist` away (times scale)."""
    c0 = np.array([cx, 0.0, 0.0])
    p00 = c0 + scale * np.array([-dist, step * (HT // 2), -step * (W // 2)])
    return H.plain_camera(W, HT, SPP, DEPTH, c0, p00, (0, 0, scale * step), (0, -scale * step, 0))


def build(name):
    """(scene description, camera, the ring's (centre, radius, material) list) of a case."""
    mats, kinds = H.ring_materials()
    ring, cam_scale, centre, cam = 1.0, None, (0.0, 0.0, 0.0), None
    if name == "a-low":
        ring = 2.0 ** -30 / np.sqrt(22.0)  # a = scale^2 (16 + x^2 + y^2), about 22 scale^2 at the median pixel
    elif name == "a-high":
        ring = 2.0 ** 30 / np.sqrt(22.0)
    elif name == "tiny":
        ring = 2.0 ** -48 / 1.13
    elif name == "cold-sqrt":
        cam_scale = 2.0 ** -31.9  # a in [16, 37] scale^2: from 2^-59.8 up
        ring = np.sqrt(2.0 ** -95 / (2.56 * 24.0)) / cam_scale  # a r^2 about 2 * 2^-96: disc is uniform in [0, a r^2]
    elif name == "subnormal-disc":
        cam_scale = 2.0 ** -31.9
        ring = np.sqrt(2.0 ** -127 / (2.56 * 24.0)) / cam_scale
    elif name == "x-2^32":
        ring = 2.0 ** 27
        centre = (2.0 ** 32 - 7.5 * ring, 0.0, 0.0)  # the ring's spheres end 0.9 ring short of the plane
        cam = x_camera(ring, centre[0] + 9.0 * ring)
    else:
        raise KeyError(name)
    balls = H.ring_balls(kinds, ring, centre)
    if cam is None:
        cam = H.ring_camera(W, HT, SPP, DEPTH, ring if cam_scale is None else cam_scale, centre)
    return H.sphere_desc(balls, mats), cam, balls


CASES = ("a-low", "a-high", "tiny", "cold-sqrt", "subnormal-disc", "x-2^32")


def a_bounds(cam):
    """Per pixel, float64 bounds of lensq(direction) over the pixel's jitter square (camera.go:265-299)."""
    c, p = np.array(cam.center[:], np.float64), np.array(cam.pixel00[:], np.float64)
    du, dv = np.array(cam.pixel_du[:], np.float64), np.array(cam.pixel_dv[:], np.float64)
    i, j = np.meshgrid(np.arange(W), np.arange(HT))
    mid = (p - c) + i[..., None] * du + j[..., None] * dv
    half = 0.5 * (np.abs(du) + np.abs(dv))
    lo = (np.maximum(np.abs(mid) - half, 0.0) ** 2).sum(-1)
    hi = ((np.abs(mid) + half) ** 2).sum(-1)
    return lo, hi


def first_segments(name):
    desc, cam, balls = build(name)
    res = ref64.trace(ctypes.pointer(desc), cam, SEED, ref64.grid(0, 0, W, HT, SPP), np.float32, dump=True)
    return desc, cam, balls, res


def disc32(o, d, c, r):
    """hittables.go:97-102 in float32."""
    with np.errstate(all="ignore"):
        oc = o - c
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        hb = (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1]) + d[:, 2] * oc[:, 2]
        cc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - r * r
        return hb * hb - a * cc


@pytest.mark.parametrize("name,edge", [("a-low", 2.0 ** -60), ("a-high", 2.0 ** 60)])
def test_camera_rays_straddle_a_ok(name, edge):
    _, cam, _ = build(name)
    lo, hi = a_bounds(cam)
    slack = 1 + 2.0 ** -20  # float32 rounding of lensq and of the sampled point, generously
    below, above = int((hi * slack < edge).sum()), int((lo > edge * slack).sum())
    print(f"{name}: {below} pixels wholly below {edge:g}, {above} wholly above, of {lo.size}")
    assert below >= lo.size // 4 and above >= lo.size // 4
    other = 2.0 ** 60 if name == "a-low" else 2.0 ** -60
    assert (hi < other).all() or (lo > other).all()  # the other edge is not in play


def test_tiny_scene_bounces_reach_no_sqrt():
    _, cam, balls, res = first_segments("tiny")
    _, hi = a_bounds(cam)
    assert (hi < 2.0 ** -60).all()  # no camera ray is safe
    d0 = res.dump[0]
    m = d0["scattered"]
    n_sqrt = sum(int((disc32(d0["point"][m], d0["next_dir"][m], np.array(c, F), F(r)) >= 0).sum()) for c, r, _ in balls)
    print(f"tiny: {len(d0['g'])} first hits, {int(m.sum())} bounce rays, {n_sqrt} of their sphere tests take a square root")
    assert len(d0["g"]) > W * HT * SPP // 4
    assert n_sqrt == 0  # why the straddle of 2^-96 is cold-sqrt's case (module docstring)


def test_cold_sqrt_first_hits_straddle_2_96():
    _, cam, balls, res = first_segments("cold-sqrt")
    lo, hi = a_bounds(cam)
    assert (lo >= 2.0 ** -60 * (1 + 2.0 ** -20)).all() and (hi < 2.0 ** 60).all()  # every camera ray is safe
    d0 = res.dump[0]
    cen = np.array([balls[p][0] for p in d0["prim"]], F)
    rad = np.array([balls[p][1] for p in d0["prim"]], F)
    disc = disc32(d0["origin"].astype(F), d0["dir"].astype(F), cen, rad)
    below, above = int(((disc >= 0) & (disc < F(2.0 ** -96))).sum()), int((disc >= F(2.0 ** -96)).sum())
    print(f"cold-sqrt: {len(disc)} first hits of {W * HT * SPP} samples, disc below 2^-96 on {below}, from it up on {above}")
    assert below + above == len(disc) > W * HT * SPP // 4
    assert below >= len(disc) // 4 and above >= len(disc) // 4


def test_subnormal_disc_near_misses():
    """Pixel-centre camera rays against every sphere, in float32: at least a quarter of the pixels have a negative
    subnormal disc against some sphere, and as many a first hit."""
    _, cam, balls, res = first_segments("subnormal-disc")
    lo, hi = a_bounds(cam)
    assert (lo >= 2.0 ** -60 * (1 + 2.0 ** -20)).all() and (hi < 2.0 ** 60).all()  # every camera ray is safe
    c, p = np.array(cam.center[:], F), np.array(cam.pixel00[:], F)
    du, dv = np.array(cam.pixel_du[:], F), np.array(cam.pixel_dv[:], F)
    i, j = np.meshgrid(np.arange(W, dtype=F), np.arange(HT, dtype=F))
    d = (((p + i.reshape(-1, 1) * du) + j.reshape(-1, 1) * dv) - c).astype(F)
    o = np.broadcast_to(c, d.shape)
    disc = np.stack([disc32(o, d, np.array(cc, F), F(r)) for cc, r, _ in balls], 1)
    neg_sub = ((disc < 0) & (disc > -F(2.0 ** -126))).any(1)
    print(f"subnormal-disc: {int(neg_sub.sum())} of {len(d)} pixel centres have a negative subnormal disc, "
          f"{int((disc >= 0).any(1).sum())} a non-negative one; {len(res.dump[0]['g'])} first hits of {W * HT * SPP} samples")
    assert neg_sub.sum() >= len(d) // 4
    assert len(res.dump[0]["g"]) > W * HT * SPP // 4


def test_x_plane_segments_straddle_near_fma_ok(built):
    desc, cam, _, res = first_segments("x-2^32")
    assert cam.center[0] > 2.0 ** 32
    box, active = rtx.walk_near_region(ctypes.pointer(desc), cam)
    assert active and box[3] > cam.center[0]  # the scene walks in two tiers for this camera
    n_cam = W * HT * SPP
    n_bounce = int(res.segments.sum()) - n_cam
    beyond = sum(int((np.abs(d["origin"][:, 0]) > F(2.0 ** 32)).sum()) for d in res.dump[1:])
    print(f"x-2^32: {n_cam} camera segments beyond the plane, {n_bounce} bounce segments, {beyond} of their hits' origins beyond it")
    assert beyond == 0 and n_bounce >= (n_cam + n_bounce) // 4 and n_cam >= (n_cam + n_bounce) // 4
    assert len(res.dump[0]["g"]) > n_cam // 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_scaled_scene_parity(torch_cuda, built, name):
    desc, cam, _ = build(name)
    pd = ctypes.pointer(desc)
    dev = rtx.DeviceScene(pd)
    if name == "x-2^32":
        assert tier_of(dev, pd, cam) is not None
    _, st, cnt = check_scene(torch_cuda, dev, pd, cam, SEED, rtx.Region(0, 0, W, HT, 0, 1))
    assert st.rng_draws == cnt["rng_draws"] and st.hits == cnt["hits"]
    assert cnt["hits"] > cnt["samples"] // 4  # more than a quarter of the samples hit (a hit per sample at the least)
    if name == "x-2^32":
        assert st.walk_layout & rtx.RTX_LAYOUT_TIERED
