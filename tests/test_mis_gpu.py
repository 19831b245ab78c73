"""Multiple importance sampling of the direct light on the GPU (rtx_emitter_weight*, rtx_accum_add_mis,
wavefront.render(direct=True, mis=True)).

The weight block is held to tests/mis_ref.py bit for bit, field by field, on real pairs of three scenes (the event-1
hit and what its bounce found) and on hand-made edge pairs.  The estimator composed from the blocks is held to the
plain render where nothing is sampled and to closed forms with tolerances derived from the geometry, on a scene whose
light lies a tenth of a unit over the floor among them; the fused pass to the composed blocks bit for bit; and the
image of the Cornell box beside its light to the bound the weighting exists for."""
import math
import os

import numpy as np
import pytest

import direct_scenes as ds
import mis_ref
import rtx
import wavefront

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 5  # records after the n the call may write: they must keep their poison
SEED = 0x5EED00D1CE
COUNTS = (0, 1, 63, 64, 65)
SCENES = ("cornell_box", "simple_light_demo", "five")


@pytest.fixture(scope="module")
def torch(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def weight_dev(torch, dev, from_hits, hits, flags=0, stats=False):
    """rtx_emitter_weight_device on torch tensors: the output poisoned with 0xFF, PAD records longer than n."""
    n = len(hits)
    d = [to_device(torch, a) for a in (from_hits, hits)]
    out = torch.full(((n + PAD) * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = dev.emitter_weight_device(*[t.data_ptr() if n else 0 for t in d], n, out.data_ptr(), flags, stream_of(torch), stats)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 16:] == 0xFF).all(), "records past n were written"
    return got[: n * 16].view(rtx.EMITTER_WEIGHT_DTYPE), st


def same_records(got, want):
    assert got.dtype == want.dtype == rtx.EMITTER_WEIGHT_DTYPE and got.shape == want.shape
    if got.tobytes() == want.tobytes():
        return
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.argwhere(g != w)
    raise AssertionError(f"{len(np.unique(bad[:, 0]))} of {len(got)} records differ; first (record, word): {bad[:6].tolist()}; "
                         f"got {got[bad[0, 0]]} want {want[bad[0, 0]]}")


_scenes = {}


def scene(torch, name):
    """(description, device scene on the caller's tree, camera, host scene or None), made once and shared."""
    if name not in _scenes:
        if name == "five":
            host = None
            desc, cam = ds.five()
        else:
            host = rtx.HostScene(name, 1)
            desc, cam = host.desc, host.camera(width=64, spp=1, depth=8)
        _scenes[name] = (desc, rtx.DeviceScene(desc, reference_bvh=True, every_box=True), cam, host)
    return _scenes[name]


WINDOWS = {"cornell_box": (12, 20, 41, 25), "simple_light_demo": (10, 6, 41, 25), "five": (8, 6, 41, 25)}
_pairs = {}


def pairs(torch, name):
    """(from hits, hits, reference records) of one scene: the hit of every camera ray of two samples of a window
    (event 1) and what its bounce found.  Computed once, shared, never modified."""
    if name in _pairs:
        return _pairs[name]
    desc, dev, cam, _ = scene(torch, name)
    region = rtx.Region(*WINDOWS[name], 0, 1)
    P = rtx.region_rows(region) * region.width * 2
    d_rays = torch.empty((P, 8), dtype=torch.float32, device="cuda")
    d_keys = torch.empty((P, 4), dtype=torch.int32, device="cuda")
    rtx.camera_rays_device(cam, SEED, region, 0, 2, d_rays.data_ptr(), d_keys.data_ptr(), stream_of(torch))
    torch.cuda.synchronize()
    rays1 = d_rays.cpu().numpy().reshape(-1).view(rtx.RAY_DTYPE).copy()
    keys1 = d_keys.cpu().numpy().reshape(-1).view(rtx.KEY_DTYPE).copy()
    hits1 = dev.trace(rays1, rtx.RTX_TRACE_UV)
    b1 = dev.shade(rays1, hits1, keys1, SEED)
    hits2 = dev.trace(b1["ray"].copy(), rtx.RTX_TRACE_UV)
    _pairs[name] = (hits1, hits2, mis_ref.weight(desc, hits1, hits2))
    return _pairs[name]


# ---- the weight block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_block_equals_reference(torch, name):
    """Every bit of every field, about 2000 real pairs; the counter is the sum over the records."""
    desc, dev, _, _ = scene(torch, name)
    frm, hits, want = pairs(torch, name)
    weighted = (want["flags"] & rtx.RTX_EMITTER_WEIGHTED) != 0
    print(f"{name}: {len(want)} pairs, {int(weighted.sum())} weighted, geom up to {want['geom'].max():.4g}, "
          f"weights in [{want['weight'][weighted].min() if weighted.any() else 1:.4g}, 1]")
    assert len(want) >= 2000 and weighted.sum() >= 10  # bounces that found an emitter
    got, st = weight_dev(torch, dev, frm, hits, rtx.RTX_EMITTER_COUNTERS, stats=True)
    same_records(got, want)
    assert (st.n, st.weighted) == (len(want), int(weighted.sum())) and st.kernel_ms > 0
    timed, none = weight_dev(torch, dev, frm, hits)
    assert none is None
    same_records(timed, want)
    w = want[weighted]
    assert (w["weight"] >= 0).all() and (w["weight"] <= 1).all() and (w["geom"] > 0).all()
    assert (w["light"] < len(dev.lights())).all()
    assert (want["weight"][~weighted] == 1).all() and not want["geom"][~weighted].view(np.uint32).any()


def edge_scene():
    """A floor, a valid sphere light and a valid quad light, a DiffuseLight sphere of negative radius beside them,
    and a Metal sphere."""
    texs = [ds.solid(0.5, 0.5, 0.5), ds.solid(3, 4, 5)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1), ds.material(ds.METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.1)]
    spheres = [ds.sphere((0, 1, 0), 0.5, 1), ds.sphere((3, 1, 0), -0.5, 1), ds.sphere((-3, 1, 0), 0.5, 2)]
    quads = [ds.quad((-6, 0, -6), (0, 0, 12), (12, 0, 0), 0), ds.quad((-1, 3, -1), (2, 0, 0), (0, 0, 2), 1)]
    return ds.world(spheres, quads, mats, texs)


def edge_pairs():
    """Hand-made pairs on edge_scene, `from` on the floor at (1, 0, 0.5) unless said otherwise."""
    S, Q = rtx.RTX_PRIM_SPHERE << 28, rtx.RTX_PRIM_QUAD << 28
    kinds = ("sphere", "quad", "miss", "metal_hit", "metal_from", "from_miss", "same_point", "nan_point", "nan_from",
             "negative_radius", "hit_material_out", "from_material_out", "prim_out_of_range", "lambertian_hit",
             "from_below", "far")
    n = len(kinds)
    f, h = np.zeros(n, rtx.HIT_DTYPE), np.zeros(n, rtx.HIT_DTYPE)
    f["prim"], f["t"], f["front_face"], f["material"], f["point"], f["normal"] = Q | 0, 1.0, 1, 0, (1, 0, 0.5), (0, 1, 0)
    h["t"], h["front_face"], h["material"] = 1.0, 1, 1
    h["prim"], h["point"], h["normal"] = S | 0, (0.25, 0.625, 0.125), (0.5, -0.75, 0.25)  # (any unit-ish normal)
    k = {name: i for i, name in enumerate(kinds)}
    h["prim"][k["quad"]], h["point"][k["quad"]], h["normal"][k["quad"]] = Q | 1, (0.5, 3, 0.25), (0, -1, 0)
    h["prim"][k["miss"]], h["t"][k["miss"]] = rtx.RTX_HIT_NONE, np.inf
    h["prim"][k["metal_hit"]], h["material"][k["metal_hit"]] = S | 2, 2
    f["material"][k["metal_from"]] = 2
    f["prim"][k["from_miss"]], f["t"][k["from_miss"]] = rtx.RTX_HIT_NONE, np.inf
    h["point"][k["same_point"]] = f["point"][k["same_point"]]
    h["point"][k["nan_point"]] = (np.nan, 0.625, 0.125)
    f["normal"][k["nan_from"]] = (0, np.nan, 0)
    h["prim"][k["negative_radius"]], h["point"][k["negative_radius"]] = S | 1, (2.75, 0.625, 0.125)
    h["material"][k["hit_material_out"]] = 3
    f["material"][k["from_material_out"]] = 3
    h["prim"][k["prim_out_of_range"]] = S | 77
    h["prim"][k["lambertian_hit"]], h["material"][k["lambertian_hit"]] = Q | 0, 0
    f["normal"][k["from_below"]] = (0, -1, 0)  # cs < 0: g < 0, g * g as any other
    h["point"][k["far"]] = (2e19, 2e19, 0)     # d2 overflows to +inf: g = 0 by the arithmetic alone, wb = 0
    return f, h, k


def test_edge_pairs(torch):
    desc = edge_scene()
    f, h, k = edge_pairs()
    want = mis_ref.weight(desc, f, h)
    W = rtx.RTX_EMITTER_WEIGHTED
    for name in ("sphere", "quad", "from_below"):
        assert want["flags"][k[name]] == W and 0 < want["weight"][k[name]] < 1, name
    assert want["light"][k["sphere"]] == 0 and want["light"][k["quad"]] == 1
    for name in ("miss", "metal_hit", "metal_from", "from_miss", "hit_material_out", "from_material_out", "lambertian_hit"):
        r = want[k[name]]
        assert (r["weight"], r["geom"], r["light"], r["flags"]) == (1, 0, rtx.RTX_LIGHT_NONE, 0), name  # not weighted
    for name in ("same_point", "nan_point", "nan_from"):
        r = want[k[name]]
        assert (r["weight"], r["geom"], r["light"], r["flags"]) == (1, 0, 0, 0), name  # the emitter's, kept whole
    for name in ("negative_radius", "prim_out_of_range"):
        r = want[k[name]]
        assert (r["weight"], r["geom"], r["light"], r["flags"]) == (1, 0, rtx.RTX_LIGHT_NONE, 0), name  # weight exactly 1
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        assert [int(p) for p in dev.lights()["prim"]] == [0, (rtx.RTX_PRIM_QUAD << 28) | 1]
        got, st = weight_dev(torch, dev, f, h, rtx.RTX_EMITTER_COUNTERS, stats=True)
        same_records(got, want)
        assert st.weighted == int((want["flags"] == W).sum())
        same_records(dev.emitter_weight(f, h), want)
    finally:
        dev.close()


@pytest.mark.parametrize("n", COUNTS)
def test_counts_and_partial_waves(torch, n):
    """n = 0, 1, 63, 64, 65: a slice of the pairs gives the slice of the reference, through both entries."""
    _, dev, _, _ = scene(torch, "five")
    frm, hits, want = pairs(torch, "five")
    lo = max(0, int(np.nonzero(want["flags"])[0][0]) - 1)  # (the slice holds a weighted record from n = 2 on)
    got, st = weight_dev(torch, dev, frm[lo: lo + n], hits[lo: lo + n], rtx.RTX_EMITTER_COUNTERS, stats=True)
    same_records(got, want[lo: lo + n])
    assert (st.n, st.weighted) == (n, int((want["flags"][lo: lo + n] != 0).sum()))
    host_got, host_st = dev.emitter_weight(frm[lo: lo + n], hits[lo: lo + n], stats=True, flags=rtx.RTX_EMITTER_COUNTERS)
    same_records(host_got, want[lo: lo + n])
    assert (host_st.n, host_st.weighted) == (st.n, st.weighted)


def test_launch_cut_changes_nothing(torch):
    _, dev, _, _ = scene(torch, "five")
    frm, hits, want = pairs(torch, "five")
    os.environ["RTX_EMITTER_LAUNCH_RECORDS"] = "64"
    try:
        got, st = weight_dev(torch, dev, frm[:333], hits[:333], rtx.RTX_EMITTER_COUNTERS, stats=True)
    finally:
        os.environ.pop("RTX_EMITTER_LAUNCH_RECORDS", None)
    same_records(got, want[:333])
    assert st.weighted == int((want["flags"][:333] != 0).sum())


# ---- the composed loop ---------------------------------------------------------------------------------------
def test_no_emitters_is_the_plain_render(torch):
    """random_spheres 24 x 13, the caller's tree, depth 8: nothing is sampled and nothing weighted, carried and
    compacted."""
    host = rtx.HostScene("random_spheres", 1)
    cam = host.camera(width=24, spp=8, depth=8)
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True)
    try:
        plain = wavefront.render(dev, cam, 11, region).cpu().numpy()
        for compact in (False, True):
            lit = wavefront.render(dev, cam, 11, region, compact=compact, direct=True, mis=True).cpu().numpy()
            assert np.array_equal(plain.view(np.uint32), lit.view(np.uint32))
    finally:
        dev.close()


def test_depth_one_is_the_plain_render(torch):
    """max_depth 1 takes no light sample and weights nothing; at 2 and 8 the image is another one than the plain and
    the direct renders; compact = carried at every depth."""
    _, dev, cam, _ = scene(torch, "five")
    region = rtx.Region(3, 2, 37, 21, 0, 1)
    for depth in (1, 2, 8):
        cam.max_depth, cam.samples_per_pixel = depth, 3
        lit = [wavefront.render(dev, cam, 17, region, compact=c, direct=True, mis=True).cpu().numpy() for c in (False, True)]
        assert np.array_equal(lit[0].view(np.uint32), lit[1].view(np.uint32)), depth
        plain = wavefront.render(dev, cam, 17, region).cpu().numpy()
        direct = wavefront.render(dev, cam, 17, region, direct=True).cpu().numpy()
        assert np.array_equal(plain.view(np.uint32), lit[0].view(np.uint32)) == (depth == 1), depth
        assert np.array_equal(direct.view(np.uint32), lit[0].view(np.uint32)) == (depth == 1), depth
        # mis without direct is the plain render
        assert np.array_equal(wavefront.render(dev, cam, 17, region, mis=True).cpu().numpy().view(np.uint32), plain.view(np.uint32))
    cam.max_depth, cam.samples_per_pixel = 8, 1


NEAR_LIGHT = ("quad", 0.38, 1.38, -0.5, 0.5, 0.1)


def near_light_scene():
    """direct_scenes.floor_scene's floor and camera under one 1 x 1 quad light at height 0.1 over x in [0.38, 1.38],
    z in [-0.5, 0.5].  The camera's outermost ray passes the light's edge (at height 0.1: x = 0.9 tan 20 = 0.328), so
    no camera ray sees it; g reaches about 30 on the nearest column, the mean form factor is 0.047."""
    desc, cam, _ = ds.floor_scene("a")
    d = desc.contents
    quads = [d.quads[0], ds.quad((0.38, 0.1, -0.5), (1, 0, 0), (0, 0, 1), 1)]
    mats, texs = [d.materials[i] for i in range(d.n_materials)], [d.textures[i] for i in range(d.n_textures)]
    return ds.world([], quads, mats, texs), cam, [NEAR_LIGHT]


def analytic(kind):
    return near_light_scene() if kind == "near" else ds.floor_scene(kind)


def mis_bounds(cam, lights):
    """(expected image, F per pixel, sigma_p, N, the image bound) of the MIS estimator at depth 2, in units of a Le: a
    sample lies in [0, M_p], M_p = (g_max <= 1 ? g_max / (1 + g_max^2) : 1/2) + g_max^2 / (1 + g_max^2) with g_max
    from the geometry (direct_scenes.g_max), so sigma_p^2 <= F_p (M_p - F_p) (Bhatia-Davis).  N is the least power of
    two from 256 that brings the image bound 6 sqrt(mean sigma_p^2 / (P N)) to at most 3 % of the mean F."""
    want, f = ds.expected_image(cam, lights)
    g = ds.g_max(cam, lights)
    M = np.where(g <= 1, g / (1 + g * g), 0.5) + g * g / (1 + g * g)
    var = f * (M - f)
    assert (var > 0).all()
    N = 256
    while 6 * math.sqrt(float(var.mean()) / (f.size * N)) > 0.03 * float(f.mean()):
        N *= 2
    assert N <= 4096, N
    return want, f, np.sqrt(var), N, 6 * math.sqrt(float(var.mean()) / (f.size * N))


def hold_to_closed_form(kind, img, want, f, sigma, N, tol_img):
    scale = np.array(ds.ALBEDO) * np.array(ds.EMIT)
    ratio = img.mean(axis=(0, 1)) / want.mean(axis=(0, 1))
    worst = np.abs(img - want).max(axis=2) / scale.max() / (6 * sigma / math.sqrt(N))
    print(f"{kind}: N {N}, mean F {f.mean():.4f}, image mean / closed form {ratio}, bound {tol_img / f.mean():.4f}; "
          f"worst pixel at {worst.max():.3f} of its bound")
    assert np.all(np.abs(img.mean(axis=(0, 1)) - want.mean(axis=(0, 1))) <= tol_img * scale), (ratio, tol_img / f.mean())
    assert np.all(np.abs(img - want) <= (6 * sigma / math.sqrt(N))[..., None] * scale[None, None, :])


def test_near_light_scene_is_what_it_says():
    """The near-light scene's figures, from the geometry alone (no GPU): no camera ray sees the light, the mean form
    factor, g on the nearest column, the N of both estimators' bounds."""
    _, cam, lights = near_light_scene()
    x0, x1, _, _ = ds.footprints(cam)
    assert abs(0.38 - x1.max() * 0.9 - 0.052) < 1e-3
    want, f, sigma, N, tol = mis_bounds(cam, lights)
    g = ds.g_max(cam, lights)
    direct_n = (6 / 0.03) ** 2 * float(((g / 2) ** 2).mean()) / (f.size * float(f.mean()) ** 2)
    print(f"near: mean F {f.mean():.4f}, g_max {g.max():.1f}, N {N} (bound {tol / f.mean():.4f}); the direct-only bound asks {direct_n:.3g}")
    assert abs(f.mean() - 0.047) < 5e-4 and 25 < g.max() < 35 and N == 4096 and direct_n > 1e6
    _, cam, lights = ds.floor_scene("a")
    assert mis_bounds(cam, lights)[3] == 256


@pytest.mark.parametrize("kind", ["a", "b", "c", "near"])
def test_unbiased_against_closed_forms(torch, kind):
    """The composed estimator on the analytic scenes, 16 x 16, depth 2, within mis_bounds' tolerances: every pixel
    within 6 sigma_p / sqrt(N), the image mean within 6 sqrt(mean sigma_p^2 / (P N)).  A weight on the wrong segment
    or a missing one moves the near-light scene's image by tens of per cent."""
    desc, cam, lights = analytic(kind)
    want, f, sigma, N, tol_img = mis_bounds(cam, lights)
    cam.samples_per_pixel = N
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(desc)
    try:
        assert len(dev.lights()) == len(lights)
        img = wavefront.render(dev, cam, 424242, region, direct=True, mis=True).cpu().numpy().astype(np.float64)
    finally:
        dev.close()
    hold_to_closed_form(kind, img, want, f, sigma, N, tol_img)


# ---- the fused pass (rtx_accum_add_mis) ------------------------------------------------------------------------
def test_fused_no_emitters_is_the_plain_pass(torch):
    """random_spheres 24 x 13, the caller's tree, depth 8: add_mis(3) + add_mis(5) resolves, rgb and var, bit-equal
    to add(8)."""
    host = rtx.HostScene("random_spheres", 1)
    cam = host.camera(width=24, spp=8, depth=8)
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True)
    try:
        a, b = dev.accumulator(cam, 11, region), dev.accumulator(cam, 11, region)
        a.add_mis(3)
        st = a.add_mis(5, stats=True)
        b.add(8)
        assert a.samples == b.samples == 8
        assert st.samples == 5 * 24 * 13 and st.kernel_ms > 0 and st.walk_layout == rtx.RTX_LAYOUT_REFERENCE
        (rgb_a, var_a, _), (rgb_b, var_b, _) = a.resolve(), b.resolve()
        assert np.array_equal(rgb_a.view(np.uint32), rgb_b.view(np.uint32))
        assert np.array_equal(var_a.view(np.uint32), var_b.view(np.uint32))
        a.close()
        b.close()
    finally:
        dev.close()


FUSED_CASES = {  # region (x0, y0, width, height, rank, world), max_depth, passes
    "ragged_37x21_3+5": ((3, 2, 37, 21, 0, 1), 8, (3, 5)),
    "rank_1_of_3_depth_2": ((0, 0, 64, 30, 1, 3), 2, (8,)),
    "depth_1": ((3, 2, 37, 21, 0, 1), 1, (8,)),
    "depth_2": ((3, 2, 37, 21, 0, 1), 2, (8,)),
    "rank_1_of_3_depth_8": ((0, 0, 64, 30, 1, 3), 8, (8,)),
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
@pytest.mark.parametrize("name", SCENES)
def test_fused_equals_composed(torch, name, case):
    """add_mis resolves bit-equal to wavefront.render(direct=True, mis=True): ragged tiles, a rank of three, passes
    3 + 5 against 8 samples at once, max_depth 1 (also the plain pass), 2 and 8 (paths through Metal and Dielectric
    bounces between two Lambertian hits: the kept normal must be the last Lambertian hit's)."""
    window, depth, passes = FUSED_CASES[case]
    desc, dev, cam, host = scene(torch, name)
    if host is not None:
        cam = host.camera(width=64, spp=8, depth=depth)
    keep = (cam.max_depth, cam.samples_per_pixel)
    cam.max_depth, cam.samples_per_pixel = depth, sum(passes)
    region = rtx.Region(*window)
    want = wavefront.render(dev, cam, 29, region, direct=True, mis=True).cpu().numpy()
    acc = dev.accumulator(cam, 29, region)
    try:
        for n in passes:
            acc.add_mis(n)
        rgb, _, _ = acc.resolve()
        bad = np.argwhere((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=2))
        print(f"{name} {case}: {len(bad)} of {rgb.shape[0] * rgb.shape[1]} pixels differ; means {rgb.mean():.6g} "
              f"{want.mean():.6g}")
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(rgb[y, x], want[y, x]) for y, x in bad[:3]])
        if depth == 1:
            acc.reset()
            acc.add(sum(passes))
            assert np.array_equal(acc.resolve()[0].view(np.uint32), rgb.view(np.uint32))
    finally:
        acc.close()
        cam.max_depth, cam.samples_per_pixel = keep


def test_fused_on_a_scene_read_from_memory(torch):
    """direct_paths' MIS instantiation on a layout read from HBM: test_direct_gpu's memory scene cannot be imported
    without its tests, so a grid of its own: 48 x 48 small spheres under the World root, a floor, a quad light and a
    sphere light; add_mis of 3 samples resolves bit-equal to the composed blocks."""
    texs = [ds.solid(0.8, 0.7, 0.6), ds.solid(6, 5, 4), ds.solid(0.2, 0.5, 0.3)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1), ds.material(ds.LAMB, 2)]
    quads = [ds.quad((-4, 0, -4), (0, 0, 8), (8, 0, 0), 0), ds.quad((-1, 3, -1), (2, 0, 0), (0, 0, 2), 1)]
    g = 48
    xz = (np.arange(g, dtype=F32) - F32((g - 1) / 2)) * F32(0.15)
    spheres = [ds.sphere((2, 1.6, 0), 0.5, 1)] + [ds.sphere((float(x), 0.9, float(z)), 0.04, 2) for x in xz for z in xz]
    desc = ds.world(spheres, quads, mats, texs)
    cam = ds.five()[1]
    cam.max_depth, cam.samples_per_pixel = 8, 3
    region = rtx.Region(20, 12, 24, 13, 0, 1)
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        rays = np.zeros(1, rtx.RAY_DTYPE)
        rays["dir"], rays["tmax"] = (0, -1, 0), 1.0
        assert dev.trace(rays, 0, stats=True)[1].scene_placement == rtx.RTX_SCENE_IN_HBM
        composed = wavefront.render(dev, cam, 29, region, direct=True, mis=True).cpu().numpy()
        acc = dev.accumulator(cam, 29, region)
        try:
            acc.add_mis(3)
            rgb = acc.resolve()[0]
        finally:
            acc.close()
        bad = np.argwhere((rgb.view(np.uint32) != composed.view(np.uint32)).any(axis=2))
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(rgb[y, x], composed[y, x]) for y, x in bad[:3]])
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ["b", "near"])
def test_fused_unbiased_against_closed_forms(torch, kind):
    """The fused pass itself on analytic scene b (two quad lights) and on the near-light scene, with mis_bounds."""
    desc, cam, lights = analytic(kind)
    want, f, sigma, N, tol_img = mis_bounds(cam, lights)
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(desc)
    try:
        acc = dev.accumulator(cam, 424242, region)
        acc.add_mis(N)
        img = acc.resolve()[0].astype(np.float64)
        acc.close()
    finally:
        dev.close()
    hold_to_closed_form(f"fused {kind}", img, want, f, sigma, N, tol_img)


def test_accumulator_modes(torch):
    """MIS after plain, adaptive or direct, and each of those after MIS, fail until reset; flags must be 0; preview,
    ppm and sample_counts of an MIS accumulator run."""
    _, dev, cam, _ = scene(torch, "five")
    cam.max_depth = 4
    region = rtx.Region(0, 0, 40, 20, 0, 1)
    acc = dev.accumulator(cam, 3, region)

    def refused(call):
        with pytest.raises(rtx.RtxError) as e:
            call()
        assert e.value.code == rtx.RTX_ERR_INVALID_ARG

    try:
        refused(lambda: acc.add_mis(0))
        refused(lambda: acc.add_mis(1, flags=1))
        assert acc.samples == 0
        acc.add_mis(2)
        refused(lambda: acc.add(1))
        refused(lambda: acc.add_adaptive(1, 0.1))
        refused(lambda: acc.add_direct(1))
        refused(lambda: acc.add_direct(1, flags=1))
        assert acc.samples == 2
        rgb = acc.resolve()[0]
        assert np.isfinite(rgb).all() and rgb.max() > 0
        assert acc.ppm().startswith(b"P3\n40 20\n255\n") and acc.preview(2).shape == (20, 40, 3)
        assert (acc.sample_counts() == 2).all()
        for first in (lambda: acc.add(2), lambda: acc.add_adaptive(2, 0.1), lambda: acc.add_direct(2)):
            acc.reset()
            first()
            refused(lambda: acc.add_mis(1))
        acc.reset()
        acc.add_mis(1)
        acc.add_mis(1)
        assert acc.samples == 2 and np.array_equal(acc.resolve()[0].view(np.uint32), rgb.view(np.uint32))
    finally:
        acc.close()
        cam.max_depth = 8


# ---- boundedness: the property the feature exists for ----------------------------------------------------------
def test_cornell_ceiling_beside_the_light_is_bounded(torch):
    """cornell_box at depth 2, a 32 x 32 window on the ceiling beside the light, 16 spp.  A sample is the emission seen
    directly (at most Le), or a light sample (at most a Le / 2) plus a weighted bounce (at most a Le): every channel of
    every pixel is at most max(Le, 1.5 a_max Le).  The direct-only estimator's largest pixel is printed beside it."""
    desc, dev, _, host = scene(torch, "cornell_box")
    d = desc.contents
    colour = lambda m: max(d.textures[m.texture].even)  # noqa: E731  (the Cornell box's textures are SolidColors)
    mats = [d.materials[i] for i in range(d.n_materials)]
    assert all(d.textures[m.texture].type == rtx.RTX_TEX_SOLID for m in mats
               if m.type in (rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT))
    a_max = max(colour(m) for m in mats if m.type == rtx.RTX_MAT_LAMBERTIAN)
    le = max(colour(m) for m in mats if m.type == rtx.RTX_MAT_DIFFUSE_LIGHT)
    assert 0 < a_max < 1 and le > 1
    cam = host.camera(width=256, spp=16, depth=2)
    # at this width the light covers rows 34 to 42, columns 106 to 150, and the ceiling starts at row 6: the window's
    # last rows are the ceiling a unit above the light's near edge, where the direct-only estimator's g is largest
    region = rtx.Region(112, 2, 32, 32, 0, 1)
    acc = dev.accumulator(cam, 7, region)
    try:
        acc.add_mis(16)
        img = acc.resolve()[0]
        acc.reset()
        acc.add_direct(16)
        old = acc.resolve()[0]
    finally:
        acc.close()
    bound = max(le, 1.5 * a_max * le)
    print(f"cornell ceiling window: a_max {a_max}, Le {le}, bound {bound}; largest MIS pixel {img.max():.4f}, "
          f"largest direct=True pixel {old.max():.4f}; means {img.mean():.4f} {old.mean():.4f}")
    assert img.min() >= 0 and img.max() > 0
    assert img.max() <= bound, (img.max(), bound)


def test_device_check_is_clean(torch):
    for rec in _scenes.values():
        rec[1].close()
    _scenes.clear()
    _pairs.clear()
    rtx.device_check(0)
