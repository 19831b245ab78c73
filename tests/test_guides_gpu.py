"""First-hit guide images on the GPU (rtx_guides*).

The contract is the one include/rtx.h spells out: a guide is the fold, in k order, of the first hits of the render's own
camera rays.  The reference composes the blocks the existing tests pin to the oracle, rtx.camera_rays ->
DeviceScene.trace(RTX_TRACE_UV) -> DeviceScene.shade (a Lambertian's attenuation is its texture value; a Metal's
albedo comes from the description), and folds them with tests/denoise_ref.py; equality is bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import denoise_ref as dr
import ref64_cases as rc
import rtx

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 7  # records after the last the call may write: they must keep their poison


@pytest.fixture(scope="module")
def torch(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def case(name):
    _, make, seed, window, _, _ = rc.CASES[rc.NAMES.index(name)]
    desc, cam = make()
    return desc, cam, seed, rtx.Region(*(window or (0, 0, cam.image_width, cam.image_height)), 0, 1)


def reference(dev, desc, cam, seed, region, first, count):
    """The guides of the region's shard from camera rays, a closest-hit trace and a shade, folded in numpy."""
    rays, keys = rtx.camera_rays(cam, seed, region, first, count)
    hits = dev.trace(rays, flags=rtx.RTX_TRACE_UV | rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)))
    bounce = dev.shade(rays, hits, keys, seed)
    d = desc.contents
    kinds = np.array([d.materials[i].type for i in range(d.n_materials)])
    albedo = np.array([list(d.materials[i].albedo) for i in range(d.n_materials)], F)
    hit = hits["prim"] != rtx.RTX_HIT_NONE
    mi = np.where(hit, hits["material"], 0)
    kind = np.where(hit, kinds[mi], -1)
    a = np.ones(hit.shape + (3,), F)  # a miss, a Dielectric, a DiffuseLight
    a[kind == rtx.RTX_MAT_LAMBERTIAN] = bounce["attenuation"][kind == rtx.RTX_MAT_LAMBERTIAN]
    a[kind == rtx.RTX_MAT_METAL] = albedo[mi][kind == rtx.RTX_MAT_METAL]
    n = np.where(hit[..., None], hits["normal"], F(0)).astype(F)
    return dr.fold_guides(a, n, hits["t"], hit), kind


def guides_dev(torch, dev, cam, seed, region, first, count, stats=False):
    """rtx_guides_device into a buffer poisoned with 0xFF, PAD records longer than the shard."""
    rows = rtx.region_rows(region)
    n = rows * region.width
    out = torch.full(((n + PAD) * 32,), 0xFF, dtype=torch.uint8, device="cuda")
    st = dev.guides_device(cam, seed, region, first, count, out.data_ptr(), stream_of(torch), stats)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 32:] == 0xFF).all(), "records past the shard were written"
    got = got[: n * 32].view(rtx.GUIDE_DTYPE).reshape(rows, region.width)
    return (got, st) if stats else got


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got.view(np.uint32).reshape(got.shape + (8,)) != want.view(np.uint32).reshape(want.shape + (8,)))
    assert len(bad) == 0, (len(bad), bad[:4], [(got[y, x], want[y, x]) for y, x, _ in bad[:4]])


# (case, samples): the Cornell box (quads), the earth (an image texture on a Lambertian), noise on lights and a
# checker on a Lambertian sphere and quad, Metal with and without fuzz, glass seen from outside, inside and as a sheet
SCENES = [("random_spheres_24x13x4", 4), ("cornell_box_window", 3), ("earth_window", 3), ("noise_sphere4_quad0.5", 2),
          ("noise_host_tables", 2), ("lambertian_checker", 3), ("metal_sphere_quad_fuzz", 3), ("dielectric_sphere", 3),
          ("dielectric_sphere_inside", 2), ("dielectric_sheet_front", 2), ("sphere_image_inside", 2), ("quad_image_back", 2)]
WANT_KINDS = {"random_spheres_24x13x4": {-1, rtx.RTX_MAT_LAMBERTIAN}, "cornell_box_window": {rtx.RTX_MAT_LAMBERTIAN},
              "earth_window": {rtx.RTX_MAT_LAMBERTIAN}, "metal_sphere_quad_fuzz": {rtx.RTX_MAT_METAL},
              "lambertian_checker": {rtx.RTX_MAT_LAMBERTIAN}, "dielectric_sphere": {rtx.RTX_MAT_DIELECTRIC},
              "dielectric_sheet_front": {rtx.RTX_MAT_DIELECTRIC}, "noise_sphere4_quad0.5": {rtx.RTX_MAT_DIFFUSE_LIGHT}}


@pytest.mark.parametrize("name,count", SCENES)
def test_guides_equal_the_folded_blocks(torch, name, count):
    desc, cam, seed, region = case(name)
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        want, kind = reference(dev, desc, cam, seed, region, 0, count)
        assert set(np.unique(kind)) >= WANT_KINDS.get(name, set()), (name, set(np.unique(kind)))
        got, st = guides_dev(torch, dev, cam, seed, region, 0, count, stats=True)
        same(got, want)
        assert st.rays == want.size * count and st.kernel_ms > 0
        same(guides_dev(torch, dev, cam, seed, region, 0, count), want)  # without stats: enqueued only
        host, hst = dev.guides(cam, seed, region, 0, count, stats=True)  # the host entry equals the device entry
        same(host, want)
        assert hst.rays == st.rays
    finally:
        dev.close()


def test_noise_on_a_lambertian(torch):
    """perlin_demo: both spheres are Lambertians with the Perlin texture (the kernels built for such scenes)."""
    host = rtx.HostScene("perlin_demo", 1)
    cam = host.camera(width=64, spp=2, depth=50)
    region = rtx.Region(5, 3, 41, 23, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True, every_box=True)
    try:
        want, kind = reference(dev, host.desc, cam, 9, region, 0, 2)
        assert (kind == rtx.RTX_MAT_LAMBERTIAN).any() and len(np.unique(want["albedo"])) > 100
        same(guides_dev(torch, dev, cam, 9, region, 0, 2), want)
    finally:
        dev.close()


_spheres = {}


def spheres(torch, library):
    """randSpheres at 256 x 144 on the caller's tree or on the library's trees, and the folded blocks of its whole
    frame over samples [0, 5): computed once, shared, never modified."""
    if library not in _spheres:
        host = rtx.HostScene("random_spheres", 1)
        cam = host.camera(width=256, spp=5, depth=50)
        dev = rtx.DeviceScene(host.desc) if library else rtx.DeviceScene(host.desc, reference_bvh=True, every_box=True)
        whole = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
        rays, keys = rtx.camera_rays(cam, 21, whole, 0, 5)
        hits = dev.trace(rays, flags=rtx.RTX_TRACE_UV | rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)))
        bounce = dev.shade(rays, hits, keys, 21)
        _spheres[library] = dict(host=host, cam=cam, dev=dev, seed=21, whole=whole, hits=hits, bounce=bounce)
    return _spheres[library]


def fold_window(s, region, first, count):
    """The reference guides of a window or shard of the shared frame, from its per-sample blocks."""
    d = s["host"].desc.contents
    kinds = np.array([d.materials[i].type for i in range(d.n_materials)])
    albedo = np.array([list(d.materials[i].albedo) for i in range(d.n_materials)], F)
    L = rtx.load()
    ys = [region.y0 + int(L.rtx_region_row(ctypes.byref(region), ctypes.c_uint32(i))) for i in range(rtx.region_rows(region))]
    hits = s["hits"][first: first + count][:, ys][:, :, region.x0: region.x0 + region.width]
    att = s["bounce"]["attenuation"][first: first + count][:, ys][:, :, region.x0: region.x0 + region.width]
    hit = hits["prim"] != rtx.RTX_HIT_NONE
    mi = np.where(hit, hits["material"], 0)
    kind = np.where(hit, kinds[mi], -1)
    a = np.ones(hit.shape + (3,), F)
    a[kind == rtx.RTX_MAT_LAMBERTIAN] = att[kind == rtx.RTX_MAT_LAMBERTIAN]
    a[kind == rtx.RTX_MAT_METAL] = albedo[mi][kind == rtx.RTX_MAT_METAL]
    n = np.where(hit[..., None], hits["normal"], F(0)).astype(F)
    return dr.fold_guides(a, n, hits["t"], hit)


@pytest.mark.parametrize("library", [False, True])
def test_whole_frame_and_library_trees(torch, library):
    s = spheres(torch, library)
    same(guides_dev(torch, s["dev"], s["cam"], s["seed"], s["whole"], 0, 4), fold_window(s, s["whole"], 0, 4))


# 1, 63, 64, 65 and 4097 pixels; a window ragged against the 8 x 8 tile in both directions; one row of tiles and a bit
@pytest.mark.parametrize("window", [(200, 100, 1, 1), (100, 80, 63, 1), (100, 80, 64, 1), (100, 80, 65, 1), (7, 60, 241, 17),
                                    (3, 2, 37, 21), (90, 70, 9, 65)])
def test_partial_waves(torch, window):
    s = spheres(torch, False)
    region = rtx.Region(*window, 0, 1)
    same(guides_dev(torch, s["dev"], s["cam"], s["seed"], region, 0, 3), fold_window(s, region, 0, 3))


def test_shard_sample_ranges_and_the_last_sample(torch):
    s = spheres(torch, False)
    shard = rtx.Region(3, 2, 137, 61, 1, 3, 4)  # rank 1 of 3, stripes of 4 rows
    rows = rtx.region_rows(shard)
    assert 0 < rows < 61
    same(guides_dev(torch, s["dev"], s["cam"], s["seed"], shard, 0, 5), fold_window(s, shard, 0, 5))
    # samples [3, 5) of [0, 5)
    region = rtx.Region(60, 50, 70, 37, 0, 1)
    part = guides_dev(torch, s["dev"], s["cam"], s["seed"], region, 3, 2)
    same(part, fold_window(s, region, 3, 2))
    assert part.tobytes() != fold_window(s, region, 0, 2).tobytes()
    # the last sample word
    top = (1 << 32) - 2
    small = rtx.Region(100, 90, 24, 13, 0, 1)
    want, _ = reference(s["dev"], s["host"].desc, s["cam"], s["seed"], small, top, 1)
    same(guides_dev(torch, s["dev"], s["cam"], s["seed"], small, top, 1), want)
    with pytest.raises(rtx.RtxError) as e:
        guides_dev(torch, s["dev"], s["cam"], s["seed"], small, top, 2)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG


def test_the_knobs_change_no_bit(torch):
    """The tile's shape and the fold threshold are A/B knobs: every setting gives the same records."""
    s = spheres(torch, False)
    region = rtx.Region(3, 2, 137, 61, 0, 1)
    want = fold_window(s, region, 0, 4)
    names = ("RTX_GUIDES_TILE_W_LOG2", "RTX_GUIDES_REFILL", "RTX_GUIDES_PRIM_BATCH")
    old = {k: os.environ.get(k) for k in names}
    try:
        for tile, refill, batch in ((6, 48, 16), (0, 48, 16), (4, 1, 16), (3, 64, 1), (3, 17, 65), (5, 33, 8)):
            os.environ.update(zip(names, (str(tile), str(refill), str(batch))))
            same(guides_dev(torch, s["dev"], s["cam"], s["seed"], region, 0, 4), want)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_a_scene_read_from_memory(torch):
    """stress_100k does not fit the LDS copy: the walk reads the layout from memory, with the rank word's tie rule."""
    host = rtx.HostScene("stress_100k", 1)
    cam = host.camera(width=96, spp=2, depth=50)
    region = rtx.Region(30, 20, 41, 13, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True, every_box=True)
    try:
        want, kind = reference(dev, host.desc, cam, 5, region, 0, 2)
        assert (kind >= 0).any()
        same(guides_dev(torch, dev, cam, 5, region, 0, 2), want)
    finally:
        dev.close()


def test_renders_are_left_alone(torch):
    """A render's image and RTX_FLAG_COUNTERS stats before and after a guides call are equal, and the sample scratch
    is not touched."""
    host = rtx.HostScene("random_spheres", seed=1)
    cam = host.camera(width=48, spp=8, depth=50)
    whole = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(host.desc)
    work = [n for n, _ in rtx.Stats._fields_ if n not in ("kernel_ms", "gather_ms", "trav_cycles", "shade_cycles",
                                                          "shade_split_cycles")]
    try:
        img0, st0 = dev.render_host(cam, 7, counters=True)
        scratch = rtx.device_scratch_bytes(0)
        assert scratch > 0
        g, st = guides_dev(torch, dev, cam, 7, whole, 0, 4, stats=True)
        assert st.rays == 4 * 48 * 27 and 0 < g["cover"].mean() < 1
        assert rtx.device_scratch_bytes(0) == scratch
        img1, st1 = dev.render_host(cam, 7, counters=True)
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
        assert {k: getattr(st0, k) for k in work} == {k: getattr(st1, k) for k in work}
        rtx.release_device_memory(0)  # releasing the device's scratch does not disturb the guides
        again = guides_dev(torch, dev, cam, 7, whole, 0, 4)
        assert again.tobytes() == g.tobytes() and rtx.device_scratch_bytes(0) == 0
    finally:
        dev.close()
    rtx.device_check(0)


def test_zz_device_check_and_close(torch):
    """Last in the module: every call above left the device's sticky error word clean; free the module's scenes."""
    rtx.device_check(0)
    for s in _spheres.values():
        s["dev"].close()
    _spheres.clear()
