"""Progressive rendering on the GPU (rtx_accum, include/rtx.h): after n accumulated samples the
resolved image is bit-identical to a one-shot render with samples_per_pixel = n and to the oracle, the variance and
the noisy-pixel count are bit-identical to the numpy reference (accum_ref.py), and every pass's work counters are the
oracle's for exactly that pass's samples."""
import ctypes

import numpy as np
import pytest

import accum_ref
import oracle_binding as ob
import rtx
from parity import WORK_KEYS, gpu_region, tier_of, walk_of

pytestmark = pytest.mark.gpu

REL_TOL = 0.1


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


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def oracle_counters(dev, desc, cam, seed, reg):
    """The oracle's counters for cam's samples on the tree the scene walks, with its skips and tiers (parity.py)."""
    tier = tier_of(dev, desc, cam)
    if tier is not None:
        walk, skip, tw = tier
    else:
        (walk, skip), tw = walk_of(dev, desc, cam), None
    rank = ob.sphere_ranks(desc) if walk is not desc else None
    return ob.render(walk, cam, seed, reg, ob.ORDER_ITERATIVE, skip=skip, tier=tw, rank=rank)[1]


def run_passes(torch, dev, scene, cam_of, seed, reg, passes, key, counting=False, check_var=True):
    """Add `passes` to a new accumulator; after each, every check of the module docstring.  cam_of(n): the camera
    with samples_per_pixel = n.  Returns the last (rgb, var, noisy)."""
    total = sum(passes)
    pixels = rtx.region_rows(reg) * reg.width
    col = accum_ref.sample_colours(key, scene.desc, cam_of(total), seed, reg, total) if check_var else None
    acc = dev.accumulator(cam_of(total), seed, reg)
    try:
        assert acc.samples == 0
        done, before, out = 0, None, None
        for count in passes:
            st = acc.add(count, stream_of(torch), stats=True, counters=counting)
            done += count
            assert acc.samples == done
            assert st.samples == pixels * count, (st.samples, pixels, count)
            assert st.sample_chunks >= 1 and st.kernel_ms > 0
            rgb, var, noisy = out = acc.resolve(REL_TOL)
            one, st1 = gpu_region(torch, dev, cam_of(done), seed, reg, counters=False)
            assert st.walk_layout == st1.walk_layout
            assert np.array_equal(rgb, one), f"after {done} samples: max {np.abs(rgb - one).max()} from the one-shot render"
            if check_var:
                want_rgb, want_var, want_noisy = accum_ref.after(col, done, REL_TOL)
                assert np.array_equal(rgb, want_rgb)
                assert np.array_equal(var, want_var), f"after {done} samples: variance differs from the reference"
                assert noisy == want_noisy, (done, noisy, want_noisy)
            if counting:
                cnt = oracle_counters(dev, scene.desc, cam_of(done), seed, reg)
                for k in WORK_KEYS:
                    assert getattr(st, k) == cnt[k] - (before[k] if before else 0), (k, done, count)
                before = cnt
        it, _ = ob.render(scene.desc, cam_of(total), seed, reg, ob.ORDER_ITERATIVE)
        assert np.array_equal(out[0], it), "not bit-identical to the oracle"
        return out
    finally:
        acc.close()


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_prefix_equality(torch_cuda, spheres, dev_spheres, counting):
    """randSpheres 48x27 in passes of 1, 2 and 5."""
    cam_of = lambda n: spheres.camera(width=48, spp=n, depth=50)
    cam = cam_of(8)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    _, _, noisy = run_passes(torch_cuda, dev_spheres, spheres, cam_of, 7, reg, (1, 2, 5), ("random_spheres", 1, 48, 50),
                             counting)
    assert 0 < noisy < reg.width * reg.height


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_ragged_tiles(torch_cuda, spheres, dev_spheres, counting):
    """A 17 x 5 region: partial tiles on both edges, a last wave with padded slots only."""
    cam_of = lambda n: spheres.camera(width=64, spp=n, depth=50)
    run_passes(torch_cuda, dev_spheres, spheres, cam_of, 9, rtx.Region(5, 3, 17, 5, 0, 1), (3, 4),
               ("random_spheres", 1, 64, 50), counting)


def test_one_pixel(torch_cuda, spheres, dev_spheres):
    """One pixel, one sample: Q / 1 - S * S is exactly 0; then a second sample."""
    cam_of = lambda n: spheres.camera(width=64, spp=n, depth=50)
    reg = rtx.Region(30, 20, 1, 1, 0, 1)
    acc = dev_spheres.accumulator(cam_of(2), 9, reg)
    acc.add(1, stream_of(torch_cuda))
    rgb, var, noisy = acc.resolve(REL_TOL)
    assert rgb.shape == (1, 1, 3) and (var == 0).all() and noisy == 0
    acc.close()
    run_passes(torch_cuda, dev_spheres, spheres, cam_of, 9, reg, (1, 1), ("random_spheres", 1, 64, 50))


def test_resolve_device_with_partial_waves(torch_cuda, spheres, dev_spheres):
    """rtx_accum_resolve_device on the passes' stream into NaN-filled device buffers: every pixel written, nothing
    past the shard, with and without the variance and the count."""
    torch = torch_cuda
    cam = spheres.camera(width=64, spp=7, depth=50)
    reg = rtx.Region(5, 3, 17, 5, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, 64, 50), spheres.desc, cam, 9, reg, 7)
    want_rgb, want_var, want_noisy = accum_ref.after(col, 7, REL_TOL)
    acc = dev_spheres.accumulator(cam, 9, reg)
    st = stream_of(torch)
    acc.add(3, st)
    acc.add(4, st)
    rgb = torch.full((5 + 1, 17, 3), float("nan"), dtype=torch.float32, device="cuda")
    var = torch.full((5 + 1, 17, 3), float("nan"), dtype=torch.float32, device="cuda")
    assert acc.resolve_device(rgb.data_ptr(), var.data_ptr(), REL_TOL, st, count_noisy=True) == want_noisy
    assert acc.resolve_device(rgb.data_ptr(), var.data_ptr(), REL_TOL, st, count_noisy=True) == want_noisy  # not added up
    assert np.array_equal(rgb[:5].cpu().numpy(), want_rgb) and np.array_equal(var[:5].cpu().numpy(), want_var)
    assert torch.isnan(rgb[5]).all() and torch.isnan(var[5]).all()
    rgb.fill_(float("nan"))
    assert acc.resolve_device(rgb.data_ptr(), 0, REL_TOL, st) is None  # enqueued only, no variance
    torch.cuda.synchronize()
    assert np.array_equal(rgb[:5].cpu().numpy(), want_rgb)
    assert acc.resolve_device(rgb.data_ptr(), 0, 0.0, st, count_noisy=True) == int((want_var.sum(axis=2) > 0).sum())
    acc.close()


def test_passes_across_chunks(torch_cuda, spheres, dev_spheres, monkeypatch):
    """A 1 MiB scratch holds 34 samples of the window's 8 x 5 tiles: passes of 40 and 50 take two chunks each, the
    second pass starting at sample 40, not at a chunk boundary of a one-shot render."""
    monkeypatch.setenv("RTX_SCRATCH_MB", "1")
    monkeypatch.setenv("RTX_ITEM_SUB", "7")
    cam = spheres.camera(width=1920, spp=90, depth=50)
    reg = rtx.Region(1000, 700, 64, 36, 0, 1)
    acc = dev_spheres.accumulator(cam, 17, reg)
    for count in (40, 50):
        st = acc.add(count, stream_of(torch_cuda), stats=True)
        assert st.sample_chunks == 2, st.sample_chunks
        assert st.samples == 64 * 36 * count
    rgb, _, _ = acc.resolve(REL_TOL)
    acc.close()
    one, st1 = gpu_region(torch_cuda, dev_spheres, cam, 17, reg, counters=False)
    assert st1.sample_chunks == 3
    assert np.array_equal(rgb, one)
    it, _ = ob.render(spheres.desc, cam, 17, reg, ob.ORDER_ITERATIVE)
    assert np.array_equal(rgb, it)


@pytest.mark.parametrize("name,width,window,check_var", [
    ("cornell_box", 600, (280, 300, 24, 12), True),       # quads and lights: untiered launch_items
    ("simple_light_demo", 400, (150, 100, 24, 12), True),  # Perlin noise: the NOISE instantiation
    ("stress_100k", 1920, (900, 500, 48, 24), False),      # tiered, from HBM with the LDS cache: no drain
])
def test_every_launch_path(torch_cuda, built, name, width, window, check_var):
    scene = rtx.HostScene(name, 1)
    dev = rtx.DeviceScene(scene.desc)
    cam_of = lambda n: scene.camera(width=width, spp=n)
    run_passes(torch_cuda, dev, scene, cam_of, 23, rtx.Region(*window, 0, 1), (2, 1), (name, 1, width, 0),
               check_var=check_var)
    dev.close()


def test_shards(torch_cuda, spheres, dev_spheres):
    """Accumulators of the two row-interleaved shards, and of the two 8-row-stripe shards (the ST instantiation),
    reassemble by rows to the whole region's resolve."""
    cam = spheres.camera(width=200, spp=4, depth=50)
    H = cam.image_height

    def resolved(reg):
        acc = dev_spheres.accumulator(cam, 5, reg)
        acc.add(2, stream_of(torch_cuda))
        acc.add(2, stream_of(torch_cuda))
        out = acc.resolve(REL_TOL)
        acc.close()
        return out

    full_rgb, full_var, full_noisy = resolved(rtx.Region(0, 0, 200, H, 0, 1))
    one, _ = gpu_region(torch_cuda, dev_spheres, cam, 5, rtx.Region(0, 0, 200, H, 0, 1), counters=False)
    assert np.array_equal(full_rgb, one)
    for stripe in (0, 8):
        rgb, var, noisy = np.full_like(full_rgb, np.nan), np.full_like(full_var, np.nan), 0
        for rank in range(2):
            reg = rtx.Region(0, 0, 200, H, rank, 2, stripe)
            r, v, n = resolved(reg)
            rows = [accum_ref.shard_row(reg, i) for i in range(rtx.region_rows(reg))]
            rgb[rows], var[rows], noisy = r, v, noisy + n
        assert np.array_equal(rgb, full_rgb) and np.array_equal(var, full_var), stripe
        assert noisy == full_noisy


def test_isolation_and_reset(torch_cuda, spheres, dev_spheres):
    """S and Q belong to the accumulator: a one-shot render of another camera between two passes, and freeing the
    device's scratch, leave them alone; the scratch never holds them; reset starts over with the same bits."""
    torch = torch_cuda
    cam_of = lambda n: spheres.camera(width=48, spp=n, depth=50)
    cam = cam_of(5)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    torch.cuda.synchronize()
    rtx.release_device_memory(0)
    assert rtx.device_scratch_bytes(0) == 0
    acc = dev_spheres.accumulator(cam, 7, reg)
    assert rtx.device_scratch_bytes(0) == 0
    slots = ((48 + 7) // 8) * ((27 + 7) // 8) * 64  # 8 x 8 tiles, ragged ones padded
    L = rtx.load()
    assert L.rtx_accum_resolve(acc._h, None, None, 0.0, None) == rtx.RTX_ERR_INVALID_ARG
    buf = np.zeros((27, 48, 3), np.float32)
    assert L.rtx_accum_resolve(acc._h, buf.ctypes.data_as(ctypes.c_void_p), None, 0.0, None) == rtx.RTX_ERR_INVALID_ARG
    assert b"nothing accumulated" in L.rtx_last_error()
    assert L.rtx_accum_add(acc._h, 0, None, 0, None) == rtx.RTX_ERR_INVALID_ARG

    def passes():
        rtx.release_device_memory(0)
        acc.add(2, stream_of(torch))
        assert rtx.device_scratch_bytes(0) == slots * 12 * 2  # two samples' colours: S and Q (24 B a slot) are not in it
        other = spheres.camera(width=400, spp=3, depth=50)
        gpu_region(torch, dev_spheres, other, 11, rtx.Region(100, 60, 64, 40, 0, 1), counters=False)
        rtx.release_device_memory(0)
        assert L.rtx_accum_add(acc._h, 0xFFFFFFFF, None, 0, None) == rtx.RTX_ERR_INVALID_ARG  # 2 + 2^32 - 1 wraps
        acc.add(3, stream_of(torch))
        assert acc.samples == 5
        return acc.resolve(REL_TOL)

    rgb, var, noisy = passes()
    one, _ = gpu_region(torch, dev_spheres, cam, 7, reg, counters=False)
    assert np.array_equal(rgb, one)
    want = accum_ref.after(accum_ref.sample_colours(("random_spheres", 1, 48, 50), spheres.desc, cam_of(8), 7, reg, 8),
                           5, REL_TOL)
    assert np.array_equal(var, want[1]) and noisy == want[2]
    again = acc.resolve(REL_TOL)  # a resolve does not modify the accumulator
    assert np.array_equal(again[0], rgb) and np.array_equal(again[1], var) and again[2] == noisy
    acc.reset()
    assert acc.samples == 0
    rgb2, var2, noisy2 = passes()
    assert np.array_equal(rgb2, rgb) and np.array_equal(var2, var) and noisy2 == noisy
    acc.close()
    rtx.device_check(0)


def test_ppm(torch_cuda, spheres, dev_spheres):
    cam = spheres.camera(width=48, spp=5, depth=50)
    acc = dev_spheres.accumulator(cam, 7, rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1))
    acc.add(3, stream_of(torch_cuda))
    acc.add(2, stream_of(torch_cuda))
    text = acc.ppm()
    acc.close()
    assert text.startswith(b"P3\n48 27\n255\n")
    assert text == dev_spheres.render_ppm(cam, 7)


def test_go_render_progressive_sequence(torch_cuda, spheres, dev_spheres):
    """The C-ABI calls of go/internal/render_gpu.go RenderProgressive, in its order and with its arguments: passes on
    the default stream, the noisy count alone after each (no image copied), a stop at noisy == 0 or at
    samplesPerPixel, then the PPM and one rtx_device_check.  The bytes are Render's at the samples done."""
    L = rtx.load()
    cam = spheres.camera(width=48, spp=7, depth=50)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, 48, 50), spheres.desc, cam, 7, reg, 8)
    for tol, stops_early in ((0.0, False), (1.0e3, True)):
        acc = ctypes.c_void_p()
        assert L.rtx_accum_create(dev_spheres.handle, ctypes.byref(cam), 7, ctypes.byref(reg), ctypes.byref(acc)) == 0
        done, seen = 0, []
        while done < cam.samples_per_pixel:
            count = min(3, cam.samples_per_pixel - done)
            assert L.rtx_accum_add(acc, count, None, 0, None) == 0
            done = L.rtx_accum_samples(acc)
            noisy = ctypes.c_uint64(1 << 40)
            assert L.rtx_accum_resolve(acc, None, None, tol, ctypes.byref(noisy)) == 0
            assert noisy.value == accum_ref.after(col, done, tol)[2]
            seen.append((done, noisy.value))
            if tol > 0 and noisy.value == 0:
                break
        assert [d for d, _ in seen] == ([3] if stops_early else [3, 6, 7]), seen
        cap = int(L.rtx_ppm_max_bytes(48, 27))
        buf = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_uint64()
        assert L.rtx_accum_ppm(acc, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)) == 0
        assert L.rtx_device_check(0) == 0
        L.rtx_accum_destroy(acc)
        assert buf[: n.value].tobytes() == dev_spheres.render_ppm(spheres.camera(width=48, spp=done, depth=50), 7)
