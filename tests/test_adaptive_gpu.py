"""Adaptive sampling on the GPU (rtx_accum_add_adaptive, include/rtx.h "adaptive sampling").  After any
adaptive passes: the map of samples per pixel, every pass's open tiles and pixels, and the resolved image, variance and
noisy count are the numpy reference's (adaptive_ref.py) bit for bit; the pixels with n_p samples are those pixels of a
one-shot render at samples_per_pixel = n_p; and the counting instantiation's work counters are the oracle's for exactly
the samples each pass rendered."""
import ctypes

import numpy as np
import pytest

import accum_ref
import adaptive_ref
import rtx
from parity import PATH_KEYS, WORK_KEYS, gpu_region

pytestmark = pytest.mark.gpu

PASSES = (4, 4, 4, 4)


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


def spheres_case(spheres):
    """Case 1: randSpheres 48 x 27, seed 7, depth 50 — (cam_of, region, colours of 16 samples)."""
    cam_of = lambda n: spheres.camera(width=48, spp=n, depth=50)
    cam = cam_of(16)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    return cam_of, reg, accum_ref.sample_colours(("random_spheres", 1, 48, 50), spheres.desc, cam, 7, reg, 16)


def uniform_reference(torch, dev, cam_of, seed, reg, passes, rel_tol, min_samples, tile_shape, flags=0):
    """adaptive_ref.simulate without the oracle, for scenes it is too slow on: the selection from the image and variance
    a UNIFORM accumulator (rtx_accum_add, held to the oracle by test_accum_gpu.py) resolves at every pass boundary, by
    resolve's own float32 test; the expected pixel at n_p samples is the uniform accumulator's at n_p.
    Returns (counts, rgb, var, [(open_tiles, open_pixels)])."""
    F = np.float32
    rows, width = rtx.region_rows(reg), reg.width
    tl = adaptive_ref.tiles(rows, width, tile_shape)
    acc = dev.accumulator(cam_of(sum(passes)), seed, reg)
    closed = np.zeros((rows, width), np.uint32)
    at, n, per_pass = {}, 0, []
    for count in passes:
        if n >= max(min_samples, 1):
            rgb, var, _ = at[n] = acc.resolve(rel_tol)[:2] + (None,)
            sv = (var[..., 0] + var[..., 1]) + var[..., 2]
            mb = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
            t = F(rel_tol) * np.where(mb > F(0.01), mb, F(0.01)).astype(F)
            noisy = sv > t * t
            for ti in tl:
                if (closed[ti] == 0).all() and not noisy[ti].any():
                    closed[ti] = n
        is_open = closed == 0
        per_pass.append((sum(1 for ti in tl if is_open[ti].all()), int(is_open.sum())))
        acc.add(count, stream_of(torch), flags=flags)
        n += count
    at[n] = acc.resolve(rel_tol)[:2] + (None,)
    acc.close()
    counts = np.where(closed == 0, np.uint32(n), closed).astype(np.uint32)
    rgb, var = np.zeros((rows, width, 3), F), np.zeros((rows, width, 3), F)
    for v in np.unique(counts):
        rgb[counts == v], var[counts == v] = at[int(v)][0][counts == v], at[int(v)][1][counts == v]
    return counts, rgb, var, per_pass


def run_adaptive(torch, dev, cam_of, seed, reg, passes, rel_tol, min_samples, col=None, counting=False, flags=0,
                 pass_counts=None, count_keys=PATH_KEYS, acc=None):
    """The passes on a new accumulator (or on `acc`, reset by the caller) and every check of the module docstring; col:
    accum_ref.sample_colours of the region (None: the reference from uniform passes on the GPU).  Returns
    (counts, rgb, var, noisy, [(open_tiles, open_pixels)])."""
    total = sum(passes)
    own = acc is None
    acc = acc or dev.accumulator(cam_of(total), seed, reg)
    try:
        shape = acc.tile_shape
        assert shape[0] * shape[1] == 64
        n_tiles = len(adaptive_ref.tiles(rtx.region_rows(reg), reg.width, shape))
        if col is not None:
            ref = adaptive_ref.simulate(col, shape, passes, rel_tol, min_samples)
            want_counts, want_pass = ref.counts, [p[:2] for p in ref.passes]
            want_rgb, want_var, want_noisy = ref.resolved(rel_tol)
        else:
            want_counts, want_rgb, want_var, want_pass = uniform_reference(torch, dev, cam_of, seed, reg, passes, rel_tol,
                                                                           min_samples, shape, flags)
            want_noisy = None
        assert acc.samples == 0 and (acc.sample_counts() == 0).all()
        done, seen = 0, []
        for i, count in enumerate(passes):
            st, ad = acc.add_adaptive(count, rel_tol, min_samples, stream_of(torch), counters=counting, flags=flags)
            done += count
            seen.append((int(ad.open_tiles), int(ad.open_pixels)))
            print(f"pass {i}: frontier {done}, open tiles {ad.open_tiles} of {ad.tiles}, open pixels {ad.open_pixels}, "
                  f"samples {st.samples}, {st.kernel_ms:.3f} ms")
            assert acc.samples == done  # the frontier, whether or not a tile was open
            assert ad.tiles == n_tiles
            assert seen[-1] == want_pass[i], (i, seen[-1], want_pass[i])
            assert st.samples == ad.open_pixels * count, (st.samples, ad.open_pixels, count)
            if pass_counts is not None:
                for k in count_keys:
                    assert getattr(st, k) == pass_counts[i][k], (k, i, getattr(st, k), pass_counts[i][k])
        counts = acc.sample_counts()
        assert counts.dtype == np.uint32 and np.array_equal(counts, want_counts), "the count map differs from the reference"
        dcounts = torch.full((rtx.region_rows(reg) + 1, reg.width), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        acc.sample_counts_device(dcounts.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert np.array_equal(dcounts[:-1].cpu().numpy().view(np.uint32), counts) and (dcounts[-1] == 0x7FFFFFFF).all()
        rgb, var, noisy = acc.resolve(rel_tol)
        assert np.array_equal(rgb, want_rgb), "the resolved image differs from the reference"
        assert np.array_equal(var, want_var), "the variance differs from the reference"
        if want_noisy is not None:
            assert noisy == want_noisy, (noisy, want_noisy)
        for v in np.unique(counts):  # the exact contract: a pixel with n_p samples is the one-shot render's at n_p
            one, _ = gpu_region(torch, dev, cam_of(int(v)), seed, reg, counters=False, flags=flags)
            m = counts == v
            assert np.array_equal(rgb[m], one[m]), f"pixels with {v} samples differ from the one-shot render at {v}"
        rtx.device_check(0)
        return counts, rgb, var, noisy, seen
    finally:
        if own:
            acc.close()


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_rand_spheres(torch_cuda, spheres, dev_spheres, counting):
    """Case 1: four passes of 4, min_samples = 4, rel_tol = 0.3, 8 x 8 tiles (24, the bottom row ragged).  The oracle
    simulation of the rule in rtx.h: 24, 21, 13 and 9 tiles open in the four passes; counts 4, 8, 12 and 16 all occur.
    Counting: the path counters (samples, segments, hits, texel fetches, draws) of every pass are the oracle's sums over
    exactly the open pixels and the pass's samples (the scene walks its own tree: the box and primitive tests are
    compared on the caller's tree below)."""
    cam_of, reg, col = spheres_case(spheres)
    want = None
    if counting:
        cnt = adaptive_ref.sample_counters(("random_spheres", 1, 48, 50), spheres.desc, cam_of(16), 7, reg, 16)
        acc = dev_spheres.accumulator(cam_of(16), 7, reg)
        shape = acc.tile_shape
        acc.close()
        want = adaptive_ref.pass_counters(cnt, adaptive_ref.simulate(col, shape, PASSES, 0.3, 4), PASSES)
    counts, _, _, _, seen = run_adaptive(torch_cuda, dev_spheres, cam_of, 7, reg, PASSES, 0.3, 4, col, counting,
                                         pass_counts=want)
    # the condition of the case, not a measurement: at least three distinct counts, an open and a closed tile at the end
    assert len(np.unique(counts)) >= 3 and 0 < seen[-1][0] < 24, (np.unique(counts), seen)
    assert [s[0] for s in seen] == [24, 21, 13, 9], seen
    assert sorted(np.unique(counts)) == [4, 8, 12, 16]


def test_rand_spheres_counters_on_the_callers_tree(torch_cuda, spheres):
    """Case 1's counting run on a scene that walks the caller's tree with every box test (RTX_SCENE_REFERENCE_BVH |
    RTX_SCENE_EVERY_BOX): node_visits and prim_tests are the oracle's sums too."""
    cam_of, reg, col = spheres_case(spheres)
    dev = rtx.DeviceScene(spheres.desc, reference_bvh=True, every_box=True)
    try:
        cnt = adaptive_ref.sample_counters(("random_spheres", 1, 48, 50), spheres.desc, cam_of(16), 7, reg, 16)
        acc = dev.accumulator(cam_of(16), 7, reg)
        shape = acc.tile_shape
        acc.close()
        want = adaptive_ref.pass_counters(cnt, adaptive_ref.simulate(col, shape, PASSES, 0.3, 4), PASSES)
        run_adaptive(torch_cuda, dev, cam_of, 7, reg, PASSES, 0.3, 4, col, counting=True, pass_counts=want,
                     count_keys=WORK_KEYS)
    finally:
        dev.close()


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_ragged_and_empty(torch_cuda, spheres, dev_spheres, counting):
    """Case 2: region (5, 3, 17, 5) of the width-64 camera, seed 9: three partial tiles.  At rel_tol = 0.1 they end at
    4, 12 and 16; at 0.2 all three close at 4 and passes 2-4 sample nothing — and complete: the frontier goes on to 16,
    the counts stay 4, the image is the one-shot render's at 4 samples, the device reports no error."""
    cam_of = lambda n: spheres.camera(width=64, spp=n, depth=50)
    reg = rtx.Region(5, 3, 17, 5, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, 64, 50), spheres.desc, cam_of(16), 9, reg, 16)
    counts, _, _, _, seen = run_adaptive(torch_cuda, dev_spheres, cam_of, 9, reg, PASSES, 0.1, 4, col, counting)
    assert sorted(int(counts[t].max()) for t in adaptive_ref.tiles(5, 17, (8, 8))) == [4, 12, 16]
    acc = dev_spheres.accumulator(cam_of(16), 9, reg)
    try:
        counts, rgb, _, _, seen = run_adaptive(torch_cuda, dev_spheres, cam_of, 9, reg, PASSES, 0.2, 4, col, counting, acc=acc)
        assert seen == [(3, 85), (0, 0), (0, 0), (0, 0)], seen
        assert acc.samples == 16 and (counts == 4).all()
        one, _ = gpu_region(torch_cuda, dev_spheres, cam_of(4), 9, reg, counters=False)
        assert np.array_equal(rgb, one)
        st, ad = acc.add_adaptive(4, 0.2, 4, stream_of(torch_cuda), counters=counting)  # one more empty pass
        assert ad.open_tiles == 0 and ad.open_pixels == 0 and st.samples == 0 and acc.samples == 20
        if counting:
            assert st.segments == 0 and st.rng_draws == 0
        rtx.device_check(0)
    finally:
        acc.close()


@pytest.mark.parametrize("env,flags,no_tier", [
    ({}, 0, False),                          # tiered, scene in LDS, camera-ray pool, drain
    ({"RTX_CAM_POOL": "0"}, 0, False),       # not pooled
    ({"RTX_DRAIN": "0"}, 0, False),          # the far pass's own launch
    ({}, rtx.RTX_FLAG_NO_LDS, False),        # the scene read from HBM
    ({}, 0, True),                           # one walk (untiered), pooled
    ({"RTX_CAM_POOL": "0"}, 0, True),        # one walk, not pooled
], ids=["tiered-pool-drain", "tiered-nopool", "tiered-nodrain", "hbm", "untiered-pool", "untiered-nopool"])
def test_launch_paths_of_the_sphere_scene(torch_cuda, spheres, env, flags, no_tier, monkeypatch):
    """Case 1 on the launch paths of a sphere scene: the claim's indirection in each instantiation."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam_of, reg, col = spheres_case(spheres)
    dev = rtx.DeviceScene(spheres.desc, no_tier=no_tier)
    try:
        _, _, _, _, seen = run_adaptive(torch_cuda, dev, cam_of, 7, reg, PASSES, 0.3, 4, col, flags=flags)
        assert [s[0] for s in seen] == [24, 21, 13, 9], seen
    finally:
        dev.close()


@pytest.mark.parametrize("name,width,window,rel_tol,use_oracle", [
    ("cornell_box", 600, (280, 300, 24, 12), 0.3, True),        # quads and lights: untiered launch_items
    ("simple_light_demo", 400, (150, 100, 24, 12), 0.3, True),  # Perlin noise: the NOISE instantiation
    ("stress_100k", 1920, (900, 500, 48, 24), 0.3, False),      # tiered, from HBM with the LDS cache: no drain
])
def test_other_scenes(torch_cuda, built, name, width, window, rel_tol, use_oracle):
    """Quads, Perlin noise and a scene in HBM with the LDS cache, at test_accum_gpu.py's windows: three passes of 4."""
    scene = rtx.HostScene(name, 1)
    dev = rtx.DeviceScene(scene.desc)
    cam_of = lambda n: scene.camera(width=width, spp=n)
    reg = rtx.Region(*window, 0, 1)
    passes = (4, 4, 4)
    col = accum_ref.sample_colours((name, 1, width, 0), scene.desc, cam_of(12), 23, reg, 12) if use_oracle else None
    try:
        counts, _, _, _, seen = run_adaptive(torch_cuda, dev, cam_of, 23, reg, passes, rel_tol, 4, col)
        if use_oracle:  # (the oracle's simulation: one of the six tiles closes at 4, five stay open)
            assert [s[0] for s in seen] == [6, 5, 5] and sorted(np.unique(counts)) == [4, 12], (seen, np.unique(counts))
    finally:
        dev.close()


def test_chunks(torch_cuda, spheres, dev_spheres, monkeypatch):
    """A 1 MiB scratch holds 34 samples of the window's 8 x 5 tiles (test_accum_gpu.py's knob): passes of 40 and 50 take
    two chunks each, the selection running once per pass — the same map and bits as the same passes in one chunk."""
    cam_of = lambda n: spheres.camera(width=1920, spp=n, depth=50)
    reg = rtx.Region(1000, 700, 64, 36, 0, 1)

    def passes():
        acc = dev_spheres.accumulator(cam_of(90), 17, reg)
        chunks = []
        for count in (40, 50):
            st, ad = acc.add_adaptive(count, 0.1, 40, stream_of(torch_cuda))
            chunks.append(int(st.sample_chunks))
            assert st.samples == ad.open_pixels * count
        out = (acc.sample_counts(),) + acc.resolve(0.1) + (chunks,)
        acc.close()
        return out

    one = passes()
    monkeypatch.setenv("RTX_SCRATCH_MB", "1")
    monkeypatch.setenv("RTX_ITEM_SUB", "7")
    two = passes()
    assert one[4] == [1, 1] and two[4] == [2, 2], (one[4], two[4])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert one[3] == two[3]
    print("counts:", dict(zip(*np.unique(one[0], return_counts=True))))
    for v in np.unique(one[0]):
        ref, _ = gpu_region(torch_cuda, dev_spheres, cam_of(int(v)), 17, reg, counters=False)
        assert np.array_equal(two[1][one[0] == v], ref[one[0] == v])


@pytest.mark.parametrize("stripe", [0, 8], ids=["rows", "stripes"])
@pytest.mark.parametrize("rank", [0, 1])
def test_shards(torch_cuda, spheres, dev_spheres, rank, stripe):
    """world = 2: each rank's shard selects on its own tiles (of its compacted rows) and equals the reference for it."""
    cam_of = lambda n: spheres.camera(width=48, spp=n, depth=50)
    cam = cam_of(16)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, rank, 2, stripe)
    col = accum_ref.sample_colours(("random_spheres", 1, 48, 50), spheres.desc, cam, 7, reg, 16)
    counts, _, _, _, seen = run_adaptive(torch_cuda, dev_spheres, cam_of, 7, reg, PASSES, 0.3, 4, col)
    assert len(np.unique(counts)) >= 2, np.unique(counts)


def test_life_cycle(torch_cuda, spheres, dev_spheres):
    """rtx_accum_add is refused after an adaptive pass until a reset; the reset reopens every tile and the same passes
    give the same result; n + count past 2^32 - 1 is refused."""
    cam_of, reg, col = spheres_case(spheres)
    L = rtx.load()
    acc = dev_spheres.accumulator(cam_of(16), 7, reg)
    try:
        acc.add(2, stream_of(torch_cuda))  # uniform passes first are fine
        acc.reset()
        first = run_adaptive(torch_cuda, dev_spheres, cam_of, 7, reg, PASSES, 0.3, 4, col, acc=acc)
        assert L.rtx_accum_add(acc._h, 1, None, 0, None) == rtx.RTX_ERR_INVALID_ARG
        assert b"adaptive" in L.rtx_last_error()
        assert L.rtx_accum_add_adaptive(acc._h, 0xFFFFFFFF, 0.3, 4, None, 0, None, None) == rtx.RTX_ERR_INVALID_ARG
        assert acc.samples == 16
        acc.reset()
        assert acc.samples == 0
        again = run_adaptive(torch_cuda, dev_spheres, cam_of, 7, reg, PASSES, 0.3, 4, col, acc=acc)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[4] == again[4]
        acc.reset()
        acc.add(3, stream_of(torch_cuda))  # and uniform passes again after the reset
        assert (acc.sample_counts() == 3).all()
        one, _ = gpu_region(torch_cuda, dev_spheres, cam_of(3), 7, reg, counters=False)
        assert np.array_equal(acc.resolve(0.3)[0], one)
    finally:
        acc.close()


def test_preview_of_an_adaptive_accumulator(torch_cuda, spheres, dev_spheres):
    """rtx_accum_preview_device on an adaptive accumulator is its resolve (every pixel at its n_p), the guides over
    [0, min(n, guide_samples)) and the filter, composed by hand; the PPM is the resolved image's."""
    torch = torch_cuda
    cam_of, reg, _ = spheres_case(spheres)
    cam = cam_of(16)
    w, h = reg.width, reg.height
    st = stream_of(torch)
    acc = dev_spheres.accumulator(cam, 7, reg)
    try:
        for count in PASSES:
            acc.add_adaptive(count, 0.3, 4, st, stats=False)
        assert len(np.unique(acc.sample_counts())) >= 3
        rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        var = torch.zeros_like(rgb)
        acc.resolve_device(rgb.data_ptr(), var.data_ptr(), 0.0, st)
        guides = torch.zeros((w * h * 32,), dtype=torch.uint8, device="cuda")
        dev_spheres.guides_device(cam, 7, reg, 0, 4, guides.data_ptr(), st)
        wb = rtx.denoise_workspace_bytes(w, h)
        work = torch.zeros((wb,), dtype=torch.uint8, device="cuda")
        out = torch.zeros_like(rgb)
        rtx.denoise_device(rgb.data_ptr(), var.data_ptr(), guides.data_ptr(), w, h, out.data_ptr(), work.data_ptr(), wb, None, st)
        prev = torch.zeros_like(rgb)
        acc.preview_device(prev.data_ptr(), 4, None, st)
        torch.cuda.synchronize()
        assert prev.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
        assert acc.preview(4).tobytes() == out.cpu().numpy().tobytes()
        assert acc.ppm() == b"P3\n%d %d\n255\n" % (w, h) + rtx.ppm_encode(rgb.cpu().numpy())
    finally:
        acc.close()
