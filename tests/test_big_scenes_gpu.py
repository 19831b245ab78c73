"""The render kernels that read the scene from HBM — with the LDS cache of its hot entries (render_items<HYB>) and
without — on the scenes of tests/big_scenes.py, whose preconditions tests/test_big_scenes.py checks on the CPU.

Every case goes through parity.check_scene: the timed and the counting kernel bit-identical to the oracle's iterative
order on the walked tree, the counting kernel's seven work counters the oracle's, the image within 1e-4 of the
reference order.  Each case also asserts what shows that the intended path ran: rtx_stats.scene_placement, the tier
bit of walk_layout, the cache hits, the waves per workgroup of the launch line (RTX_DEBUG_LAUNCH).

RTX_HOT_ENTRIES and RTX_HOT_BY_READS are read when a layout is uploaded, on a scene's first render: the tests set them
before they make the scene.
"""
import re

import numpy as np
import pytest

import accum_ref
import adaptive_ref
import big_scenes as bs
import rtx
from parity import PATH_KEYS, check_scene, gpu_region
from test_accum_gpu import run_passes
from test_adaptive_gpu import run_adaptive
from test_big_scenes import ADAPT_TOL, SEED

pytestmark = pytest.mark.gpu

LDS, CACHE, HBM = rtx.RTX_SCENE_IN_LDS, rtx.RTX_SCENE_LDS_CACHE, rtx.RTX_SCENE_IN_HBM


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


def region(name, rank=0, world=1, stripe=0):
    return rtx.Region(*bs.window(name), rank, world, stripe)


def waves_of(err: str):
    """Waves per workgroup of every launch line in `err`: (waves,) of an untiered launch, (near, far) of a tiered one."""
    return [tuple(int(w) for w in m.group(1).split(" / ")) for m in re.finditer(r"waves/wg (\d+(?: / \d+)?),", err)]


def checked(torch, name, cam, reg, capfd=None, monkeypatch=None, **scene_flags):
    """check_scene on a scene made here (so that it takes the environment's hot-set knobs); (image, counting stats,
    launch lines' waves)."""
    b = bs.scene(name)
    dev = rtx.DeviceScene(b.desc, **scene_flags)
    try:
        if capfd is not None:
            monkeypatch.setenv("RTX_DEBUG_LAUNCH", "1")
            capfd.readouterr()
        img, st, _ = check_scene(torch, dev, b.desc, cam, SEED, reg)
        waves = waves_of(capfd.readouterr().err) if capfd is not None else None
        return img, st, waves
    finally:
        dev.close()


def assert_cached(st, waves, want_waves):
    """The LDS cache ran: some entries came from it and some from HBM, in workgroups of want_waves waves."""
    assert st.scene_placement == CACHE, st.scene_placement
    assert 0 < st.cache_hits < st.node_visits + st.prim_tests, (st.cache_hits, st.node_visits, st.prim_tests)
    assert waves and all(w == (want_waves,) for w in waves), waves


@pytest.mark.parametrize("axis_aligned", [False, True], ids=["random", "axis"])
def test_mixed_lds_cache(torch_cuda, built, monkeypatch, capfd, axis_aligned):
    """Quads, emitters, image texels and nested Worlds through render_items<QUADS, HYB> in 12-wave workgroups: the
    quad table, the materials and the textures read from global memory beside an LDS cache of 2560 entries."""
    _, st, waves = checked(torch_cuda, "mixed", bs.camera("mixed", axis_aligned), region("mixed"), capfd, monkeypatch)
    assert_cached(st, waves, 12)
    assert st.texel_fetches > 0 and not st.walk_layout & rtx.RTX_LAYOUT_TIERED


def test_mixed_small_cache_8_waves(torch_cuda, built, monkeypatch, capfd):
    monkeypatch.setenv("RTX_HOT_ENTRIES", "832")
    _, st, waves = checked(torch_cuda, "mixed", bs.camera("mixed"), region("mixed"), capfd, monkeypatch)
    assert_cached(st, waves, 8)


def test_mixed_hot_set_by_top_levels(torch_cuda, built, monkeypatch):
    """RTX_HOT_BY_READS=0: the hot set is the tree's top levels, not the most-read entries — another storage order,
    the same image bit for bit."""
    cam, reg = bs.camera("mixed"), region("mixed")
    want, st0, _ = checked(torch_cuda, "mixed", cam, reg)
    monkeypatch.setenv("RTX_HOT_BY_READS", "0")
    got, st, _ = checked(torch_cuda, "mixed", cam, reg)
    assert st.scene_placement == st0.scene_placement == CACHE
    assert 0 < st.cache_hits < st.node_visits + st.prim_tests and st.cache_hits != st0.cache_hits
    assert np.array_equal(got, want)


def test_mixed_without_cache(torch_cuda, built, monkeypatch):
    monkeypatch.setenv("RTX_HOT_ENTRIES", "0")
    _, st, _ = checked(torch_cuda, "mixed", bs.camera("mixed"), region("mixed"))
    assert st.scene_placement == HBM and st.cache_hits == 0


@pytest.mark.parametrize("axis_aligned", [False, True], ids=["random", "axis"])
def test_mixed_noise_from_hbm(torch_cuda, built, axis_aligned):
    """A Perlin texture turns the cache off: the NOISE kernel on a hot-first layout it reads from HBM alone."""
    _, st, _ = checked(torch_cuda, "mixed_noise", bs.camera("mixed_noise", axis_aligned), region("mixed_noise"))
    assert st.scene_placement == HBM and st.cache_hits == 0 and st.texel_fetches > 0


def test_mixed_world_list(torch_cuda, built, capfd, monkeypatch):
    """A World of 2060 primitives: no node, every entry at depth 0, all of them in the cache."""
    _, st, waves = checked(torch_cuda, "mixed_world", bs.camera("mixed_world"), region("mixed_world"), capfd, monkeypatch)
    assert st.scene_placement == CACHE and st.walk_layout == rtx.RTX_LAYOUT_REFERENCE
    assert st.node_visits == 0 and 0 < st.cache_hits <= st.prim_tests
    assert waves and all(w == (12,) for w in waves), waves


@pytest.mark.parametrize("hot", [None, "0"], ids=["cache", "no-cache"])
@pytest.mark.parametrize("no_tier", [False, True], ids=["tiered", "no-tier"])
def test_big_ties(torch_cuda, built, monkeypatch, no_tier, hot):
    """Exact ties through the rank words of a hot-first layout: 'a' halves from LDS byte 0 and 'b' halves from HOT_B
    for the cached entries, both from HBM for the rest — the near and the guarded tree, and the guarded tree alone."""
    if hot is not None:
        monkeypatch.setenv("RTX_HOT_ENTRIES", hot)
    _, st, _ = checked(torch_cuda, "big_ties", bs.camera("big_ties"), region("big_ties"), no_tier=no_tier)
    assert st.scene_placement == (CACHE if hot is None else HBM), st.scene_placement
    assert bool(st.walk_layout & rtx.RTX_LAYOUT_TIERED) == (not no_tier)
    assert (st.cache_hits > 0) == (hot is None)


def test_big_ties_striped_shard(torch_cuda, built):
    """The tiered walk through the cache on one shard of 8-row stripes: the ST instantiations of its three passes."""
    reg = region("big_ties", 1, 2, 8)
    assert 0 < rtx.region_rows(reg) < reg.height
    _, st, _ = checked(torch_cuda, "big_ties", bs.camera("big_ties"), reg)
    assert st.scene_placement == CACHE and st.walk_layout & rtx.RTX_LAYOUT_TIERED and st.cache_hits > 0


def test_split_tier_placed_unalike(torch_cuda, built, monkeypatch):
    """tier_placement's a != b: the near tree fits the LDS copy, the guarded tree does not, so both passes read from
    HBM — the near layout in the small storage order (primitives first, prim_end), the far one hot-first.  Then the
    same with a queue of 64 records and a redo list of 100 ids: the samples that do not fit are rendered again by the
    redo pass over the far layout; the same image, the oracle's path counters."""
    b = bs.scene("split_tier")
    cam, reg = bs.camera("split_tier"), region("split_tier")
    dev = rtx.DeviceScene(b.desc)
    try:
        want, st, cnt = check_scene(torch_cuda, dev, b.desc, cam, SEED, reg)  # (asserts redo_chunks == 0)
        assert st.walk_layout & rtx.RTX_LAYOUT_TIERED and st.scene_placement == HBM
        assert st.deferred_paths > 64 and st.cache_hits == 0, st.deferred_paths
        monkeypatch.setenv("RTX_DEFER_CAP", "64")
        monkeypatch.setenv("RTX_REDO_CAP", "100")
        for counters in (False, True):
            got, s = gpu_region(torch_cuda, dev, cam, SEED, reg, counters=counters)
            assert s.walk_layout & rtx.RTX_LAYOUT_TIERED and s.scene_placement == HBM and s.redo_chunks == 1
            assert np.array_equal(got, want), (counters, int((got != want).any(axis=2).sum()))
            if counters:
                for k in PATH_KEYS:
                    assert getattr(s, k) == cnt[k], (k, getattr(s, k), cnt[k])
    finally:
        dev.close()


@pytest.mark.parametrize("rank,world,stripe", [(1, 2, 8), (1, 3, 0)])
def test_mixed_shards(torch_cuda, built, monkeypatch, capfd, rank, world, stripe):
    """One shard of stripes of 8 rows (the ST instantiations) and one of single rows of three, of the ragged window."""
    reg = region("mixed", rank, world, stripe)
    assert 0 < rtx.region_rows(reg) < reg.height
    _, st, waves = checked(torch_cuda, "mixed", bs.camera("mixed"), reg, capfd, monkeypatch)
    assert_cached(st, waves, 12)


CHUNK_SPP = 192


def test_mixed_sample_chunks(torch_cuda, built, monkeypatch):
    """A 1 MB scratch holds 91 samples of the window's 15 tiles (11 520 B each), so 192 samples per pixel run in three
    chunks whose sums are carried in the output; still the oracle's bits.  (RTX_SCRATCH_MB has no smaller value, and
    24 samples would fit one chunk.)"""
    monkeypatch.setenv("RTX_SCRATCH_MB", "1")
    _, st, _ = checked(torch_cuda, "mixed", bs.camera("mixed", spp=CHUNK_SPP), region("mixed"))
    assert st.sample_chunks > 2 and st.scene_placement == CACHE


@pytest.mark.parametrize("counting", [False, True], ids=["timed", "counting"])
def test_mixed_accumulator(torch_cuda, built, counting):
    """add(2), add(2): after each pass the resolve is the one-shot render's bit for bit, the image, variance and noisy
    count are those of accum_ref.fold's S and Q, and the counting passes' counters are the oracle's."""
    b = bs.scene("mixed")
    dev = rtx.DeviceScene(b.desc)
    try:
        run_passes(torch_cuda, dev, b, lambda n: bs.camera("mixed", spp=n), SEED, region("mixed"), (2, 2),
                   ("big_scenes.mixed", bs.SEED, bs.CAM_SEED), counting)
    finally:
        dev.close()


def test_mixed_adaptive_pass(torch_cuda, built):
    """A pass of 4 samples with every tile open, then one adaptive pass (render_items<ADAPT> over the open tiles'
    list, with the cache): the open tiles, the sample counts, the image and the variance are adaptive_ref's, and the
    pixels of the closed tiles are the one-shot render's at 4 samples, those of the open ones at 8."""
    b = bs.scene("mixed")
    reg = region("mixed")
    cam_of = lambda n: bs.camera("mixed", spp=n)  # noqa: E731
    col = accum_ref.sample_colours(("big_scenes.mixed", bs.SEED, bs.CAM_SEED), b.desc, cam_of(8), SEED, reg, 8)
    dev = rtx.DeviceScene(b.desc)
    try:
        counts, _, _, _, seen = run_adaptive(torch_cuda, dev, cam_of, SEED, reg, (4, 4), ADAPT_TOL, 4, col)
    finally:
        dev.close()
    tiles = len(adaptive_ref.tiles(rtx.region_rows(reg), reg.width, (8, 8)))
    assert seen[0][0] == tiles and 0 < seen[1][0] < tiles, seen  # the case's condition: a closed and an open tile
    assert sorted(np.unique(counts)) == [4, 8]


def test_device_is_clean(torch_cuda, built):
    """Last: no render of this module failed in its kernel (watchdog, partial-wave claim)."""
    rtx.device_check(0)
