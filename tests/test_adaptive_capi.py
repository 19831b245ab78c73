"""Adaptive sampling on the CPU (include/rtx.h, "adaptive sampling"): the refusals that come before any device call,
the Python wrappers against the header's prototypes, and the test reference itself (adaptive_ref.py) held to
accum_ref where nothing closes and to its own stated rule on the two workloads the GPU tests run."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import accum_ref
import adaptive_ref
import rtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "rtx.h")).read()


def stand_in_accumulator():
    """Zeroed memory standing for an accumulator: the argument checks fail before it is looked at beyond its sample
    count, which reads as 0."""
    buf = ctypes.create_string_buffer(8192)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_refusals_come_before_any_device_call(built):
    L = rtx.load()
    E = rtx.RTX_ERR_INVALID_ARG
    st, ad = rtx.Stats(), rtx.AdaptStats()
    assert L.rtx_accum_add_adaptive(None, 4, 0.1, 4, None, 0, ctypes.byref(st), ctypes.byref(ad)) == E
    assert b"accumulator" in L.rtx_last_error()
    keep, acc = stand_in_accumulator()
    assert L.rtx_accum_add_adaptive(acc, 0, 0.1, 4, None, 0, None, None) == E
    assert b"0 samples" in L.rtx_last_error()
    for bad in (-0.5, float("nan"), -float("inf")):
        assert L.rtx_accum_add_adaptive(acc, 4, bad, 4, None, 0, None, None) == E
        assert b"rel_tol" in L.rtx_last_error()
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.rtx_accum_tile_shape(None, ctypes.byref(w), ctypes.byref(h)) == E
    assert L.rtx_accum_tile_shape(acc, None, ctypes.byref(h)) == E
    assert L.rtx_accum_sample_counts(None, keep) == E
    assert L.rtx_accum_sample_counts_device(None, keep, None) == E
    assert b"accumulator" in L.rtx_last_error()
    assert rtx.load().rtx_version() == 10  # additive: the ABI version stays


def test_wrappers_match_the_header(built):
    flat = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")]
              for m in re.finditer(r"\bint\s+(rtx_accum_\w+)\(([^)]*)\);", flat)}
    L = rtx.load()
    for name in ("rtx_accum_add_adaptive", "rtx_accum_tile_shape", "rtx_accum_sample_counts_device",
                 "rtx_accum_sample_counts"):
        assert name in rtx.RTX_SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(protos[name]), name
    assert [a.split()[-1].lstrip("*") for a in protos["rtx_accum_add_adaptive"]] == [
        "accum", "count", "rel_tol", "min_samples", "hip_stream", "flags", "stats", "adapt_stats"]
    assert L.rtx_accum_add_adaptive.argtypes[2] is ctypes.c_float
    m = re.search(r"typedef struct rtx_adapt_stats\s*\{(.*?)\}", flat, re.S)
    assert re.findall(r"uint64_t\s+(\w+);", m.group(1)) == [n for n, _ in rtx.AdaptStats._fields_]
    assert ctypes.sizeof(rtx.AdaptStats) == 24
    sig = inspect.signature(rtx.Accumulator.add_adaptive)
    assert list(sig.parameters)[:7] == ["self", "count", "rel_tol", "min_samples", "stream", "stats", "counters"]
    for name in ("sample_counts", "sample_counts_device", "tile_shape"):
        assert hasattr(rtx.Accumulator, name)


@pytest.fixture(scope="module")
def spheres(built):
    return rtx.HostScene("random_spheres", seed=1)


def test_reference_with_nothing_closing_is_the_uniform_fold(spheres):
    """min_samples above the frontier: no tile closes, and the adaptive reference is accum_ref.after."""
    cam = spheres.camera(width=64, spp=7, depth=50)
    reg = rtx.Region(5, 3, 17, 5, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, 64, 50), spheres.desc, cam, 9, reg, 7)
    res = adaptive_ref.simulate(col, (8, 8), (3, 4), 0.1, min_samples=100)
    assert (res.counts == 7).all() and res.n == 7
    assert [p[:2] for p in res.passes] == [(3, 85), (3, 85)]
    want = accum_ref.after(col, 7, 0.1)
    got = res.resolved(0.1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_reference_on_the_ragged_region(spheres):
    """The workload of the GPU tests' ragged case, by the rule rtx.h states: at rel_tol = 0.1 the three tiles of the
    17 x 5 region end at 4, 12 and 16 samples; at 0.2 all three close at 4 and passes 2-4 sample nothing while the
    frontier goes on to 16."""
    cam = spheres.camera(width=64, spp=16, depth=50)
    reg = rtx.Region(5, 3, 17, 5, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, 64, 50), spheres.desc, cam, 9, reg, 16)
    res = adaptive_ref.simulate(col, (8, 8), (4, 4, 4, 4), 0.1, min_samples=4)
    per_tile = sorted(int(res.counts[t].max()) for t in adaptive_ref.tiles(5, 17, (8, 8)))
    assert per_tile == [4, 12, 16], per_tile
    for t in adaptive_ref.tiles(5, 17, (8, 8)):  # a tile closes whole
        assert (res.counts[t] == res.counts[t].max()).all()
    # a pixel with n_p samples is the uniform fold's pixel at n_p
    for v in np.unique(res.counts):
        want = accum_ref.after(col, int(v), 0.1)
        got = res.resolved(0.1)
        assert np.array_equal(got[0][res.counts == v], want[0][res.counts == v])
        assert np.array_equal(got[1][res.counts == v], want[1][res.counts == v])
    res = adaptive_ref.simulate(col, (8, 8), (4, 4, 4, 4), 0.2, min_samples=4)
    assert (res.counts == 4).all() and res.n == 16
    assert [p[:2] for p in res.passes] == [(3, 85), (0, 0), (0, 0), (0, 0)]
    assert np.array_equal(res.resolved(0.2)[0], accum_ref.after(col, 4, 0.2)[0])
