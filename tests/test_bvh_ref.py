"""tests/bvh_ref.py (the independent NewBVHFromWorld) proven on the CPU before a GPU test relies on it: against the host
mirror's trees of four main.go scenes, on trees worked out by hand, and rtx_scene_create_spheres' refusals, which
return before a device is touched."""
import ctypes
import struct

import numpy as np
import pytest

import bvh_ref
import rtx
import trace_ref

F32 = np.float32
NODE = -1


def sphere_records(spheres, n):
    """[n, 5] uint32: centre, radius, material — the 20 bytes of an rtx_sphere that carry data."""
    raw = np.ctypeslib.as_array(ctypes.cast(spheres, ctypes.POINTER(ctypes.c_uint32)), shape=(n, 8))
    return raw[:, :5].copy()


def same_but_for_the_sphere_word(got, got_records, want, want_records):
    """Every word equal except a sphere entry's sphere word; through that word both name the same sphere record."""
    assert got.shape == want.shape
    tag = want[:, 7].view(np.int32)
    mask = np.ones(got.shape, bool)
    mask[tag >= 0, 5] = False
    bad = np.nonzero(((got != want) & mask).any(axis=1))[0]
    assert not bad.size, f"{bad.size} entries differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    s = np.nonzero(tag >= 0)[0]
    a, b = got_records[got[s, 5]], want_records[want[s, 5]]
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert not bad.size, f"entry {s[bad[0]]} names {a[bad[0]]} vs {b[bad[0]]}"


@pytest.mark.parametrize("scene", ["random_spheres", "earth_dielectric", "simple_light_demo", "stress_100k"])
def test_reference_equals_host_mirror(built, scene):
    """The host mirror numbers its spheres in walk order, the reference in Add order: the same tree, other labels."""
    host = rtx.HostScene(scene, 1)
    arr, n, draw0, seed = host.world_spheres()
    d = host.desc.contents
    assert n == d.n_spheres
    got = trace_ref.entries_of(bvh_ref.build(arr, n, seed, draw0))
    want = trace_ref.entries_of(host.desc)
    same_but_for_the_sphere_word(got, sphere_records(arr, n), want, sphere_records(d.spheres, n))
    assert sorted(got[got[:, 7].view(np.int32) >= 0, 5].tolist()) == list(range(n))  # every sphere once


def table(spheres):
    arr = (rtx.Sphere * len(spheres))()
    for s, (c, r, m) in zip(arr, spheres):
        s.center[:], s.radius, s.material = list(c), r, m
    return arr


def f(x):  # the bits of a float32
    return struct.unpack("<I", struct.pack("<f", x))[0]


def node(bmin, esc, bmax):
    return [f(v) for v in bmin] + [esc] + [f(v) for v in bmax] + [NODE & 0xFFFFFFFF]


def prim(c, r, index, material):
    return [f(v) for v in c] + [f(r), f(r * r), index, 0, material]


def test_axes_of_the_hand_cases():
    """Words 3.. of host stream 1 of seed 1 under Intn(3) = (word * 3) >> 32: the draws the two trees below use.
    (Philox itself is held to the Random123 vectors in test_ref64.py; this reduction and the stream's counter are
    held to the host mirror by test_reference_equals_host_mirror.)"""
    assert bvh_ref.axes(1, 3, 5) == [1, 1, 0, 2, 0]
    assert bvh_ref.axes(1, 0, 8)[3:] == [1, 1, 0, 2, 0]
    assert bvh_ref.calls(1) == bvh_ref.calls(2) == 1 and bvh_ref.calls(3) == 3 and bvh_ref.calls(5) == 5


def test_two_spheres_by_hand():
    """A list of two is swapped when compare > 0 and kept on a tie.  P (0, 0, 0), Q (0, 3, 0), radius 1.  Seed 1,
    draw0 3 draws y: sign(Q.min.y - P.min.y) = sign(2 - -1) > 0: Q, P.  Draw0 5 draws x: the minima tie: P, Q."""
    P, Q = ((0, 0, 0), 1.0, 4), ((0, 3, 0), 1.0, 5)
    box = node((-1, -1, -1), 3, (1, 4, 1))
    got = trace_ref.entries_of(bvh_ref.build(table([P, Q]), 2, 1, 3))
    assert np.array_equal(got, np.array([box, prim(*Q[:2], 1, 5), prim(*P[:2], 0, 4)], np.uint32))
    got = trace_ref.entries_of(bvh_ref.build(table([P, Q]), 2, 1, 5))
    assert np.array_equal(got, np.array([box, prim(*P[:2], 0, 4), prim(*Q[:2], 1, 5)], np.uint32))


def test_three_spheres_by_hand():
    """Seed 1, draw0 3: the calls draw y (root), y (the list of one: drawn, unused), x (the pair).
      A (1, .5, 0)  r .5    box x: [.5, 1.5]   y: [+0, 1]     (.5 + -.5 = +0)
      B (.5, -0, 2) r 0     box x: [.5, .5]    y: [-0, +0]    (-0 + -0 = -0, -0 + 0 = +0)
      C (1.5, 1, 5) r 1     box x: [.5, 2.5]   y: [+0, 2]
    The three y minima compare equal (diff = +-0): the stable sort keeps A, B, C, split 1 | 2.  The pair draws x, on
    which B and C tie as well: kept, B then C.  Unions take Min(+0, -0) = -0.  A sort that told -0 from +0 would order
    the root's list A, C, B, and the tied pair would stay C, B."""
    A, B, C = ((1, 0.5, 0), 0.5, 7), ((0.5, -0.0, 2), 0.0, 8), ((1.5, 1, 5), 1.0, 9)
    desc = bvh_ref.build(table([A, B, C]), 3, 1, 3)
    want = np.array([
        node((0.5, -0.0, -0.5), 6, (2.5, 2, 6)),    # root
        node((0.5, 0.0, -0.5), 3, (1.5, 1, 0.5)),   # NewBVH([A]): left == right, emitted once
        prim(*A[:2], 0, 7),
        node((0.5, -0.0, 2), 6, (2.5, 2, 6)),       # NewBVH([B, C])
        prim(*B[:2], 1, 8),
        prim(*C[:2], 2, 9),
    ], np.uint32)
    got = trace_ref.entries_of(desc)
    assert np.array_equal(got, want), (got, want)
    nodes = desc.contents.nodes
    assert nodes[1].left == nodes[1].right == rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 0)


def test_five_spheres_by_hand():
    """Seed 1, draw0 3: the calls draw y (root), y (left pair), x (right three), z (its list of one), x (its pair).
    Radius 1 throughout, so min = centre - 1.  Centres in Add order:
      0 (0, 2, 6)   1 (4, 5, 1)   2 (2, 2, 2)   3 (4, 5, 3)   4 (2, 2, 4)
    y minima 1 4 1 4 1: descending and stable 1 3 | 0 2 4.  The pair (1, 3) ties on y: kept.  The three sort by x
    minima -1 1 1: 2 | 4 0; the pair (4, 0) on x: sign(-1 - 1) < 0: kept.  An ascending or an unstable sort moves a
    tie; were the axis drawn after the size switch (the list of one drawing none), the last pair would draw z and be
    swapped (z minima 3, 5)."""
    centres = [(0, 2, 6), (4, 5, 1), (2, 2, 2), (4, 5, 3), (2, 2, 4)]
    desc = bvh_ref.build(table([(c, 1.0, 10 + i) for i, c in enumerate(centres)]), 5, 1, 3)

    def s(i):
        return prim(centres[i], 1.0, i, 10 + i)

    want = np.array([
        node((-1, 1, 0), 10, (5, 6, 7)),
        node((3, 4, 0), 4, (5, 6, 4)), s(1), s(3),
        node((-1, 1, 1), 10, (3, 3, 7)),
        node((1, 1, 1), 7, (3, 3, 3)), s(2),
        node((-1, 1, 3), 10, (3, 3, 7)), s(4), s(0),
    ], np.uint32)
    got = trace_ref.entries_of(desc)
    assert np.array_equal(got, want), (got, want)


def test_min_max_are_gos():
    """math.Min / math.Max: an infinity first, then NaN, then the signed zeros."""
    inf, nan = float("inf"), float("nan")
    sign = lambda v: np.signbit(v)
    assert sign(bvh_ref.go_min(0.0, -0.0)) and sign(bvh_ref.go_min(-0.0, 0.0))
    assert not sign(bvh_ref.go_max(0.0, -0.0)) and not sign(bvh_ref.go_max(-0.0, 0.0))
    assert bvh_ref.go_min(-inf, nan) == -inf and bvh_ref.go_max(nan, inf) == inf
    assert np.isnan(bvh_ref.go_min(inf, nan)) and np.isnan(bvh_ref.go_max(-inf, nan))
    assert bvh_ref.go_min(2.0, -3.0) == -3.0 and bvh_ref.go_max(2.0, -3.0) == 2.0
    with pytest.raises(ValueError):
        bvh_ref.build(table([((float("nan"), 0, 0), 1.0, 0)]), 1, 1, 0)


# ---- rtx_scene_create_spheres' refusals -------------------------------------------------------------------------
def test_create_spheres_refusals(built):
    """Each returns RTX_ERR_INVALID_ARG before a device call (this runs without a GPU) and leaves *out NULL.  The
    count is checked before any sphere is read: 2^25 + 1 with an array of one."""
    L = rtx.load()
    one = table([((0, 0, 0), 1.0, 0)])
    mats = (rtx.Material * 1)()
    texs = (rtx.Texture * 1)()

    def create(spheres, n, out):
        return L.rtx_scene_create_spheres(spheres, n, mats, 1, texs, 1, None, 0, 1, 0, out, None)

    h = ctypes.c_void_p(0xDEAD)
    assert create(one, 1, None) == rtx.RTX_ERR_INVALID_ARG
    assert b"NULL" in L.rtx_last_error()
    for spheres, n, word in ((None, 1, b"NULL"), (one, 0, b"empty World"), (one, (1 << 25) + 1, b"too many spheres")):
        h.value = 0xDEAD
        assert create(spheres, n, ctypes.byref(h)) == rtx.RTX_ERR_INVALID_ARG, word
        assert word in L.rtx_last_error(), L.rtx_last_error()
        if spheres is not None:
            assert not h.value, word
    bad = table([((0, 0, 0), 1.0, 0), ((1, 0, 0), 1.0, 1)])  # material 1 of a table of one
    h.value = 0xDEAD
    assert create(bad, 2, ctypes.byref(h)) == rtx.RTX_ERR_INVALID_ARG
    assert b"sphere 1 material 1 out of range" in L.rtx_last_error()
    assert not h.value
