"""Ray queries on the CPU (include/rtx.h, "ray queries"): the structs, the argument checks that need no device, and
the numpy reference (trace_ref.py) pinned against itself on the ray sets of trace_sets.py."""
import ctypes

import numpy as np
import pytest

import rtx
import trace_ref
import trace_sets as ts

LEFT_OUT_CAP = 0.01  # the cap tests/ref64 gives a probe; every set but `edges` must stay under half of it


def test_struct_sizes_match_the_dtypes(built):
    assert ctypes.sizeof(rtx.TraceRay) == rtx.RAY_DTYPE.itemsize == 32
    assert ctypes.sizeof(rtx.TraceHit) == rtx.HIT_DTYPE.itemsize == 48
    assert ctypes.sizeof(rtx.TraceStats) == 7 * 8
    for struct, dtype in ((rtx.TraceRay, rtx.RAY_DTYPE), (rtx.TraceHit, rtx.HIT_DTYPE)):
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
            assert getattr(struct, name).size == dtype.fields[name][0].itemsize, name
    assert rtx.RTX_TRACE_OCTANT(5) == 5 << 8 and rtx.RTX_TRACE_OCTANT(9) == 1 << 8


def test_trace_argument_validation(built):
    L = rtx.load()
    E = rtx.RTX_ERR_INVALID_ARG
    scene = ctypes.create_string_buffer(4096)  # stands for a scene: these checks fail before it is looked at
    s = ctypes.cast(scene, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(4096)
    base = ctypes.addressof(buf)
    al = base + (-base) % 16  # a 16-B aligned address inside buf
    st = rtx.TraceStats()
    for call in (lambda *a: L.rtx_trace_device(*a[:5], None, a[5]), L.rtx_trace):
        assert call(None, al, 4, al + 1024, 0, None) == E
        assert b"scene" in L.rtx_last_error()
        assert call(None, al, 0, al + 1024, 0, None) == E  # a NULL scene even for no rays
        assert call(s, None, 4, al + 1024, 0, None) == E
        assert call(s, al, 4, None, 0, ctypes.byref(st)) == E
        assert call(s, al + 4, 4, al + 1024, 0, None) == E  # numpy's natural alignment of the structs is 4 B
        assert b"16" in L.rtx_last_error()
        assert call(s, al, 4, al + 1024 + 8, 0, None) == E
        assert call(s, al, 4, al + 1024, 8, None) == E  # an unknown flag bit
        assert call(s, al, 4, al + 1024, 1 << 11, None) == E
        assert b"flags" in L.rtx_last_error()
        # n == 0: RTX_OK, nothing launched, no pointer looked at; stats zeroed
        st.rays = 99
        assert call(s, None, 0, None, rtx.RTX_TRACE_ANY | rtx.RTX_TRACE_UV | rtx.RTX_TRACE_COUNTERS | rtx.RTX_TRACE_OCTANT(7),
                    ctypes.byref(st)) == rtx.RTX_OK
        assert st.rays == 0


@pytest.mark.parametrize("name", [n for n in ts.SETS if n != "edges"])
def test_sets_leave_out_at_most_half_the_cap(built, name):
    s = ts.ray_set(name)
    assert len(s.rays) == ts.SIZES[name]
    left = float((~s.kept).mean())
    print(f"{name}: {(~s.kept).sum()} of {len(s.rays)} rays left out, {int((s.scan32.tie | s.scan64.tie).sum())} of them "
          f"ties; {int(s.scan32.mask.sum())} hits")
    assert left <= LEFT_OUT_CAP / 2, left
    assert 0.1 < s.scan32.mask.mean() < 0.95  # neither trivial: the set hits and misses


@pytest.mark.parametrize("name", ts.SETS)
def test_walk_equals_scan(built, name):
    """The reference pinned against itself: its walk over the caller's tree returns scan's records, bit for bit,
    on every kept ray, and on ALL of `edges` (whose ties the walk resolves as scan does: the first met wins)."""
    s = ts.ray_set(name)
    k = np.ones(len(s.rays), bool) if name == "edges" else s.kept
    w, sc = s.walk32.records(), s.scan32.records()
    bad = np.nonzero(k & (w.view(np.uint8).reshape(-1, 48) != sc.view(np.uint8).reshape(-1, 48)).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], w[bad[:3]], sc[bad[:3]])
    # the any-hit walk accepts a primitive for exactly the rays the closest-hit walk does
    a = trace_ref.walk(s.scene.ref, s.rays, np.float32, uv=False, any_hit=True)
    assert np.array_equal(a.mask, s.walk32.mask)
    assert (a.prim_tests <= s.walk32.prim_tests).all()


def test_edges_cases(built):
    """What `edges` is there for, by name (trace_sets.edge_rays)."""
    s = ts.ray_set("edges")
    h, r = s.walk32, s.rays
    assert len(s.scene.entries) == 9 and list(s.scene.ref.sphere[s.scene.ref.prims]) == [0, 1, 2, 3, 4]
    # the coincident pair: sphere 0, first in the reference walk, wins the exact tie (and it is reported)
    assert (h.prim[:3] == 0).all() and (h.material[:3] == 0).all() and s.scan32.tie[:3].all()
    assert h.t[0] == np.float32(4.0) and h.front[0] == 1
    # outside the pair's slab (y = 1.5): on to sphere 2.  Exactly on a box plane (rays 5-7) the rays are tangent:
    # whatever they return, the walk returns scan's (test_walk_equals_scan)
    assert h.prim[3] == 2
    # a zero direction, NaN or infinite components: legal, and a miss here
    assert (h.prim[8:16] == rtx.RTX_HIT_NONE).all() and np.isinf(h.t[8:16]).all()
    # tmin == tmax, tmin > tmax: misses; tmin past the first root: the far side, from inside (back face)
    assert h.prim[16] == h.prim[17] == rtx.RTX_HIT_NONE
    assert h.prim[18] == 0 and h.t[18] == np.float32(6.0) and h.front[18] == 0
    # tmin = -1 from (5, 0, 0), on sphere 3's surface: its root -1 is not inside (-1, inf), its root 0 is, and is
    # closer than sphere 2's 1
    assert h.prim[19] == 3 and h.t[19] == 0 and h.front[19] == 0
    assert h.prim[20] == h.prim[21] == rtx.RTX_HIT_NONE  # a NaN bound
    assert h.prim[22] == 0 and h.prim[23] == 0
    # origins inside spheres: back faces
    assert h.prim[24] == 0 and h.front[24] == 0
    assert h.prim[25] == 3 and h.prim[26] == 3 and h.front[26] == 0
    # tmax exactly a root: that sphere (and its coincident twin) is no hit; one float32 further it is
    n = len(r)
    assert (h.prim[n - 6: n - 3] != 0).all() and (h.prim[n - 3:] == 0).all()
    assert np.array_equal(h.t[n - 3:], r["tmax"][n - 6: n - 3])


def test_entries_of_is_the_reference_walk_order(built):
    """entries_of restates rtx_scene_export's format (test_trace_gpu.py compares the bytes on the GPU): pre-order,
    every node's escape past its subtree, Cornell's nested Worlds in line."""
    for name in ("random_spheres", "cornell_box", "lists", "edges"):
        sc = ts.scene(name).ref
        n = len(sc.entries)
        assert n > 0
        for i in np.nonzero(sc.is_node)[0]:
            assert i + 1 < sc.escape[i] <= n
        assert sc.is_node.sum() + sc.is_sphere.sum() + sc.is_quad.sum() == n
    assert ts.scene("lists").ref.is_node.sum() == 0 and ts.scene("cornell_box").ref.is_quad.sum() == 18
    assert len(ts.scene("big").entries) * 16 > 32768  # past the LDS copy's 'a' halves: the HBM path
