"""Ray queries on the GPU (rtx_trace_device / rtx_trace) against tests/trace_ref.py on the ray sets of
tests/trace_sets.py.

Caller's tree (RTX_SCENE_REFERENCE_BVH | RTX_SCENE_EVERY_BOX: the trace walks exactly the exported entries): every
field of every hit of every set is bit-equal to trace_ref.walk in float32 — no ray left out — and the counting
instantiation's node_visits / prim_tests / hits are its sums.  Default scenes (the library's own trees where the scene
qualifies): bit-equal to trace_ref.scan in float32 on the kept rays, whichever octant is hinted."""
import ctypes
import os

import numpy as np
import pytest

import oracle_binding as ob
import rtx
import trace_ref
import trace_sets as ts

pytestmark = pytest.mark.gpu

ANY, UV, COUNT = rtx.RTX_TRACE_ANY, rtx.RTX_TRACE_UV, rtx.RTX_TRACE_COUNTERS
PAD = 7  # records after the n the call may write: they must keep their poison


@pytest.fixture(scope="module")
def torch(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


_scenes = {}


def device_scene(name: str, reference: bool) -> rtx.DeviceScene:
    """One device scene per (scene, tree) for the module: the caller's tree with every box test, or the default."""
    key = (name, reference)
    if key not in _scenes:
        _scenes[key] = rtx.DeviceScene(ts.scene(name).desc, reference_bvh=reference, every_box=reference)
    return _scenes[key]


def trace(torch, dev, rays, flags=0, stats=False):
    """rtx_trace_device on torch tensors: the hit buffer poisoned with 0xFF, PAD records longer than n."""
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.full(((n + PAD) * 48,), 0xFF, dtype=torch.uint8, device="cuda")
    st = dev.trace_device(d_rays.data_ptr() if n else 0, n, d_hits.data_ptr(), flags,
                          torch.cuda.current_stream().cuda_stream, stats)
    torch.cuda.synchronize()
    out = d_hits.cpu().numpy()
    assert (out[n * 48:] == 0xFF).all(), "records past n were written"
    return out[: n * 48].view(rtx.HIT_DTYPE), st


def differing(a, b, mask=None):
    """Indices of the records that differ in any byte."""
    bad = (a.view(np.uint8).reshape(-1, 48) != b.view(np.uint8).reshape(-1, 48)).any(axis=1)
    return np.nonzero(bad if mask is None else bad & mask)[0]


@pytest.mark.parametrize("name", ts.SETS)
def test_callers_tree_is_the_reference_walk(torch, name):
    s = ts.ray_set(name)
    dev = device_scene(ts.SCENE_OF[name], True)
    assert dev.export() == s.scene.entries.tobytes()  # the trace walks what trace_ref walks
    w = s.walk32
    for flags in (UV, 0):
        want = w.records(uv=bool(flags & UV))
        got, st = trace(torch, dev, s.rays, flags, stats=True)  # timed
        bad = differing(got, want)
        assert bad.size == 0, (flags, bad[:8], got[bad[:3]], want[bad[:3]])
        assert (st.rays, st.walk_layout) == (len(s.rays), rtx.RTX_LAYOUT_REFERENCE)
        assert st.scene_placement == (rtx.RTX_SCENE_IN_HBM if name == "big" else rtx.RTX_SCENE_IN_LDS)
        assert (st.hits, st.node_visits, st.prim_tests) == (0, 0, 0)  # the timed kernel counts nothing
        got, st = trace(torch, dev, s.rays, flags | COUNT, stats=True)  # counting
        assert differing(got, want).size == 0
        assert (st.hits, st.node_visits, st.prim_tests) == (int(w.mask.sum()), int(w.node_visits.sum()), int(w.prim_tests.sum()))
    if name != "edges":
        assert (want["u"] == 0).all() and (want["v"] == 0).all() and (w.u[w.mask] != 0).any()


@pytest.mark.parametrize("name", ts.SETS)
def test_default_scene_equals_scan_on_kept_rays(torch, name):
    s = ts.ray_set(name)
    dev = device_scene(ts.SCENE_OF[name], False)
    want = s.scan32.records(uv=True)
    first = None
    for octant in (0, 5, 7):
        got, st = trace(torch, dev, s.rays, UV | rtx.RTX_TRACE_OCTANT(octant), stats=True)
        bad = differing(got, want, s.kept)
        assert bad.size == 0, (octant, bad[:8], got[bad[:3]], want[bad[:3]])
        assert st.walk_layout in (octant, rtx.RTX_LAYOUT_REFERENCE)
        if first is None:
            first = got
        assert differing(got, first).size == 0, octant  # every hint: the same hits, left-out rays included
    if name in ("primary", "incoherent"):
        assert st.walk_layout == 7  # randSpheres walks the library's own tree
    if name == "edges":  # the coincident pair by name: sphere 0, first in the reference walk, whatever tree is walked
        assert (first["prim"][:3] == 0).all() and (first["material"][:3] == 0).all()
        assert s.scan32.tie[:3].all() and not s.kept[:3].any()
        n = len(s.rays)
        assert (first["prim"][n - 3:] == 0).all()


@pytest.mark.parametrize("reference", [True, False])
@pytest.mark.parametrize("name", ts.SETS)
def test_any_hit_mask_is_the_closest_hit_mask(torch, name, reference):
    s = ts.ray_set(name)
    dev = device_scene(ts.SCENE_OF[name], reference)
    closest, _ = trace(torch, dev, s.rays)
    anyhit, st = trace(torch, dev, s.rays, ANY | COUNT, stats=True)
    assert np.array_equal(anyhit["prim"] != rtx.RTX_HIT_NONE, closest["prim"] != rtx.RTX_HIT_NONE)
    assert st.hits == int((closest["prim"] != rtx.RTX_HIT_NONE).sum())
    if reference:  # the any-hit walk of the caller's tree is the reference's, stopped at the first accepted primitive
        a = trace_ref.walk(s.scene.ref, s.rays, np.float32, uv=False, any_hit=True)
        assert differing(anyhit, a.records(uv=False)).size == 0
        assert (st.node_visits, st.prim_tests) == (int(a.node_visits.sum()), int(a.prim_tests.sum()))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_batch_sizes(torch, n):
    s = ts.ray_set("incoherent")
    dev = device_scene("random_spheres", True)
    rays = np.resize(s.rays, n)
    want = np.resize(s.walk32.records(uv=False), n)
    got, st = trace(torch, dev, rays, COUNT, stats=True)
    assert differing(got, want).size == 0
    assert st.rays == n and st.hits == int((want["prim"] != rtx.RTX_HIT_NONE).sum())
    got, st = trace(torch, dev, rays)  # enqueued without stats
    assert st is None and differing(got, want).size == 0


@pytest.fixture
def knobs():
    """Set the library's per-call knobs for one test (read from the environment by every trace)."""
    names = ("RTX_TRACE_REFILL", "RTX_TRACE_RANGE", "RTX_TRACE_LAUNCH_RAYS", "RTX_TRACE_PRIM_BATCH")
    old = {k: os.environ.get(k) for k in names}

    def set_(**kw):
        for k in names:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in kw.items()})

    yield set_
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def test_refill_and_launch_cut(torch, knobs):
    """One ray in 64 walks the scene, the rest miss the root box: parked lanes take the next rays of the wave's range
    while the long walks go on (the refill), at every threshold and range; several launches give the same bytes."""
    s = ts.ray_set("primary")
    dev = device_scene("random_spheres", True)
    n = 4097
    rays = ts.make_rays(np.tile([0, 5000, 0], (n, 1)), np.tile([0, 1, 0], (n, 1)), np.float32(0.001), ts.INF)
    long_ = np.arange(0, n, 64)
    walkers = np.nonzero(s.walk32.node_visits > 8)[0]  # (the sky's rays miss the root box themselves)
    rays[long_] = s.rays[walkers[np.linspace(0, len(walkers) - 1, len(long_)).astype(int)]]
    ref = trace_ref.walk(s.scene.ref, rays, np.float32)
    want = ref.records(uv=True)
    assert (ref.node_visits[np.setdiff1d(np.arange(n), long_)] == 1).all() and ref.node_visits[long_].min() > 8
    for kw in ({}, {"RTX_TRACE_REFILL": 64}, {"RTX_TRACE_REFILL": 32}, {"RTX_TRACE_REFILL": 1},
               {"RTX_TRACE_REFILL": 48, "RTX_TRACE_RANGE": 64}, {"RTX_TRACE_REFILL": 16, "RTX_TRACE_RANGE": 4096},
               {"RTX_TRACE_LAUNCH_RAYS": 1024}, {"RTX_TRACE_PRIM_BATCH": 1}, {"RTX_TRACE_PRIM_BATCH": 65}):
        knobs(**kw)
        got, st = trace(torch, dev, rays, UV | COUNT, stats=True)
        bad = differing(got, want)
        assert bad.size == 0, (kw, bad[:8])
        assert (st.hits, st.node_visits, st.prim_tests) == (int(ref.mask.sum()), int(ref.node_visits.sum()),
                                                           int(ref.prim_tests.sum())), kw
        got, _ = trace(torch, dev, rays, UV)
        assert differing(got, want).size == 0, kw


def test_host_entry_equals_device_entry(torch):
    for name, reference in (("secondary", False), ("cornell", True), ("big", False)):
        s = ts.ray_set(name)
        dev = device_scene(ts.SCENE_OF[name], reference)
        got, _ = trace(torch, dev, s.rays, UV)
        host, st = dev.trace(s.rays, UV | COUNT, stats=True)
        assert host.dtype == rtx.HIT_DTYPE and host.shape == s.rays.shape
        assert host.tobytes() == got.tobytes()
        assert st.rays == len(s.rays) and st.hits == int((got["prim"] != rtx.RTX_HIT_NONE).sum()) and st.kernel_ms > 0
        assert dev.trace(s.rays.reshape(-1, 64), UV).tobytes() == got.tobytes()
    assert dev.trace(s.rays[:0]).shape == (0,)


def test_wrong_device_and_flags(torch):
    dev = device_scene("edges", True)
    rays = ts.ray_set("edges").rays
    with pytest.raises(rtx.RtxError) as e:
        dev.trace(rays, 1 << 12)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG
    if torch.cuda.device_count() > 1:  # a device without a copy of the scene
        torch.cuda.set_device(1)
        try:
            with pytest.raises(rtx.RtxError) as e:
                dev.trace(rays)
            assert e.value.code == rtx.RTX_ERR_INVALID_ARG
        finally:
            torch.cuda.set_device(0)


def test_a_trace_leaves_renders_alone(torch):
    """A render's image and RTX_FLAG_COUNTERS stats before and after a counting trace are equal (the trace plans and
    replaces no layout a render uses, and counts in memory of its own); the sample scratch is not touched."""
    host = rtx.HostScene("random_spheres", seed=1)
    cam = host.camera(width=48, spp=8, depth=50)
    dev = rtx.DeviceScene(host.desc)
    s = ts.ray_set("incoherent")
    work = [n for n, _ in rtx.Stats._fields_ if n not in ("kernel_ms", "gather_ms", "trav_cycles", "shade_cycles",
                                                          "shade_split_cycles")]
    try:
        # a trace BEFORE the scene's first render: that render must still plan its own (collapsed) walk
        first, _ = trace(torch, dev, s.rays, UV | COUNT | rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)), stats=True)
        img0, st0 = dev.render_host(cam, 7, counters=True)
        scratch = rtx.device_scratch_bytes(0)
        assert scratch > 0
        got, st = trace(torch, dev, s.rays, UV | COUNT | rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)), stats=True)
        assert rtx.device_scratch_bytes(0) == scratch
        assert differing(got, first).size == 0 and st.node_visits > 0
        img1, st1 = dev.render_host(cam, 7, counters=True)
        assert np.array_equal(img0, img1)
        assert {k: getattr(st0, k) for k in work} == {k: getattr(st1, k) for k in work}
        # the same scene without any trace: the same walk, box test for box test
        fresh = rtx.DeviceScene(host.desc)
        try:
            img2, st2 = fresh.render_host(cam, 7, counters=True)
        finally:
            fresh.close()
        assert np.array_equal(img0, img2)
        assert {k: getattr(st0, k) for k in work} == {k: getattr(st2, k) for k in work}
        # releasing the device's scratch does not disturb a trace
        rtx.release_device_memory(0)
        assert rtx.device_scratch_bytes(0) == 0
        again, _ = trace(torch, dev, s.rays, UV | rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)))
        assert differing(again, first).size == 0 and rtx.device_scratch_bytes(0) == 0
    finally:
        dev.close()
    assert rtx.load().rtx_device_check(0) == rtx.RTX_OK


def test_auto_focus(torch):
    """The feature used as intended: focus_dist from what the centre pixel sees.  t * |dir| of the centre-pixel ray of
    rand_spheres_camera lies within float32 rounding of the distance trace_ref.scan gives in float64: the bound is the
    reference's own float32 error on this ray (four times it, at least four float32 ulps of the distance)."""
    cam = ob.rand_spheres_camera(400, 1, 1)
    p00, du, dv, cen = (np.array(list(v), np.float32) for v in (cam.pixel00, cam.pixel_du, cam.pixel_dv, cam.center))
    d = (p00 + du * np.float32(cam.image_width // 2)) + dv * np.float32(cam.image_height // 2) - cen
    ray = ts.make_rays(cen, d, np.float32(0.001), ts.INF)
    sc = ts.scene("random_spheres")
    h64, h32 = trace_ref.scan(sc.ref, ray, np.float64), trace_ref.scan(sc.ref, ray, np.float32)
    assert h64.mask[0] and not h64.tie[0] and h32.prim[0] == h64.prim[0]
    length = float(np.linalg.norm(d.astype(np.float64)))
    want = float(h64.t[0]) * length
    tol = max(4 * abs(float(h32.t[0]) * length - want), 4 * float(np.spacing(np.float32(want))))
    got = device_scene("random_spheres", False).trace(ray)
    focus = float(got["t"][0]) * length
    print(f"auto-focus: {focus!r} (float64 reference {want!r}, tolerance {tol:.3g}), sphere {got['prim'][0]}")
    assert got["prim"][0] == h64.prim[0]
    assert abs(focus - want) <= tol
    assert 9.0 < focus < 14.0  # main.go focuses at 10; the centre pixel sees the spheres around the origin


def test_zz_device_check_and_close(torch):
    """Last in the module: every trace above left the device's sticky error word clean; free the module's scenes."""
    assert rtx.load().rtx_device_check(0) == rtx.RTX_OK
    for dev in _scenes.values():
        dev.close()
    _scenes.clear()
