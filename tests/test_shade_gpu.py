"""Path building blocks on the GPU (rtx_camera_rays*, rtx_shade*).

The contract is the loop include/rtx.h spells out: camera rays, then trace and shade max_depth times, is a render.
wavefront.render is that loop; on every case of tests/ref64_cases.py (caller's tree, every box test) its image equals
the oracle's iterative order bit for bit on every pixel and its segments, hits, rng_draws and texel_fetches are the
oracle's counters.  The other tests take the two kernels apart: partial waves and record order, keys and seed at their
limits against a numpy reading of DESIGN.md §3, the camera rays' order and draws, the zero records, the entry forms,
and that renders are left alone."""
import ctypes
import os

import numpy as np
import pytest

import oracle_binding as ob
import parity
import ref64
import ref64_cases as rc
import rtx
import trace_sets as ts
import wavefront

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 7  # records after the n the call may write: they must keep their poison
WORK = ("segments", "hits", "rng_draws", "texel_fetches")
SEED_LIMIT = 0xFEDCBA9876543210


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


def case(name):
    _, make, seed, window, spp, _ = rc.CASES[rc.NAMES.index(name)]
    desc, cam = make()
    assert cam.samples_per_pixel == spp
    return desc, cam, seed, rtx.Region(*(window or (0, 0, cam.image_width, cam.image_height)), 0, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def loop_equals_oracle(torch, dev, desc, cam, seed, region):
    want, cnt = ob.render(desc, cam, seed, region, ob.ORDER_ITERATIVE)
    ref, _ = ob.render(desc, cam, seed, region, ob.ORDER_REFERENCE)
    for compact in (False, True):
        img, work = wavefront.render(dev, cam, seed, region, compact=compact, counters=True)
        img = img.cpu().numpy()
        assert img.shape == want.shape and img.dtype == F
        bad = np.argwhere((bits(img) != bits(want)).any(axis=2))
        print(f"compact={compact}: {len(bad)} of {want.shape[0] * want.shape[1]} pixels differ; work {work}; "
              f"max |loop - reference order| {np.abs(img - ref).max():.3g}")
        assert len(bad) == 0, (compact, bad[:4], [(img[y, x], want[y, x]) for y, x in bad[:4]])
        assert work == {k: cnt[k] for k in WORK}, (compact, work, cnt)
        assert np.abs(img - ref).max() <= parity.TOL
        plain = wavefront.render(dev, cam, seed, region, compact=compact)  # the timed shade, no stats
        assert np.array_equal(bits(plain.cpu().numpy()), bits(want))


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_loop_is_the_render(torch, name):
    desc, cam, seed, region = case(name)
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        loop_equals_oracle(torch, dev, desc, cam, seed, region)
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["random_spheres_64x36", "random_spheres_24x13x4"])
def test_the_loop_is_the_render_on_the_library_trees(torch, name):
    desc, cam, seed, region = case(name)
    dev = rtx.DeviceScene(desc)
    try:
        loop_equals_oracle(torch, dev, desc, cam, seed, region)
    finally:
        dev.close()


# ---- the two kernels taken apart -----------------------------------------------------------------------
def shade_dev(torch, dev, rays, hits, keys, seed, flags=0, stats=False):
    """rtx_shade_device on torch tensors: the bounce buffer poisoned with 0xFF, PAD records longer than n."""
    n = len(rays)
    d = [to_device(torch, a) for a in (rays, hits, keys)]
    out = torch.full(((n + PAD) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    st = dev.shade_device(seed, *[t.data_ptr() if n else 0 for t in d], n, out.data_ptr(), flags, stream_of(torch), stats)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 64:] == 0xFF).all(), "records past n were written"
    return got[: n * 64].view(rtx.BOUNCE_DTYPE), st


def trace_dev(torch, dev, rays, flags=rtx.RTX_TRACE_UV):
    n = len(rays)
    d_rays = to_device(torch, rays)
    d_hits = torch.zeros((n * 48,), dtype=torch.uint8, device="cuda")
    dev.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags, stream_of(torch))
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(rtx.HIT_DTYPE)


def camera_dev(torch, cam, seed, region, first, count, want_keys=True):
    """rtx_camera_rays_device: (rays, keys or None), PAD poisoned records after each."""
    n = count * rtx.region_rows(region) * region.width
    d_rays = torch.full(((n + PAD) * 32,), 0xFF, dtype=torch.uint8, device="cuda")
    d_keys = torch.full(((n + PAD) * 16,), 0xFF, dtype=torch.uint8, device="cuda")
    rtx.camera_rays_device(cam, seed, region, first, count, d_rays.data_ptr(), d_keys.data_ptr() if want_keys else 0,
                           stream_of(torch))
    torch.cuda.synchronize()
    r, k = d_rays.cpu().numpy(), d_keys.cpu().numpy()
    assert (r[n * 32:] == 0xFF).all() and (k[(n if want_keys else 0) * 16:] == 0xFF).all(), "records past n were written"
    return r[: n * 32].view(rtx.RAY_DTYPE), (k[: n * 16].view(rtx.KEY_DTYPE) if want_keys else None)


_event2 = {}


def event2(torch):
    """random_spheres_64x36 after one bounce: (scene, seed, rays, hits, keys, bounces) of event 2: mixed materials and
    misses in every wave.  Computed once, shared, never modified."""
    if not _event2:
        desc, cam, seed, region = case("random_spheres_64x36")
        dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
        rays, keys = camera_dev(torch, cam, seed, region, 0, 1)
        hits = trace_dev(torch, dev, rays)
        b, _ = shade_dev(torch, dev, rays, hits, keys, seed)
        rays2, keys2 = b["ray"].copy(), keys.copy()
        keys2["event"] += 1
        hits2 = trace_dev(torch, dev, rays2)
        out, _ = shade_dev(torch, dev, rays2, hits2, keys2, seed)
        _event2.update(dev=dev, seed=seed, rays=rays2, hits=hits2, keys=keys2, out=out, desc=desc, first=(rays, hits, keys, b))
    e = _event2
    return e["dev"], e["seed"], e["rays"], e["hits"], e["keys"], e["out"]


def test_event2_mixes_materials_and_misses_within_waves(torch):
    dev, seed, rays, hits, keys, out = event2(torch)
    d = _event2["desc"].contents
    kinds = np.array([d.materials[i].type for i in range(d.n_materials)])
    hit = hits["prim"] != rtx.RTX_HIT_NONE
    kind = np.where(hit, kinds[np.where(hit, hits["material"], 0)], -1)
    mixed = sum(len(set(kind[64 * w: 64 * w + 64])) >= 2 for w in range(len(rays) // 64))
    print(f"{mixed} of {len(rays) // 64} waves hold more than one kind of record (a row of sky holds misses alone)")
    assert mixed > 0
    assert set(kind) >= {-1, rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_METAL, rtx.RTX_MAT_DIELECTRIC}
    assert (keys["event"] == 2).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_partial_waves_and_order(torch, n):
    dev, seed, rays, hits, keys, out = event2(torch)
    r, h, k, want = (np.resize(a, n) for a in (rays, hits, keys, out))
    sums = (n, int((h["prim"] != rtx.RTX_HIT_NONE).sum()), int((want["flags"] & rtx.RTX_BOUNCE_SCATTERED != 0).sum()),
            int(want["rng_draws"].sum(dtype=np.uint64)), 0)
    for flags, stats in ((0, False), (0, True), (rtx.RTX_SHADE_COUNTERS, True), (rtx.RTX_SHADE_COUNTERS, False)):
        got, st = shade_dev(torch, dev, r, h, k, seed, flags, stats)
        assert got.tobytes() == want.tobytes(), (flags, stats)
        if stats:
            counted = (st.n, st.hits, st.scattered, st.rng_draws, st.texel_fetches)
            assert counted == (sums if flags else (n, 0, 0, 0, 0)), (flags, counted, sums)
            assert st.kernel_ms > 0 or n == 0
        else:
            assert st is None
    perm = np.random.default_rng(n).permutation(n)
    got, _ = shade_dev(torch, dev, r[perm], h[perm], k[perm], seed)
    assert got.tobytes() == want[perm].tobytes()


def test_launch_cut(torch):
    """Several launches give the same bytes and the same sums (RTX_SHADE_LAUNCH_RECORDS, RTX_CAMERA_LAUNCH_RAYS)."""
    dev, seed, rays, hits, keys, out = event2(torch)
    desc, cam, cseed, region = case("random_spheres_24x13x4")
    want_r, want_k = camera_dev(torch, cam, cseed, region, 0, 4)
    old = {k: os.environ.get(k) for k in ("RTX_SHADE_LAUNCH_RECORDS", "RTX_CAMERA_LAUNCH_RAYS")}
    try:
        os.environ["RTX_SHADE_LAUNCH_RECORDS"] = "1000"
        os.environ["RTX_CAMERA_LAUNCH_RAYS"] = "700"  # two samples of 24 x 13 per launch
        got, st = shade_dev(torch, dev, rays, hits, keys, seed, rtx.RTX_SHADE_COUNTERS, True)
        assert got.tobytes() == out.tobytes()
        assert (st.n, st.rng_draws) == (len(rays), int(out["rng_draws"].sum()))
        r, k = camera_dev(torch, cam, cseed, region, 0, 4)
        assert r.tobytes() == want_r.tobytes() and k.tobytes() == want_k.tobytes()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_keys_and_seed_at_their_limits(torch):
    """One Lambertian sphere, 256 hits, keys from {0, 1, 2^31, 2^32 - 1}^3, the seed with every byte different:
    ray.dir = normal + s in numpy float32, s the first attempt inside the unit sphere from ref64's Philox, made a
    unit vector as vec3.go:103-107 does."""
    t = rc.Tables()
    t.sphere((0.0, 0.0, 0.0), 1.0, t.material(rtx.RTX_MAT_LAMBERTIAN, t.solid((0.5, 0.625, 0.75))))
    dev = rtx.DeviceScene(t.desc(), reference_bvh=True, every_box=True)
    try:
        rs = np.random.default_rng(34)
        n = 256
        d = ts.unit_dirs(rs, n).astype(F)
        rays = ts.make_rays(F(3) * d, -d, F(0.001), ts.INF)
        hits = trace_dev(torch, dev, rays)
        assert (hits["prim"] == 0).all()
        limits = np.array([0, 1, 1 << 31, (1 << 32) - 1], np.uint32)
        keys = np.zeros(n, rtx.KEY_DTYPE)
        triples = np.array([(a, b, c) for a in limits for b in limits for c in limits], np.uint32)  # all 64, four times
        sel = np.concatenate([rs.permutation(64) for _ in range(4)])
        keys["pixel"], keys["sample"], keys["event"] = triples[sel].T
        keys["draws"] = 0xDEADBEEF  # ignored on input
        got, st = shade_dev(torch, dev, rays, hits, keys, SEED_LIMIT, rtx.RTX_SHADE_COUNTERS, True)

        k0, k1 = SEED_LIMIT & 0xFFFFFFFF, SEED_LIMIT >> 32
        s = np.zeros((n, 3), F)
        attempts = np.zeros(n, np.int64)
        todo = np.ones(n, bool)
        for a in range(64):
            w = ref64.philox4x32_10(keys["pixel"], keys["sample"], keys["event"], np.full(n, a), k0, k1)
            v = np.stack([(x >> np.uint64(8)).astype(F) * F(2.0 ** -23) - F(1) for x in w[:3]], axis=1)
            lsq = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            ok = todo & (lsq < F(1))
            length = np.sqrt(lsq[ok])
            s[ok] = v[ok] * (F(1) / length)[:, None]  # vec3.go:103-107: Scale(1 / Len())
            attempts[todo] += 1
            todo &= ~ok
            if not todo.any():
                break
        assert not todo.any() and attempts.max() > 1
        normal = hits["normal"]
        want = normal + s
        near_zero = (np.abs(want) < F(1e-8)).all(axis=1)
        want[near_zero] = normal[near_zero]
        assert want.dtype == F
        bad = np.nonzero((bits(got["ray"]["dir"]) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, (bad[:4], got["ray"]["dir"][bad[:4]], want[bad[:4]], keys[bad[:4]])
        assert np.array_equal(got["rng_draws"], 3 * attempts)
        assert (got["flags"] == rtx.RTX_BOUNCE_SCATTERED).all() and (got["emitted"] == 0).all()
        assert np.array_equal(bits(got["attenuation"]), bits(np.tile(np.array([0.5, 0.625, 0.75], F), (n, 1))))
        assert np.array_equal(bits(got["ray"]["origin"]), bits(hits["point"]))
        assert (got["ray"]["tmin"] == F(0.001)).all() and (got["ray"]["tmax"] == ts.INF).all()
        assert (st.n, st.hits, st.scattered, st.rng_draws, st.texel_fetches) == (n, n, n, int(3 * attempts.sum()), 0)
    finally:
        dev.close()


def region_row(region, i):
    return int(rtx.load().rtx_region_row(ctypes.byref(region), ctypes.c_uint32(i)))


@pytest.mark.parametrize("scene,width,window", [("random_spheres", 64, (3, 2, 37, 21)), ("cornell_box", 40, (1, 5, 38, 30))])
def test_camera_rays(torch, scene, width, window):
    host = rtx.HostScene(scene, 1)
    cam = host.camera(width=width, spp=5, depth=50)
    assert (cam.defocus_angle > 0) == (scene == "random_spheres")
    seed, W = 11, cam.image_width
    x0, y0, w, h = window
    whole = rtx.Region(x0, y0, w, h, 0, 1)
    P = w * h
    rays, keys = camera_dev(torch, cam, seed, whole, 0, 5)
    assert len(rays) == 5 * P
    assert (rays["tmin"] == F(0.001)).all() and (rays["tmax"] == ts.INF).all()
    ks, ys, xs = np.meshgrid(np.arange(5), np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    assert np.array_equal(keys["pixel"], (ys * W + xs).reshape(-1)) and np.array_equal(keys["sample"], ks.reshape(-1))
    assert (keys["event"] == 1).all() and (keys["draws"] >= 4).all() and (keys["draws"] % 2 == 0).all()
    assert (keys["draws"] > 4).any()  # some disk sample was rejected: the loop runs with and without defocus
    if scene == "cornell_box":
        assert (bits(rays["origin"]) == bits(np.array(list(cam.center), F))).all()
    # the oracle's GetRay draws: a render of the same region without a single segment
    c0 = rtx.Camera.from_buffer_copy(cam)
    c0.max_depth = 0
    _, cnt = ob.render(host.desc, c0, seed, whole, ob.ORDER_ITERATIVE)
    assert cnt["segments"] == 0 and int(keys["draws"].sum()) == cnt["rng_draws"]
    # d_keys = NULL; samples [3, 5) alone; the host entry
    only, none = camera_dev(torch, cam, seed, whole, 0, 5, want_keys=False)
    assert none is None and only.tobytes() == rays.tobytes()
    r2, k2 = camera_dev(torch, cam, seed, whole, 3, 2)
    assert r2.tobytes() == rays[3 * P:].tobytes() and k2.tobytes() == keys[3 * P:].tobytes()
    hr, hk = rtx.camera_rays(cam, seed, whole, 0, 5)
    assert hr.shape == (5, h, w) and hr.tobytes() == rays.tobytes() and hk.tobytes() == keys.tobytes()
    # a shard: the rows rtx_region_row names, of every sample
    shard = rtx.Region(x0, y0, w, h, 1, 3, 4)
    rows = rtx.region_rows(shard)
    assert 0 < rows < h
    pick = [region_row(shard, i) for i in range(rows)]
    sr, sk = camera_dev(torch, cam, seed, shard, 0, 5)
    assert sr.tobytes() == rays.reshape(5, h, w)[:, pick].tobytes()
    assert sk.tobytes() == keys.reshape(5, h, w)[:, pick].tobytes()
    # the last sample word
    top = (1 << 32) - 2
    rt, kt = camera_dev(torch, cam, seed, whole, top, 1)
    assert (kt["sample"] == top).all() and rt.tobytes() != rays[:P].tobytes()


def test_zero_records_and_entry_forms(torch):
    dev, seed, rays, hits, keys, out = event2(torch)
    zero = np.zeros(len(rays), rtx.BOUNCE_DTYPE)
    # misses: rays that leave the scene
    away = ts.make_rays(np.tile([0, 5000, 0], (len(rays), 1)), np.tile([0, 1, 0], (len(rays), 1)), F(0.001), ts.INF)
    miss = trace_dev(torch, dev, away)
    assert (miss["prim"] == rtx.RTX_HIT_NONE).all()
    got, st = shade_dev(torch, dev, away, miss, keys, seed, rtx.RTX_SHADE_COUNTERS, True)
    assert got.tobytes() == zero.tobytes() and (st.hits, st.scattered, st.rng_draws) == (0, 0, 0)
    # ended paths: the all-zero bounce ray is a miss, and shades to an all-zero bounce again
    ended = ~(out["flags"] & rtx.RTX_BOUNCE_SCATTERED).astype(bool)
    assert ended.any() and out["ray"][ended].tobytes() == zero["ray"][ended].tobytes()
    again = trace_dev(torch, dev, out["ray"])
    assert (again["prim"][ended] == rtx.RTX_HIT_NONE).all()
    nxt = keys.copy()
    nxt["event"] += 1
    got, _ = shade_dev(torch, dev, out["ray"], again, nxt, seed)
    assert got[ended].tobytes() == zero[ended].tobytes()
    # a material index outside the table is no hit
    wild = hits.copy()
    wild["material"] = 0x7FFFFFFF
    got, _ = shade_dev(torch, dev, rays, wild, keys, seed)
    assert got.tobytes() == zero.tobytes()
    # the host entry equals the device entry, with stats and without, in any shape
    host, st = dev.shade(rays, hits, keys, seed, stats=True, flags=rtx.RTX_SHADE_COUNTERS)
    assert host.dtype == rtx.BOUNCE_DTYPE and host.shape == rays.shape and host.tobytes() == out.tobytes()
    assert st.n == len(rays) and st.rng_draws == int(out["rng_draws"].sum()) and st.kernel_ms > 0
    assert dev.shade(rays.reshape(-1, 64), hits.reshape(-1, 64), keys.reshape(-1, 64), seed).tobytes() == out.tobytes()
    assert dev.shade(rays[:0], hits[:0], keys[:0], seed).shape == (0,)


def test_wrong_device_and_flags(torch):
    dev, seed, rays, hits, keys, out = event2(torch)
    with pytest.raises(rtx.RtxError) as e:
        dev.shade(rays, hits, keys, seed, flags=2)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG
    with pytest.raises(rtx.RtxError) as e:
        shade_dev(torch, dev, rays, hits, keys, seed, flags=1 << 8)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG
    if torch.cuda.device_count() > 1:  # a device without a copy of the scene
        torch.cuda.set_device(1)
        try:
            with pytest.raises(rtx.RtxError) as e:
                dev.shade(rays, hits, keys, seed)
            assert e.value.code == rtx.RTX_ERR_INVALID_ARG
        finally:
            torch.cuda.set_device(0)


def test_renders_are_left_alone(torch):
    """A render's image and RTX_FLAG_COUNTERS stats before and after a counting shade and a camera-ray call are equal,
    and the sample scratch is not touched."""
    _, seed, rays, hits, keys, out = event2(torch)
    host = rtx.HostScene("random_spheres", seed=1)
    cam = host.camera(width=48, spp=8, depth=50)
    other = host.camera(width=64, spp=1, depth=50)
    dev = rtx.DeviceScene(host.desc)
    work = [n for n, _ in rtx.Stats._fields_ if n not in ("kernel_ms", "gather_ms", "trav_cycles", "shade_cycles",
                                                          "shade_split_cycles")]
    try:
        img0, st0 = dev.render_host(cam, 7, counters=True)
        scratch = rtx.device_scratch_bytes(0)
        assert scratch > 0
        got, st = shade_dev(torch, dev, rays, hits, keys, seed, rtx.RTX_SHADE_COUNTERS, True)
        assert got.tobytes() == out.tobytes() and st.hits > 0  # (the same materials: the same scene)
        camera_dev(torch, other, seed, rtx.Region(0, 0, other.image_width, other.image_height, 0, 1), 0, 1)
        assert rtx.device_scratch_bytes(0) == scratch
        img1, st1 = dev.render_host(cam, 7, counters=True)
        assert np.array_equal(bits(img0), bits(img1))
        assert {k: getattr(st0, k) for k in work} == {k: getattr(st1, k) for k in work}
        rtx.release_device_memory(0)  # releasing the device's scratch does not disturb a shade
        again, _ = shade_dev(torch, dev, rays, hits, keys, seed)
        assert again.tobytes() == out.tobytes() and rtx.device_scratch_bytes(0) == 0
    finally:
        dev.close()
    rtx.device_check(0)


def test_zz_device_check_and_close(torch):
    """Last in the module: every call above left the device's sticky error word clean; free the module's scene."""
    rtx.device_check(0)
    if _event2:
        _event2.pop("dev").close()
        _event2.clear()
