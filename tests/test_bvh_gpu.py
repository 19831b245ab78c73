"""GPU BVH build: rtx_scene_create_spheres builds NewBVHFromWorld (bvh.go:138-185) on the device.

Its threaded entries are held, byte for byte and sphere word included, to tests/bvh_ref.py, the independent reading of
NewBVH: on lists of every size at which the build takes another path (1, 2, the 256-thread launch boundary, block
counts that are powers of two, hipCUB's multi-block sort), with distinct minima, with many exact ties (where only the
stability of the sort decides) and with every sphere identical; on float edges (signed zeros, radii <= 0, subnormals,
differences that overflow, infinities); and on the axis stream's edges (a block index that carries past 32 bits, seeds
with high bits set).  The inputs are generated here from seeded numpy Generators.  NaN inputs are out of contract (the
comparator is no order there, and the reference refuses them): none is generated.

The ray queries, the emitter table, the light-sample block and the renders are then run on a GPU-built scene whose Add
order differs from every walk order: `prim` must name the CALLER's sphere.  The main.go scenes are also compared with
the host mirror's build, which numbers its spheres in walk order: the same tree, other labels."""
import ctypes
import functools

import numpy as np
import pytest

import bvh_ref
import direct_ref
import direct_scenes as ds
import oracle_binding as ob
import rtx
import trace_ref
import wavefront

F32 = np.float32
SEEDS = (1, 0xFFFFFFFF00000001, 2 ** 64 - 1)
DRAWS = (0, 3, 2 ** 34 - 2)  # the last: words 2^34 - 2, 2^34 - 1 are block 2^32 - 1, the next block carries
SIZES = list(range(1, 10)) + [31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4097]
PATTERNS = ("distinct", "quantised", "identical")


def test_world_spheres_export(built):
    host = rtx.HostScene("random_spheres", 1)
    arr, n, draw0, seed = host.world_spheres()
    d = host.desc.contents
    assert n == d.n_spheres and seed == 1
    assert draw0 > 0  # the scene generation drew from the global stream before NewBVH
    assert all(arr[i].material < d.n_materials for i in range(n))
    with pytest.raises(rtx.RtxError):
        rtx.HostScene("cornell_box", 1).world_spheres()  # quads: not a World of spheres


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


# ---- inputs and the two builds ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """Material and texture tables for the generated worlds: 0 Lambertian (solid), 1 Lambertian (checkered), 2 Metal,
    3 Dielectric, 4 and 5 DiffuseLight."""
    texs = [ds.solid(0.6, 0.5, 0.4), ds.checker(0.8, (0.8, 0.8, 0.7), (0.2, 0.3, 0.4)), ds.solid(4, 5, 6), ds.solid(7, 3, 2)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LAMB, 1), ds.material(ds.METAL, albedo=(0.8, 0.7, 0.9), fuzz=0.05),
            ds.material(rtx.RTX_MAT_DIELECTRIC, ior=1.5), ds.material(ds.LIGHT, 2), ds.material(ds.LIGHT, 3)]
    return ds.world([], [], mats, texs)


N_MATERIALS = 6


def sphere_table(center, radius, material):
    n = len(radius)
    arr = (rtx.Sphere * n)()
    raw = np.ctypeslib.as_array(ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint32)), shape=(n, 8))
    raw[:, 0:3].view(F32)[...] = np.asarray(center, F32).reshape(n, 3)
    raw[:, 3].view(F32)[...] = np.asarray(radius, F32)
    raw[:, 4] = np.asarray(material, np.uint32)
    return arr


def world_of(pattern: str, n: int, seed: int):
    """distinct: centres on a permuted grid of step 1/8 per axis, radii of 1, 3 or 5 sixty-fourths: no two box minima
    are equal on any axis.  quantised: 4 values per axis, one radius: 64 places, so ties on every axis from 5 spheres
    on and exact duplicates (with other materials) beyond 64.  identical: one sphere, n times."""
    rng = np.random.default_rng(seed)
    material = rng.integers(0, N_MATERIALS, n)
    if pattern == "distinct":
        center = np.stack([rng.permutation(n) - n // 2 for _ in range(3)], axis=1).astype(F32) * F32(0.125)
        radius = (F32(1) + F32(2) * rng.integers(0, 3, n).astype(F32)) * F32(1 / 64)
        bmin = center - radius[:, None]
        assert all(len(np.unique(bmin[:, a])) == n for a in range(3))
    elif pattern == "quantised":
        center = np.array([-4.5, -1.5, 1.5, 4.5], F32)[rng.integers(0, 4, (n, 3))]
        radius = np.full(n, 0.75, F32)
    else:
        center = np.tile(np.array([1.5, -2.25, 0.5], F32), (n, 1))
        radius = np.full(n, 0.75, F32)
        material[:] = 2
    return sphere_table(center, radius, material)


def reference(arr, n, seed, draw0):
    """(description, entries) of the independent build."""
    desc = bvh_ref.build(arr, n, seed, draw0, tables=tables())
    return desc, trace_ref.entries_of(desc)


def gpu_scene(arr, n, seed, draw0) -> rtx.DeviceScene:
    """rtx_scene_create_spheres over the caller's table (RTX_BVH is read here)."""
    t = tables().contents
    h, ms = ctypes.c_void_p(), ctypes.c_double()
    rtx.check(rtx.load().rtx_scene_create_spheres(arr, n, t.materials, t.n_materials, t.textures, t.n_textures, t.texels,
                                                  t.n_texels, seed, draw0, ctypes.byref(h), ctypes.byref(ms)),
              "rtx_scene_create_spheres")
    dev = rtx.DeviceScene(handle=h)
    dev.build_ms = ms.value
    return dev


def same_entries(got: bytes, want: np.ndarray, what: str):
    want = np.ascontiguousarray(want, np.uint32).reshape(-1, 8)
    assert len(got) == want.nbytes, f"{what}: {len(got) // 32} entries, not {len(want)}"
    if got != want.tobytes():
        g = np.frombuffer(got, np.uint32).reshape(-1, 8)
        bad = np.nonzero((g != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} entries differ, first {bad[0]}: got {g[bad[0]].tolist()} "
                             f"want {want[bad[0]].tolist()}; differing words {sorted(set(np.nonzero(g != want)[1].tolist()))}")


def check_build(monkeypatch, arr, n, seed, draw0):
    """RTX_BVH=reference: the export is the reference's entries.  Default tree: it is the export of the scene
    rtx_scene_create makes from the reference's description (and so the same bytes again)."""
    desc, want = reference(arr, n, seed, draw0)
    monkeypatch.setenv("RTX_BVH", "reference")
    dev = gpu_scene(arr, n, seed, draw0)
    try:
        same_entries(dev.export(), want, f"n {n}, RTX_BVH=reference")
    finally:
        dev.close()
    monkeypatch.delenv("RTX_BVH")
    dev, made = gpu_scene(arr, n, seed, draw0), rtx.DeviceScene(desc)
    try:
        same_entries(dev.export(), np.frombuffer(made.export(), np.uint32), f"n {n}, default tree")
        same_entries(made.export(), want, f"n {n}, rtx_scene_create")
    finally:
        dev.close()
        made.close()
    return want


# ---- the main.go scenes against the host mirror -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", ["reference", "default"])
@pytest.mark.parametrize("scene", ["random_spheres", "earth_dielectric", "simple_light_demo", "stress_100k"])
def test_gpu_build_equals_host_build(torch_cuda, built, monkeypatch, scene, bvh):
    """The GPU build against rtx_scene_create of the host mirror's tree.  The mirror's sphere table is in walk order,
    the caller's in Add order, so a sphere entry's sphere word differs; every other word is equal, and through the
    sphere word both entries name the same sphere record.  (Byte for byte, sphere word included: the tests below,
    against bvh_ref.)  RTX_BVH=reference: the reference's own layout from both builds; default: the walk's tree
    (rtx_topology.h) over them, the same again."""
    if bvh == "reference":
        monkeypatch.setenv("RTX_BVH", "reference")
    host = rtx.HostScene(scene, 1)
    arr, n, _, _ = host.world_spheres()
    ref = rtx.DeviceScene(host.desc)
    gpu = rtx.DeviceScene.from_spheres(host)
    a = np.frombuffer(ref.export(), np.uint32).reshape(-1, 8)
    b = np.frombuffer(gpu.export(), np.uint32).reshape(-1, 8)
    assert a.shape == b.shape
    sphere = a[:, 7].view(np.int32) >= 0
    mask = np.ones(a.shape, bool)
    mask[sphere, 5] = False
    bad = np.nonzero(((a != b) & mask).any(axis=1))[0]
    assert not bad.size, f"{len(bad)} entries differ, first {bad[:5]}: {a[bad[0]]} vs {b[bad[0]]}"
    records = lambda table: np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint32)), shape=(n, 8))[:, :5]  # noqa: E731
    ra, rb = records(host.desc.contents.spheres)[a[sphere, 5]], records(arr)[b[sphere, 5]]
    bad = np.nonzero((ra != rb).any(axis=1))[0]
    assert not bad.size, f"{len(bad)} sphere entries name another sphere, first: {ra[bad[0]]} vs {rb[bad[0]]}"
    assert sorted(b[sphere, 5].tolist()) == list(range(n))
    print(f"{scene}: GPU build {gpu.build_ms:.1f} ms, {len(a)} entries")


# ---- against the independent reference --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
def test_gpu_build_small_worlds(torch_cuda, built, monkeypatch, n):
    """Lists of 1 (left == right), 2 (ordered pair) and odd splits, from randSpheres' first spheres: every entry."""
    host = rtx.HostScene("random_spheres", 3)
    arr, total, draw0, seed = host.world_spheres()
    small = (rtx.Sphere * n)(*[arr[i] for i in range(n)])
    for i in range(n):
        small[i].material %= N_MATERIALS
    entries = check_build(monkeypatch, small, n, seed, 77)
    expect = {1: 2, 2: 3}.get(n)
    if expect:
        assert len(entries) == expect


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_gpu_build_sizes_and_ties(torch_cuda, built, monkeypatch, n, pattern):
    k = SIZES.index(n)
    check_build(monkeypatch, world_of(pattern, n, 1000 + n), n, SEEDS[k % 3], DRAWS[(k // 3) % 3])


@pytest.mark.gpu
def test_gpu_build_multi_block_ties(torch_cuda, built, monkeypatch):
    """65 537 spheres at 64 places: about a thousand exact ties per key through hipCUB's multi-block passes."""
    n = 65537
    arr = world_of("quantised", n, 65537)
    desc, want = reference(arr, n, SEEDS[1], DRAWS[1])
    monkeypatch.setenv("RTX_BVH", "reference")
    dev = gpu_scene(arr, n, SEEDS[1], DRAWS[1])
    try:
        same_entries(dev.export(), want, "65537 quantised")
    finally:
        dev.close()


def float_edges(shuffle_seed: int):
    """A few dozen spheres at the edges of float32; no NaN arises (no inf - inf in a box, no 0 * inf)."""
    inf, big, sub = float("inf"), 3.0e38, 1.0e-45
    S = []  # (centre, radius)
    # box minima of -0 (centre -0, radius 0: -0 + -0) and of +0 (centre r, radius r: r + -r), per axis
    S += [((-0.0, -0.0, -0.0), 0.0), ((0.5, 0.5, 0.5), 0.5), ((-0.0, 2.0, 1.0), 0.0), ((1.0, -0.0, 2.0), 1.0),
          ((2.0, 1.0, -0.0), 0.0), ((0.0, 0.0, 0.0), 0.0), ((2.0, 2.0, 2.0), 2.0), ((-0.0, -0.0, 3.0), 0.0)]
    # negative and zero radii: NewAabb orders the corners, the leaf keeps r * r
    S += [((1.0, 2.0, 3.0), -0.5), ((-1.0, 0.5, 0.25), -1.0), ((0.5, 0.5, 0.5), -0.5), ((3.0, -2.0, 1.0), 0.0),
          ((3.0, -2.0, 1.0), -0.0), ((-2.0, -2.0, -2.0), -2.0)]
    # subnormal centres and radii: differences of subnormals are exact and non-zero
    S += [((sub, -sub, 2 * sub), 0.0), ((-sub, sub, 3 * sub), 0.0), ((2 * sub, 2 * sub, -sub), sub), ((1.0e-40, -3.0e-39, 0.0), 0.0),
          ((-1.0e-40, 3.0e-39, sub), 1.0e-41), ((0.0, sub, -0.0), 0.0), ((5.0e-39, 5.0e-39, 5.0e-39), 5.0e-39)]
    # |centre| near 3e38: b.min - a.min overflows to an infinity, which still has the right sign
    S += [((big, -big, big), 1.0e37), ((-big, big, -big), 1.0e37), ((big, big, -big), 0.0), ((-big, -big, big), 2.0e37),
          ((3.3e38, -3.3e38, 0.0), 1.0e36), ((big, -big, big), 1.0e37)]
    # infinite centres with a finite radius: inf +- r = inf; two equal infinities compare equal (inf - inf is NaN)
    S += [((inf, 0.0, -inf), 1.0), ((-inf, inf, 1.0), 0.5), ((inf, 1.0, 2.0), 2.0), ((inf, -1.0, -inf), 0.0),
          ((0.0, -inf, inf), 1.0), ((-inf, -inf, -inf), 3.0), ((inf, inf, inf), 0.25), ((1.0, 2.0, inf), 1.0)]
    # ordinary spheres among them
    S += [((0.25 * i - 2.0, 1.0 - 0.5 * i, 0.125 * i * i), 0.25 + 0.125 * (i % 3)) for i in range(10)]
    rng = np.random.default_rng(shuffle_seed)
    order = rng.permutation(len(S))
    old = np.seterr(all="ignore")
    try:
        return sphere_table([S[i][0] for i in order], [S[i][1] for i in order], rng.integers(0, N_MATERIALS, len(S)))
    finally:
        np.seterr(**old)


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [11, 12, 13])
def test_gpu_build_float_edges(torch_cuda, built, monkeypatch, shuffle):
    arr = float_edges(shuffle)
    want = check_build(monkeypatch, arr, len(arr), SEEDS[shuffle % 3], DRAWS[shuffle % 2])
    boxes = want[want[:, 7].view(np.int32) == -1][:, [0, 1, 2, 4, 5, 6]]
    assert (boxes == 0x80000000).any() and (boxes == 0).any()  # both zeros reach node boxes
    assert not np.isnan(want.view(F32)[:, :3]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("draw0", DRAWS)
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_build_streams(torch_cuda, built, monkeypatch, seed, draw0):
    """Every seed with every draw position, 100 quantised spheres (127 NewBVH calls: 32 Philox blocks)."""
    check_build(monkeypatch, world_of("quantised", 100, 7), 100, seed, draw0)
    assert bvh_ref.calls(100) == 127


@pytest.mark.gpu
def test_gpu_built_scene_renders_identically(torch_cuda, built):
    host = rtx.HostScene("random_spheres", 1)
    cam = host.camera(width=160, spp=3)
    ref = rtx.DeviceScene(host.desc).render_host(cam, 4)[0]
    got = rtx.DeviceScene.from_spheres(host).render_host(cam, 4)[0]
    assert np.array_equal(ref, got)


# ---- the blocks on a GPU-built scene ----------------------------------------------------------------------------
BLOCKS_SEED, BLOCKS_DRAW0, RAY_SEED = 0xFFFFFFFF00000001, 5, 0xB10C5
DUP = (3.0, 3.5, 3.0)  # the place of the two coincident spheres, nearest the camera


@functools.lru_cache(maxsize=None)
def blocks_world():
    """40 spheres on a 4 x 4 x 4 grid of places (step 2, radius 0.7: many tied minima), among them two coincident ones
    with different materials at DUP, eight DiffuseLights, one of those with a negative radius (hittable: Sphere.Hit
    squares it; no emitter: rtx.h asks radius > 0); Add order shuffled.  -> (table, n, description, entries, camera)"""
    rng = np.random.default_rng(40)
    grid = np.array([-3.0, -1.0, 1.0, 3.0], F32)
    cells = [(x, y + 2.5, z) for x in grid for y in grid for z in grid if (x, y + 2.5, z) != DUP]
    place = [cells[i] for i in rng.permutation(len(cells))[:38]]
    center = [DUP, DUP] + place
    radius = [0.7, 0.7] + [0.7] * 37 + [-0.7]
    material = [0, 2] + [(0, 1, 2, 3, 0, 1, 4, 2, 0, 5)[i % 10] for i in range(37)] + [4]
    order = rng.permutation(40)
    arr = sphere_table([center[i] for i in order], [radius[i] for i in order], [material[i] for i in order])
    desc, entries = reference(arr, 40, BLOCKS_SEED, BLOCKS_DRAW0)
    walk_order = entries[entries[:, 7].view(np.int32) >= 0, 5]
    assert sorted(walk_order.tolist()) == list(range(40)) and (walk_order != np.arange(40)).sum() > 30
    cam = ob.camera(F32(16.0 / 9.0), 64, samples_per_pixel=1, max_depth=6, look_from=(10, 7, 12), look_at=(0, 2.5, 0),
                    fov_degrees=40, defocus_degrees=0, background=(0.1, 0.15, 0.3))
    return arr, 40, desc, entries, cam


@functools.lru_cache(maxsize=None)
def blocks_rays():
    """64 x 36 camera rays, then 1800 incoherent ones, each with its own interval."""
    arr, n, desc, entries, cam = blocks_world()
    rays, keys = rtx.camera_rays(cam, RAY_SEED, rtx.Region(0, 0, 64, 36, 0, 1), 0, 1)
    rays, keys = rays.reshape(-1).copy(), keys.reshape(-1).copy()
    rng = np.random.default_rng(41)
    m = 1800
    d = rng.normal(size=(m, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (m, 1))
    more = np.zeros(m, rtx.RAY_DTYPE)
    more["origin"], more["dir"] = rng.uniform((-5, -2, -5), (5, 7, 5), (m, 3)), d
    more["tmin"] = np.array([-1, 0, 0.001, 0.5], F32)[rng.integers(0, 4, m)]
    more["tmax"] = np.where(rng.random(m) < 0.5, np.inf, rng.uniform(0, 30, m) / np.linalg.norm(d, axis=1))
    return np.concatenate([rays, more]), keys


def trace_dev(torch, dev, rays, flags):
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros((len(rays) * 48,), dtype=torch.uint8, device="cuda")
    dev.trace_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(rtx.HIT_DTYPE)


def direct_dev(torch, dev, hits, keys, seed):
    d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (hits, keys)]
    out = torch.zeros((len(hits) * 64,), dtype=torch.uint8, device="cuda")
    dev.direct_device(seed, d[0].data_ptr(), d[1].data_ptr(), len(hits), out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(rtx.DIRECT_DTYPE)


@pytest.fixture(params=["default", "reference"])
def blocks(request, torch_cuda, built, monkeypatch):
    """(GPU-built scene, rtx_scene_create of the reference's description) under one RTX_BVH setting."""
    if request.param == "reference":
        monkeypatch.setenv("RTX_BVH", "reference")
    arr, n, desc, entries, cam = blocks_world()
    gpu, made = gpu_scene(arr, n, BLOCKS_SEED, BLOCKS_DRAW0), rtx.DeviceScene(desc)
    yield gpu, made
    gpu.close()
    made.close()


@pytest.mark.gpu
def test_blocks_closest_and_any_hit(torch_cuda, blocks):
    """Every field of every hit bit-equal to trace_ref.walk over the reference's entries: prim is the Add-order index,
    and on the coincident pair the one the reference walk meets first."""
    gpu, made = blocks
    arr, n, desc, entries, cam = blocks_world()
    rays, _ = blocks_rays()
    w = trace_ref.walk(trace_ref.Scene(entries, desc), rays, F32, uv=True)
    want = w.records(uv=True)
    pair = [i for i in range(n) if tuple(arr[i].center) == DUP]
    first = next(int(p) for p in entries[entries[:, 7].view(np.int32) >= 0, 5] if int(p) in pair)
    assert len(pair) == 2 and (want["prim"] == first).sum() > 20 and not (want["prim"] == sum(pair) - first).any()
    assert w.mask.sum() > 900 and (~w.mask).sum() > 500
    same_entries(gpu.export(), entries, "the GPU-built scene")
    for name, dev in (("GPU-built", gpu), ("rtx_scene_create", made)):
        got = trace_dev(torch_cuda, dev, rays, rtx.RTX_TRACE_UV)
        bad = np.nonzero((got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12)).any(axis=1))[0]
        wrong_prim = int((got["prim"] != want["prim"]).sum())
        print(f"{name}: {len(bad)} of {len(rays)} hits differ, {wrong_prim} in prim")
        assert not bad.size, (name, len(bad), wrong_prim, bad[:5], got[bad[:2]], want[bad[:2]])
        anyhit = trace_dev(torch_cuda, dev, rays, rtx.RTX_TRACE_ANY)
        assert np.array_equal(anyhit["prim"] != rtx.RTX_HIT_NONE, got["prim"] != rtx.RTX_HIT_NONE), name


@pytest.mark.gpu
def test_blocks_lights(torch_cuda, blocks):
    """The emitter table in the caller's table order, the sphere of negative radius left out."""
    gpu, made = blocks
    arr, n, desc, entries, cam = blocks_world()
    want = direct_ref.lights(desc)
    lit = [i for i in range(n) if arr[i].material in (4, 5) and arr[i].radius > 0]
    assert want["prim"].tolist() == lit and len(lit) == 7 and sum(arr[i].material in (4, 5) for i in range(n)) == 8
    assert rtx.lights(desc).tobytes() == want.tobytes()
    assert made.lights().tobytes() == want.tobytes()
    got = gpu.lights()
    assert got.tobytes() == want.tobytes(), (got, want)


@pytest.mark.gpu
def test_blocks_direct_and_renders(torch_cuda, blocks):
    """rtx_direct_device, wavefront.render (plain and direct) and the megakernel (scene in LDS and in HBM): bit-equal
    between the GPU-built scene and rtx_scene_create of the reference's description."""
    gpu, made = blocks
    arr, n, desc, entries, cam = blocks_world()
    rays, keys = blocks_rays()
    rays = rays[: len(keys)]
    keys = keys.copy()
    keys["event"] = 1
    hits = trace_dev(torch_cuda, made, rays, rtx.RTX_TRACE_UV)
    a, b = direct_dev(torch_cuda, gpu, hits, keys, 77), direct_dev(torch_cuda, made, hits, keys, 77)
    sampled = (b["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
    assert sampled.sum() > 100 and len(np.unique(b["light"][sampled])) == 7
    bad = np.nonzero((a.view(np.uint32).reshape(-1, 16) != b.view(np.uint32).reshape(-1, 16)).any(axis=1))[0]
    assert not bad.size, (len(bad), a[bad[:2]], b[bad[:2]])
    cam = rtx.Camera.from_buffer_copy(cam)
    cam.samples_per_pixel = 3
    region = rtx.Region(14, 8, 36, 20, 0, 1)
    for direct in (False, True):
        x = wavefront.render(gpu, cam, 9, region, direct=direct).cpu().numpy()
        y = wavefront.render(made, cam, 9, region, direct=direct).cpu().numpy()
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), direct
        assert x.max() > 0
    for flags in (0, rtx.RTX_FLAG_NO_LDS):
        out = []
        for dev in (gpu, made):
            t = torch_cuda.zeros((20, 36, 3), dtype=torch_cuda.float32, device="cuda")
            dev.render_region(cam, 9, region, t.data_ptr(), torch_cuda.cuda.current_stream().cuda_stream, flags=flags)
            torch_cuda.cuda.synchronize()
            out.append(t.cpu().numpy())
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), flags
