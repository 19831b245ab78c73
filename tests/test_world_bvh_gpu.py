"""GPU BVH build for whole Worlds: rtx_scene_create_world builds NewBVHFromWorld (bvh.go:138-185) over spheres and quads
in World.Add order on the device.

Its threaded entries are held, byte for byte and index word included, to tests/world_bvh_ref.py, the independent reading
of NewBVH over a mixed list: on lists of every size at which the build takes another path (1, 2, odd splits, the
256-thread launch boundary, hipCUB's multi-block sort), with kinds interleaved by a seeded permutation (about a third
quads) and both tables numbered in another order than the list; with distinct padded minima, with exact ties between
spheres and quads (where only the stability of the sort decides), with every box identical; on the float edges of the
quad's padded box (extents around 0.0001f, signed zeros, subnormals, differences that overflow, infinities).  NaN boxes
are out of contract (the reference refuses them): none is generated, and that is asserted.

A World of spheres through the new entry gives rtx_scene_create_spheres' bytes; the main.go scenes are compared with the
host mirror's build, which numbers its primitives in walk order: the same tree, other labels.  The ray queries, the
emitter table, the light-sample block and the renders are then run on a GPU-built mixed scene whose Add order differs
from every walk order: `prim` must name the CALLER's sphere or quad."""
import ctypes
import functools

import numpy as np
import pytest

import direct_ref
import oracle_binding as ob
import rtx
import trace_ref
import world_bvh_ref
from test_bvh_gpu import DRAWS, N_MATERIALS, SEEDS, direct_dev, float_edges, same_entries, sphere_table, tables, trace_dev
from test_bvh_gpu import world_of as sphere_world_of

F32 = np.float32
SPH, QD = rtx.RTX_PRIM_SPHERE, rtx.RTX_PRIM_QUAD
QUAD_TAG = -2
SIZES = list(range(1, 10)) + [255, 256, 257, 1000, 4097]
PATTERNS = ("distinct", "quantised", "identical", "alternating")
EPS = float(F32(0.0001))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


# ---- inputs and the two builds ----------------------------------------------------------------------------------
def quad_table(Q, u, v, material):
    """NewQuad per row through rtx_quad_init (held to NewQuad in numpy by test_world_bvh_ref.py)."""
    arr = (rtx.Quad * len(material))()
    with np.errstate(all="ignore"):
        for i in range(len(material)):
            arr[i] = rtx.quad(Q[i], u[i], v[i], int(material[i]))
    return arr


def interleave(rng, n_spheres, n_quads):
    """The World's list: the kinds in a seeded order, and each kind's table numbered by its own seeded permutation,
    so that an item's index is neither its list position nor its rank among its kind."""
    kind = np.array([SPH] * n_spheres + [QD] * n_quads)[rng.permutation(n_spheres + n_quads)]
    index = np.zeros(len(kind), np.int64)
    index[kind == SPH], index[kind == QD] = rng.permutation(n_spheres), rng.permutation(n_quads)
    return [rtx.ref_prim(int(k), int(i)) for k, i in zip(kind, index)], kind, index


def world_of(pattern: str, n: int, seed: int):
    """(items, spheres, quads) of n items, about a third of them quads (a list of one is a quad).
    distinct: places on a permuted grid of step 1/8 per axis; spheres with radii of 1, 3 or 5 sixty-fourths, quads with
      edges of a few 1/256: no two padded minima are equal on any axis (asserted).
    quantised: four positions per axis; spheres of radius 0.75 and axis-aligned quads of side 1.5 whose corner is a
      sphere's box corner, so spheres and quads tie exactly on the quad's two long axes, quads among themselves on all.
    identical: one quad, n times (n records).
    alternating: a quad whose corners span the cube [0, 1.5]^3 and the sphere with that box, in turn."""
    rng = np.random.default_rng(seed)
    nq = max(1, round(n / 3))
    ns = n - nq
    if pattern == "identical":
        ns, nq = 0, n
    elif pattern == "alternating":
        ns, nq = n // 2, n - n // 2
    items, kind, index = interleave(rng, ns, nq)
    pos_s, pos_q = np.nonzero(kind == SPH)[0], np.nonzero(kind == QD)[0]
    center, radius = np.zeros((ns, 3), F32), np.zeros(ns, F32)
    Q, u, v = np.zeros((nq, 3), F32), np.zeros((nq, 3), F32), np.zeros((nq, 3), F32)
    if pattern == "distinct":
        place = np.stack([rng.permutation(n) - n // 2 for _ in range(3)], axis=1).astype(F32) * F32(0.125)
        center[index[pos_s]] = place[pos_s]
        radius[:] = (F32(1) + F32(2) * rng.integers(0, 3, ns).astype(F32)) * F32(1 / 64)
        Q[index[pos_q]] = place[pos_q]
        u[:], v[:] = rng.integers(-7, 8, (nq, 3)) / 256.0, rng.integers(-7, 8, (nq, 3)) / 256.0
        flat = ~np.cross(u, v).any(axis=1)  # a degenerate quad has a NaN normal: take a small square instead
        u[flat], v[flat] = (1 / 256, 0, 0), (0, 1 / 256, 0)
    elif pattern == "quantised":
        grid = np.array([-4.5, -1.5, 1.5, 4.5], F32)
        center[:], radius[:] = grid[rng.integers(0, 4, (ns, 3))], 0.75
        corner = grid[rng.integers(0, 4, (nq, 3))] - F32(0.75)  # a sphere's box minimum
        axes3 = np.array([rng.permutation(3) for _ in range(nq)]).reshape(nq, 3)
        down = rng.integers(0, 2, (nq, 2)).astype(bool)  # an edge may run from the far corner back
        for i in range(nq):
            a, b = axes3[i, 0], axes3[i, 1]
            Q[i] = corner[i]
            u[i, a], v[i, b] = 1.5, 1.5
            if down[i, 0]:
                Q[i, a], u[i, a] = Q[i, a] + F32(1.5), -1.5
            if down[i, 1]:
                Q[i, b], v[i, b] = Q[i, b] + F32(1.5), -1.5
    elif pattern == "identical":
        Q[:], u[:], v[:] = (1.5, -2.25, 0.5), (0, 1.5, 0), (0.75, 0, -1.5)
    else:
        center[:], radius[:] = (0.75, 0.75, 0.75), 0.75
        Q[:], u[:], v[:] = (0, 0, 0), (1.5, 0, 0), (0, 1.5, 1.5)
    mat_s, mat_q = rng.integers(0, N_MATERIALS, ns), rng.integers(0, N_MATERIALS, nq)
    if pattern in ("identical", "alternating"):
        mat_s[:], mat_q[:] = 2, 0
    spheres = sphere_table(center, radius, mat_s) if ns else None
    quads = quad_table(Q, u, v, mat_q)
    bmin, bmax = world_bvh_ref.item_boxes(items, spheres, quads)
    assert not np.isnan(bmin).any() and not np.isnan(bmax).any()
    if pattern == "distinct":
        assert all(len(np.unique(bmin[:, a])) == n for a in range(3))
    elif pattern == "quantised" and n >= 257:
        for a in range(3):  # exact ties between a sphere and a quad on every axis
            assert np.intersect1d(bmin[pos_s, a], bmin[pos_q, a]).size
    elif pattern in ("identical", "alternating"):
        assert (bmin == bmin[0]).all() and (bmax == bmax[0]).all()
    return items, spheres, quads


def reference(items, spheres, quads, seed, draw0):
    """(description, entries) of the independent build."""
    desc = world_bvh_ref.build(items, spheres, quads, seed, draw0, tables=tables())
    return desc, trace_ref.entries_of(desc)


def gpu_scene(items, spheres, quads, seed, draw0) -> rtx.DeviceScene:
    """rtx_scene_create_world over the caller's tables (RTX_BVH is read here)."""
    return rtx.DeviceScene.from_tables(items, spheres, quads, tables(), seed, draw0)


def check_build(monkeypatch, items, spheres, quads, seed, draw0):
    """RTX_BVH=reference: the export is the reference's entries.  Default tree: it is the export of the scene
    rtx_scene_create makes from the reference's description (and so the same bytes again)."""
    n = len(items)
    desc, want = reference(items, spheres, quads, seed, draw0)
    monkeypatch.setenv("RTX_BVH", "reference")
    dev = gpu_scene(items, spheres, quads, seed, draw0)
    try:
        same_entries(dev.export(), want, f"n {n}, RTX_BVH=reference")
    finally:
        dev.close()
    monkeypatch.delenv("RTX_BVH")
    dev, made = gpu_scene(items, spheres, quads, seed, draw0), rtx.DeviceScene(desc)
    try:
        assert dev.build_ms > 0
        same_entries(dev.export(), np.frombuffer(made.export(), np.uint32), f"n {n}, default tree")
        same_entries(made.export(), want, f"n {n}, rtx_scene_create")
    finally:
        dev.close()
        made.close()
    return want


# ---- against the independent reference --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_world_build_sizes_and_ties(torch_cuda, built, monkeypatch, n, pattern):
    k = SIZES.index(n)
    want = check_build(monkeypatch, *world_of(pattern, n, 2000 + n), SEEDS[k % 3], DRAWS[(k // 3) % 3])
    if n == 1:
        assert len(want) == 2 and want[1, 7].view(np.int32) == QUAD_TAG  # one quad: left == right, emitted once


@pytest.mark.gpu
def test_world_build_multi_block_ties(torch_cuda, built, monkeypatch):
    """65 537 quantised items: about a thousand exact ties per key through hipCUB's multi-block passes."""
    items, spheres, quads = world_of("quantised", 65537, 65537)
    desc, want = reference(items, spheres, quads, SEEDS[1], DRAWS[1])
    monkeypatch.setenv("RTX_BVH", "reference")
    dev = gpu_scene(items, spheres, quads, SEEDS[1], DRAWS[1])
    try:
        same_entries(dev.export(), want, "65537 quantised")
    finally:
        dev.close()


def quad_float_edges(shuffle_seed: int):
    """Quads at the edges of the padded box's arithmetic, spheres among them; no NaN arises."""
    inf, big, sub = float("inf"), 3.0e38, 1.0e-45
    below, above = float(np.nextafter(F32(EPS), F32(0))), float(np.nextafter(F32(EPS), F32(1)))
    E = np.eye(3)
    Qs = []  # (Q, u, v)
    # extents of exactly 0, the float32 below 0.0001f, 0.0001f and the one above, on each axis; Q = 0: hi - lo is exact
    for a in range(3):
        for ext in (0.0, below, EPS, above, -below, -EPS, -above):
            Qs.append(((0.0, 0.0, 0.0), tuple(ext * E[a] + 2.0 * E[(a + 1) % 3]), tuple(3.0 * E[(a + 2) % 3])))
    # negative components and -0 in u and v (Min(-0, +0) = -0: the box keeps the sign)
    Qs += [((1.0, 2.0, 3.0), (-1.0, -0.0, 0.5), (0.25, -2.0, -0.0)), ((0.0, 0.0, 0.0), (-0.0, -1.0, -0.0), (-0.0, -0.0, -1.0)),
           ((-0.0, -0.0, -0.0), (-0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), ((0.5, -0.5, 0.0), (-0.5, 0.5, -0.0), (-0.0, -0.0, 2.0)),
           ((-1.0, -1.0, -1.0), (-2.0, -3.0, -0.0), (-0.0, -1.0, -4.0))]
    # subnormal extents (padded: they are below eps) and subnormal corners
    Qs += [((0.0, 0.0, 0.0), (sub, 1.0, 0.0), (0.0, 0.0, sub)), ((sub, -sub, 0.0), (3.0e-39, 0.0, 1.0), (0.0, -1.0e-40, 0.0)),
           ((-3.0e-39, 1.0e-41, sub), (sub, sub, 0.0), (0.0, sub, 2 * sub))]
    # |Q| near 3e38 with a finite far corner: b.min - a.min overflows to an infinity of the right sign
    Qs += [((big, -big, big), (1.0e37, 0.0, 0.0), (0.0, 1.0e37, 0.0)), ((-big, big, -big), (0.0, -1.0e37, 0.0), (0.0, 0.0, 1.0e37)),
           ((big, big, -big), (2.0e37, 0.0, 0.0), (0.0, 0.0, -2.0e37)), ((-big, -big, big), (-2.0e37, 0.0, 0.0), (0.0, -1.0e37, 1.0e37))]
    # an infinite Q component with finite edges: lo = hi = inf, hi - lo is NaN, the comparison false: no padding
    Qs += [((inf, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), ((-inf, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 2.0)),
           ((0.0, inf, -inf), (1.0, 0.0, 0.0), (0.0, 3.0, 1.0)), ((inf, 2.0, 1.0), (5.0, 0.0, 1.0), (0.0, 1.0, 0.0))]
    # ordinary quads and spheres among them
    Qs += [((0.25 * i - 2.0, 1.0 - 0.5 * i, 0.125 * i * i), (1.0, 0.25 * i, 0.0), (0.0, 1.0, 0.5)) for i in range(6)]
    S = [((0.25 * i - 1.0, 0.5 * i, 0.125 * i), 0.25 + 0.125 * (i % 3)) for i in range(8)]
    S += [((0.0, 0.0, 0.0), EPS), ((-0.0, -0.0, -0.0), 0.0), ((big, -big, big), 1.0e37), ((inf, 0.0, -inf), 1.0), ((sub, -sub, 0.0), sub)]
    rng = np.random.default_rng(shuffle_seed)
    items, kind, index = interleave(rng, len(S), len(Qs))
    with np.errstate(all="ignore"):
        spheres = sphere_table([S[i][0] for i in range(len(S))], [S[i][1] for i in range(len(S))],
                               rng.integers(0, N_MATERIALS, len(S)))
        quads = quad_table([q[0] for q in Qs], [q[1] for q in Qs], [q[2] for q in Qs], rng.integers(0, N_MATERIALS, len(Qs)))
    return items, spheres, quads


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [21, 22, 23])
def test_world_build_quad_float_edges(torch_cuda, built, monkeypatch, shuffle):
    items, spheres, quads = quad_float_edges(shuffle)
    bmin, bmax = world_bvh_ref.item_boxes(items, spheres, quads)
    assert not np.isnan(bmin).any() and not np.isnan(bmax).any()  # no NaN arises
    assert np.isinf(bmin).any() and (bmin.view(np.uint32) == 0x80000000).any()
    ext = (bmax - bmin)[np.isfinite(bmin).all(axis=1) & np.isfinite(bmax).all(axis=1)]
    assert (ext == F32(EPS)).any() and (ext == F32(2) * F32(EPS)).any()  # an unpadded eps and a padded 0
    want = check_build(monkeypatch, items, spheres, quads, SEEDS[shuffle % 3], DRAWS[shuffle % 2])
    nodes = want[want[:, 7].view(np.int32) == -1]
    assert not np.isnan(nodes.view(F32)[:, [0, 1, 2, 4, 5, 6]]).any()


# ---- a World of spheres: the old entry's bytes --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quantised 257", "distinct 1000", "float edges", "one"])
def test_sphere_world_equals_create_spheres(torch_cuda, built, monkeypatch, case):
    """items == NULL with no quads: every sphere in table order.  The same bytes as rtx_scene_create_spheres."""
    if case == "float edges":
        arr = float_edges(12)
    else:
        pattern, n = ("quantised", 1) if case == "one" else (case.split()[0], int(case.split()[1]))
        arr = sphere_world_of(pattern, n, 31)
    n, t = len(arr), tables().contents
    for bvh in ("reference", None):
        if bvh:
            monkeypatch.setenv("RTX_BVH", bvh)
        else:
            monkeypatch.delenv("RTX_BVH")
        h = ctypes.c_void_p()
        rtx.check(rtx.load().rtx_scene_create_spheres(arr, n, t.materials, t.n_materials, t.textures, t.n_textures, t.texels,
                                                      t.n_texels, SEEDS[1], DRAWS[1], ctypes.byref(h), None),
                  "rtx_scene_create_spheres")
        old, new = rtx.DeviceScene(handle=h), gpu_scene(None, arr, None, SEEDS[1], DRAWS[1])
        explicit = gpu_scene([rtx.ref_prim(SPH, i) for i in range(n)], arr, None, SEEDS[1], DRAWS[1])
        try:
            assert new.export() == old.export() == explicit.export(), (case, bvh)
        finally:
            for d in (old, new, explicit):
                d.close()


# ---- the main.go scenes against the host mirror -----------------------------------------------------------------
def records(table, n, per):
    if n == 0:
        return np.zeros((0, per), np.uint32)
    return np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint32)), shape=(n, per))


HOST_SCENES = ["cornell_box", "quad_demo", "simple_light_demo", "random_spheres", "earth_dielectric", "earth", "earth_rgba",
               "earth_far_side", "perlin_demo", "stress_100k"]


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", ["reference", "default"])
@pytest.mark.parametrize("scene", HOST_SCENES)
def test_world_build_equals_host_build(torch_cuda, built, monkeypatch, scene, bvh):
    """The GPU build against rtx_scene_create of the host mirror's tree.  The mirror's tables are in walk order, the
    caller's in Add order, so a leaf's index word differs; every other word is equal, and through the index word both
    entries name the same record."""
    if bvh == "reference":
        monkeypatch.setenv("RTX_BVH", "reference")
    host = rtx.HostScene(scene, 1)
    items, spheres, quads, _, _ = host.world()
    d = host.desc.contents
    ref, gpu = rtx.DeviceScene(host.desc), rtx.DeviceScene.from_world(host)
    try:
        a = np.frombuffer(ref.export(), np.uint32).reshape(-1, 8)
        b = np.frombuffer(gpu.export(), np.uint32).reshape(-1, 8)
    finally:
        ref.close()
        gpu.close()
    assert a.shape == b.shape
    tag = a[:, 7].view(np.int32)
    assert np.array_equal(tag, b[:, 7].view(np.int32))
    sphere, quad = tag >= 0, tag == QUAD_TAG
    mask = np.ones(a.shape, bool)
    mask[sphere, 5] = False
    mask[quad, 4] = False
    bad = np.nonzero(((a != b) & mask).any(axis=1))[0]
    assert not bad.size, f"{len(bad)} entries differ, first {bad[:5]}: {a[bad[0]]} vs {b[bad[0]]}"
    ns, nq = len(spheres), len(quads)
    assert (ns, nq) == (d.n_spheres, d.n_quads)
    ra, rb = records(d.spheres, ns, 8)[a[sphere, 5]][:, :5], records(spheres, ns, 8)[b[sphere, 5]][:, :5]
    assert np.array_equal(ra, rb), "a sphere entry names another sphere"
    ra, rb = records(d.quads, nq, 20)[a[quad, 4]], records(quads, nq, 20)[b[quad, 4]]
    assert np.array_equal(ra, rb), "a quad entry names another quad"
    assert sorted(b[sphere, 5].tolist()) == list(range(ns)) and sorted(b[quad, 4].tolist()) == list(range(nq))
    print(f"{scene}: GPU build {gpu.build_ms:.1f} ms, {len(a)} entries")


# ---- the blocks on a GPU-built mixed scene ------------------------------------------------------------------------
BLOCKS_SEED, BLOCKS_DRAW0, RAY_SEED = 0xFFFFFFFF00000001, 5, 0xB10C5


@functools.lru_cache(maxsize=None)
def blocks_world():
    """26 spheres (radius 0.7) and 14 axis-aligned square quads (side 1.4) at 40 places of a 4 x 4 x 4 grid of step 2
    (many tied minima); seven DiffuseLights among them, five spheres (one of negative radius: hittable, no emitter)
    and three quads; Add order and both table orders shuffled.  -> (items, spheres, quads, description, entries,
    camera)"""
    rng = np.random.default_rng(44)
    grid = np.array([-3.0, -1.0, 1.0, 3.0], F32)
    cells = [(x, y + 2.5, z) for x in grid for y in grid for z in grid]
    place = np.array([cells[i] for i in rng.permutation(len(cells))[:40]], F32)
    ns, nq = 26, 14
    items, kind, index = interleave(rng, ns, nq)
    pos_s, pos_q = np.nonzero(kind == SPH)[0], np.nonzero(kind == QD)[0]
    center, radius, mat_s = np.zeros((ns, 3), F32), np.full(ns, 0.7, F32), np.zeros(ns, np.int64)
    center[index[pos_s]] = place[pos_s]
    mat_s[:] = [(0, 1, 2, 3, 4, 1, 0, 2, 5, 0)[i % 10] for i in range(ns)]
    radius[4] = -0.7  # material 4: a light that is no emitter
    Q, u, v, mat_q = np.zeros((nq, 3), F32), np.zeros((nq, 3), F32), np.zeros((nq, 3), F32), np.zeros(nq, np.int64)
    for k, p in enumerate(pos_q):
        i = index[p]
        a, b = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)][k % 6]
        Q[i] = place[p]
        Q[i, a] -= F32(0.7)
        Q[i, b] -= F32(0.7)
        u[i, a], v[i, b] = 1.4, 1.4
        mat_q[i] = (0, 4, 1, 2, 5, 0, 3)[k % 7]
    spheres, quads = sphere_table(center, radius, mat_s), quad_table(Q, u, v, mat_q)
    desc, entries = reference(items, spheres, quads, BLOCKS_SEED, BLOCKS_DRAW0)
    tag = entries[:, 7].view(np.int32)
    walk_s, walk_q = entries[tag >= 0, 5], entries[tag == QUAD_TAG, 4]
    assert sorted(walk_s.tolist()) == list(range(ns)) and (walk_s != np.arange(ns)).sum() > 18
    assert sorted(walk_q.tolist()) == list(range(nq)) and (walk_q != np.arange(nq)).sum() > 8
    add_s, add_q = index[pos_s], index[pos_q]  # Add order is no table order either
    assert (add_s != np.arange(ns)).sum() > 18 and (add_q != np.arange(nq)).sum() > 8
    cam = ob.camera(F32(16.0 / 9.0), 64, samples_per_pixel=1, max_depth=6, look_from=(10, 7, 12), look_at=(0, 2.5, 0),
                    fov_degrees=40, defocus_degrees=0, background=(0.1, 0.15, 0.3))
    return items, spheres, quads, desc, entries, cam


@functools.lru_cache(maxsize=None)
def blocks_rays():
    """64 x 36 camera rays, then 1800 incoherent ones, each with its own interval."""
    cam = blocks_world()[5]
    rays, keys = rtx.camera_rays(cam, RAY_SEED, rtx.Region(0, 0, 64, 36, 0, 1), 0, 1)
    rays, keys = rays.reshape(-1).copy(), keys.reshape(-1).copy()
    rng = np.random.default_rng(45)
    m = 1800
    d = rng.normal(size=(m, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (m, 1))
    more = np.zeros(m, rtx.RAY_DTYPE)
    more["origin"], more["dir"] = rng.uniform((-5, -2, -5), (5, 7, 5), (m, 3)), d
    more["tmin"] = np.array([-1, 0, 0.001, 0.5], F32)[rng.integers(0, 4, m)]
    more["tmax"] = np.where(rng.random(m) < 0.5, np.inf, rng.uniform(0, 30, m) / np.linalg.norm(d, axis=1))
    return np.concatenate([rays, more]), keys


@pytest.fixture(params=["default", "reference"])
def blocks(request, torch_cuda, built, monkeypatch):
    """(GPU-built scene, rtx_scene_create of the reference's description) under one RTX_BVH setting."""
    if request.param == "reference":
        monkeypatch.setenv("RTX_BVH", "reference")
    items, spheres, quads, desc, entries, cam = blocks_world()
    gpu, made = gpu_scene(items, spheres, quads, BLOCKS_SEED, BLOCKS_DRAW0), rtx.DeviceScene(desc)
    yield gpu, made
    gpu.close()
    made.close()


@pytest.mark.gpu
def test_blocks_closest_and_any_hit(torch_cuda, blocks):
    """Every field of every hit bit-equal to trace_ref.walk over the reference's entries: prim is the caller's sphere or
    quad (type << 28 | table index)."""
    gpu, made = blocks
    items, spheres, quads, desc, entries, cam = blocks_world()
    rays, _ = blocks_rays()
    w = trace_ref.walk(trace_ref.Scene(entries, desc), rays, F32, uv=True)
    want = w.records(uv=True)
    hit = want["prim"] != rtx.RTX_HIT_NONE
    on_quad = hit & ((want["prim"] >> 28) == QD)
    assert on_quad.sum() > 100 and (hit & ~on_quad).sum() > 400 and (~hit).sum() > 500
    assert len(np.unique(want["prim"][on_quad])) >= 8
    same_entries(gpu.export(), entries, "the GPU-built scene")
    for name, dev in (("GPU-built", gpu), ("rtx_scene_create", made)):
        got = trace_dev(torch_cuda, dev, rays, rtx.RTX_TRACE_UV)
        bad = np.nonzero((got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12)).any(axis=1))[0]
        wrong_prim = int((got["prim"] != want["prim"]).sum())
        print(f"{name}: {len(bad)} of {len(rays)} hits differ, {wrong_prim} in prim")
        assert not bad.size, (name, len(bad), wrong_prim, bad[:5], got[bad[:2]], want[bad[:2]])
        anyhit = trace_dev(torch_cuda, dev, rays, rtx.RTX_TRACE_ANY)
        assert np.array_equal(anyhit["prim"] != rtx.RTX_HIT_NONE, hit), name


@pytest.mark.gpu
def test_blocks_lights(torch_cuda, blocks):
    """The emitter table in the caller's table order: spheres, then quads; the sphere of negative radius left out."""
    gpu, made = blocks
    items, spheres, quads, desc, entries, cam = blocks_world()
    want = direct_ref.lights(desc)
    lit_s = [i for i in range(len(spheres)) if spheres[i].material in (4, 5) and spheres[i].radius > 0]
    lit_q = [(QD << 28) | i for i in range(len(quads)) if quads[i].material in (4, 5)]
    assert want["prim"].tolist() == lit_s + lit_q and len(lit_s) == 4 and len(lit_q) == 4
    assert sum(spheres[i].material in (4, 5) for i in range(len(spheres))) == 5
    assert rtx.lights(desc).tobytes() == want.tobytes()
    assert made.lights().tobytes() == want.tobytes()
    got = gpu.lights()
    assert got.tobytes() == want.tobytes(), (got, want)


@pytest.mark.gpu
def test_blocks_direct(torch_cuda, blocks):
    """rtx_direct_device on the hits of the camera rays and of the incoherent ones (keys of their own): bit-equal to
    direct_ref.sample over the reference's description."""
    gpu, made = blocks
    items, spheres, quads, desc, entries, cam = blocks_world()
    rays, keys = blocks_rays()
    more = np.zeros(len(rays) - len(keys), rtx.KEY_DTYPE)
    more["pixel"], more["sample"] = 5000 + np.arange(len(more)), np.arange(len(more)) % 3
    keys = np.concatenate([keys, more])
    keys["event"] = 1
    hits = trace_dev(torch_cuda, made, rays, rtx.RTX_TRACE_UV)
    want = direct_ref.sample(desc, entries, hits, keys, 77)
    sampled = (want["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
    assert sampled.sum() > 100 and len(np.unique(want["light"][sampled])) == 8
    for name, dev in (("GPU-built", gpu), ("rtx_scene_create", made)):
        got = direct_dev(torch_cuda, dev, hits, keys, 77)
        bad = np.nonzero((got.view(np.uint32).reshape(-1, 16) != want.view(np.uint32).reshape(-1, 16)).any(axis=1))[0]
        assert not bad.size, (name, len(bad), got[bad[:2]], want[bad[:2]])


# ---- the Cornell box: GPU-built against host-built ----------------------------------------------------------------
COUNTERS = ("samples", "segments", "node_visits", "prim_tests", "hits", "texel_fetches", "rng_draws")


@pytest.mark.gpu
def test_cornell_window_renders_identically(torch_cuda, built):
    """A 24 x 20 window of cornell_box at 4 spp from the GPU-built scene and from the host-built one: the same image
    and the same seven work counters; one add_mis pass on both gives the same bytes."""
    host = rtx.HostScene("cornell_box", 1)
    cam = host.camera(width=64, spp=4, depth=8)
    region = rtx.Region(20, 22, 24, 20, 0, 1)
    ref, gpu = rtx.DeviceScene(host.desc), rtx.DeviceScene.from_world(host)
    try:
        out = []
        for dev in (ref, gpu):
            acc = rtx.Accumulator(dev, cam, 9, region)
            st = acc.add(4, counters=True)
            rgb = acc.resolve()[0]
            acc.close()
            mis = rtx.Accumulator(dev, cam, 9, region)
            mis.add_mis(1, stats=True)
            out.append((rgb, [getattr(st, c) for c in COUNTERS], mis.resolve()[0]))
            mis.close()
        assert out[0][0].shape == (20, 24, 3) and out[0][0].max() > 0 and out[0][2].max() > 0
        assert out[0][0].tobytes() == out[1][0].tobytes()
        assert out[0][1] == out[1][1] and out[0][1][0] > 0 and out[0][1][3] > 0, (out[0][1], out[1][1])
        assert out[0][2].tobytes() == out[1][2].tobytes()
    finally:
        ref.close()
        gpu.close()


# ---- primitives named twice or not at all -------------------------------------------------------------------------
@pytest.mark.gpu
def test_named_twice_and_not_at_all(torch_cuda, built, monkeypatch):
    """A quad and a sphere named twice give two entries each (the same Hittable added twice); an emitter quad and an
    emitter sphere no item names are uploaded but absent from the walk and from the emitter table.  (Seed 1 at draw 0
    puts no two items that name one primitive under one pair node: a description reads such a node's left == right
    as the one-element split and emits its child once, the one corner where rtx_scene_create cannot say what the
    build does.)"""
    spheres = sphere_table([(0, 0, 0), (3, 0, 0), (0, 9, 0)], [1.0, 0.5, 1.0], [0, 4, 5])
    quads = quad_table([(-1, -1, 2), (0, 5, 0), (4, 4, 4)], [(2, 0, 0), (1, 0, 0), (1, 0, 0)], [(0, 2, 0), (0, 0, 1), (0, 1, 0)],
                       [1, 4, 5])
    S, Q = (lambda i: rtx.ref_prim(SPH, i)), (lambda i: rtx.ref_prim(QD, i))
    items = [Q(0), S(1), S(0), Q(0), Q(1), S(1)]  # sphere 2 and quad 2, both emitters, are named by no item
    want = check_build(monkeypatch, items, spheres, quads, 1, 0)
    tag = want[:, 7].view(np.int32)
    assert (tag != -1).sum() == len(items)
    assert sorted(want[tag >= 0, 5].tolist()) == [0, 1, 1] and sorted(want[tag == QUAD_TAG, 4].tolist()) == [0, 0, 1]
    dev = gpu_scene(items, spheres, quads, 1, 0)
    try:
        got = dev.lights()
        assert got["prim"].tolist() == [1, (QD << 28) | 1]
        assert got.tobytes() == direct_ref.lights(world_bvh_ref.build(items, spheres, quads, 1, 0, tables=tables())).tobytes()
    finally:
        dev.close()
