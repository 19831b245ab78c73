"""tests/world_bvh_ref.py (the independent NewBVHFromWorld over spheres and quads) proven on the CPU before a GPU test
relies on it: against the host mirror's trees of the main.go scenes with quads, and on trees worked out by hand.  Then
the host-only parts of the feature: rtx_quad_init and rtx_box_quads against NewQuad written out in numpy
(direct_scenes.quad) and against the mirror's records, the record layouts through the compiler, every refusal of
rtx_scene_create_world (each returns before a device is touched), and the Go file's new call."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import direct_scenes as ds
import rtx
import trace_ref
import world_bvh_ref

F32 = np.float32
NODE, QUAD = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(table, n, per):
    """[n, per] uint32 view of a ctypes record table."""
    if n == 0:
        return np.zeros((0, per), np.uint32)
    return np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint32)), shape=(max(n, 1), per))[:n]


def same_but_for_the_index_word(got, got_s, got_q, want, want_s, want_q):
    """Every word equal except a leaf's index word (a sphere entry's word 5, a quad entry's word 4); through that
    word both entries name the same primitive record (a sphere's 5 data words, a quad's 20)."""
    assert got.shape == want.shape
    tag = want[:, 7].view(np.int32)
    assert np.array_equal(tag, got[:, 7].view(np.int32))
    mask = np.ones(got.shape, bool)
    mask[tag >= 0, 5] = False
    mask[tag == QUAD, 4] = False
    bad = np.nonzero(((got != want) & mask).any(axis=1))[0]
    assert not bad.size, f"{bad.size} entries differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    s, q = np.nonzero(tag >= 0)[0], np.nonzero(tag == QUAD)[0]
    a, b = got_s[got[s, 5]][:, :5], want_s[want[s, 5]][:, :5]
    assert np.array_equal(a, b), "a sphere entry names another sphere"
    a, b = got_q[got[q, 4]], want_q[want[q, 4]]
    assert np.array_equal(a, b), "a quad entry names another quad"


@pytest.mark.parametrize("scene", ["cornell_box", "quad_demo", "simple_light_demo"])
def test_reference_equals_host_mirror(built, scene):
    """The mirror numbers its primitives in walk order, the reference in Add order: the same tree, other labels."""
    host = rtx.HostScene(scene, 1)
    items, spheres, quads, draw0, seed = host.world()
    d = host.desc.contents
    assert len(spheres) == d.n_spheres and len(quads) == d.n_quads and len(items) == d.n_spheres + d.n_quads
    assert seed == 1
    got = trace_ref.entries_of(world_bvh_ref.build(items, spheres, quads, seed, draw0))
    want = trace_ref.entries_of(host.desc)
    same_but_for_the_index_word(got, words(spheres, len(spheres), 8), words(quads, len(quads), 20), want,
                                words(d.spheres, d.n_spheres, 8), words(d.quads, d.n_quads, 20))
    tag = got[:, 7].view(np.int32)
    assert sorted(got[tag >= 0, 5].tolist()) == list(range(len(spheres)))  # every primitive once
    assert sorted(got[tag == QUAD, 4].tolist()) == list(range(len(quads)))
    if scene == "cornell_box":
        assert len(quads) == 18 and len(spheres) == 0
    with pytest.raises(rtx.RtxError):
        rtx.HostScene("nested_worlds", 1).world()  # a World holding Worlds and BVHs


# ---- trees worked out by hand -----------------------------------------------------------------------------------
def f(x):  # the bits of a float32
    return struct.unpack("<I", struct.pack("<f", x))[0]


def node(bmin, esc, bmax):
    return [f(v) for v in bmin] + [esc] + [f(v) for v in bmax] + [NODE & 0xFFFFFFFF]


def sphere_entry(c, r, index, material):
    return [f(v) for v in c] + [f(r), f(r * r), index, 0, material]


def quad_entry(normal, d, index):
    return [f(v) for v in normal] + [f(d), index, 0, 0, QUAD & 0xFFFFFFFF]


def sphere_table(spheres):
    arr = (rtx.Sphere * len(spheres))()
    for s, (c, r, m) in zip(arr, spheres):
        s.center[:], s.radius, s.material = list(c), r, m
    return arr


def quad_table(quads):
    return (rtx.Quad * len(quads))(*[ds.quad(*q) for q in quads])


SPH, QD = rtx.RTX_PRIM_SPHERE, rtx.RTX_PRIM_QUAD
EPS = float(F32(0.0001))
BELOW_ONE = float(F32(1) - F32(0.0001))  # the padded minimum of a quad flat at 1
ABOVE_ONE = float(F32(1) + F32(0.0001))


def test_one_quad_by_hand():
    """A list of one: left == right, the leaf emitted once.  Q (1, 2, 3), u (0, 2, 0), v (0, 0, 4): n = (8, 0, 0),
    normal (1, 0, 0), d 1; the box is flat on x and padded there alone.  The quad is number 3 of its table."""
    quads = quad_table([((9, 9, 9), (1, 0, 0), (0, 1, 0), 0)] * 3 + [((1, 2, 3), (0, 2, 0), (0, 0, 4), 7)])
    desc = world_bvh_ref.build([rtx.ref_prim(QD, 3)], None, quads, 1, 3)
    got = trace_ref.entries_of(desc)
    want = np.array([node((BELOW_ONE, 2, 3), 2, (ABOVE_ONE, 4, 7)), quad_entry((1, 0, 0), 1.0, 3)], np.uint32)
    assert np.array_equal(got, want), (got, want)
    nodes = desc.contents.nodes
    assert desc.contents.n_nodes == 1 and nodes[0].left == nodes[0].right == rtx.ref_prim(QD, 3)


def test_padding_decides_a_pair():
    """A quad flat on x at x = 1 (Q (1, 0, 0), u (0, 1, 0), v (0, 0, 1)) has the padded minimum 1 - 0.0001f; a sphere
    with centre x 1.5 and radius 0.50005 has the minimum 0.99995, between that and 1.  Seed 1, draw0 5 draws x: the
    list (quad, sphere) compares sign(sphere.min - quad.min) > 0 and is swapped: sphere, quad.  With the unpadded
    minimum 1 the pair would stay.  Draw0 3 draws y, minima 0 (quad) and -0.00005: kept."""
    r = float(F32(0.50005))
    smin = float(F32(1.5) + F32(r) * F32(-1))
    assert BELOW_ONE < smin < 1.0
    spheres, quads = sphere_table([((1.5, 0.5, 0.5), r, 4)]), quad_table([((1, 0, 0), (0, 1, 0), (0, 0, 1), 2)])
    items = [rtx.ref_prim(QD, 0), rtx.ref_prim(SPH, 0)]
    lo = float(F32(0.5) + F32(r) * F32(-1))
    hi = float(F32(0.5) + F32(r))
    box = node((BELOW_ONE, lo, lo), 3, (float(F32(1.5) + F32(r)), hi, hi))
    s, q = sphere_entry((1.5, 0.5, 0.5), r, 0, 4), quad_entry((1, 0, 0), 1.0, 0)
    got = trace_ref.entries_of(world_bvh_ref.build(items, spheres, quads, 1, 5))
    assert np.array_equal(got, np.array([box, s, q], np.uint32)), got
    got = trace_ref.entries_of(world_bvh_ref.build(items, spheres, quads, 1, 3))
    assert np.array_equal(got, np.array([box, q, s], np.uint32)), got


def test_add_order_decides_a_tie():
    """A sphere (centre (.5, .5, 0), radius .5: x minimum .5 + -.5 = +0) and a quad (Q 0, u (1, 0, 0), v (0, 1, 0): x
    minimum 0, x extent 1, unpadded) tie on x (seed 1, draw0 5): either Add order is kept.  The quad's z extent is 0:
    padded to +-0.0001f."""
    spheres, quads = sphere_table([((0.5, 0.5, 0), 0.5, 1)]), quad_table([((0, 0, 0), (1, 0, 0), (0, 1, 0), 3)])
    s, q = sphere_entry((0.5, 0.5, 0), 0.5, 0, 1), quad_entry((0, 0, 1), 0.0, 0)
    box = node((0, 0, -0.5), 3, (1, 1, 0.5))
    for items, want in (([rtx.ref_prim(SPH, 0), rtx.ref_prim(QD, 0)], [box, s, q]),
                        ([rtx.ref_prim(QD, 0), rtx.ref_prim(SPH, 0)], [box, q, s])):
        got = trace_ref.entries_of(world_bvh_ref.build(items, spheres, quads, 1, 5))
        assert np.array_equal(got, np.array(want, np.uint32)), (got, want)
    lo, hi = world_bvh_ref.quad_boxes([(0, 0, 0)], [(1, 0, 0)], [(0, 1, 0)])
    assert lo[0].tolist() == [0, 0, -EPS] and hi[0].tolist() == [1, 1, EPS]


def test_quad_box_padding_threshold():
    """max - min < eps pads; eps itself does not.  Q = 0, so the extent is exact."""
    below, above = float(np.nextafter(F32(EPS), F32(0))), float(np.nextafter(F32(EPS), F32(1)))
    for ext, padded in ((0.0, True), (below, True), (EPS, False), (above, False), (-below, True), (-EPS, False)):
        lo, hi = world_bvh_ref.quad_boxes([(0, 0, 0)], [(ext, 1, 0)], [(0, 0, 1)])
        a, b = min(0.0, ext), max(0.0, ext)
        want = (float(F32(a) - F32(EPS)), float(F32(b) + F32(EPS))) if padded else (a, b)
        assert (float(lo[0, 0]), float(hi[0, 0])) == want, ext
    with pytest.raises(ValueError):  # inf - inf in a corner: a NaN bound
        inf = float("inf")
        world_bvh_ref.build([rtx.ref_prim(QD, 0)], None, quad_table([((inf, 0, 0), (-inf, 0, 1), (0, 1, 0), 0)]), 1, 0)
    with pytest.raises(ValueError):
        world_bvh_ref.build([], None, None, 1, 0)
    with pytest.raises(ValueError):
        world_bvh_ref.build([3], None, None, 1, 0)  # a node ref


# ---- the constructors -------------------------------------------------------------------------------------------
def same_quad(got: rtx.Quad, want: rtx.Quad, what):
    a, b = words(ctypes.pointer(got), 1, 20)[0], words(ctypes.pointer(want), 1, 20)[0]
    nan_a, nan_b = np.isnan(a.view(F32)), np.isnan(b.view(F32))
    assert np.array_equal(nan_a, nan_b), (what, a, b)
    assert np.array_equal(a[~nan_a], b[~nan_b]), (what, a, b)


def test_quad_init_is_new_quad(built):
    """rtx_quad_init against NewQuad written out in numpy float32, byte for byte (a NaN by its position): a few
    hundred seeded quads over many magnitudes, axis-aligned ones, degenerate ones (u x v = 0), and the Cornell
    box's, those also against the mirror's records."""
    rng = np.random.default_rng(2024)
    cases = []
    for _ in range(300):
        scale = 10.0 ** rng.uniform(-3, 3, 3)
        cases.append(tuple(rng.normal(size=3) * s for s in scale))
    for _ in range(60):  # axis-aligned, with signed zeros
        a, b = rng.permutation(3)[:2]
        u, v = np.zeros(3), np.zeros(3)
        u[a], v[b] = rng.uniform(-5, 5), rng.uniform(-5, 5)
        cases.append((rng.integers(-9, 9, 3).astype(float), u * rng.choice([1.0, -1.0]), v))
    cases += [((1, 2, 3), (0, 0, 0), (1, 0, 0)), ((1, 2, 3), (1, 2, 3), (2, 4, 6)), ((0, 0, 0), (0, 0, 0), (0, 0, 0)),
              ((1, 1, 1), (1e-30, 0, 0), (0, 1e-30, 0)), ((1, 1, 1), (1e25, 0, 0), (0, 1e25, 0))]
    degenerate = 0
    for k, (Q, u, v) in enumerate(cases):
        got, want = rtx.quad(Q, u, v, k), ds.quad(Q, u, v, k)
        same_quad(got, want, (k, Q, u, v))
        assert got.material == k and got.pad0 == got.pad1 == got.pad2 == 0
        degenerate += bool(np.isnan(np.array(list(got.normal))).any())
    assert degenerate >= 3
    _, _, quads, _, _ = rtx.HostScene("cornell_box", 1).world()
    for i, m in enumerate(quads):
        same_quad(rtx.quad(list(m.q), list(m.u), list(m.v), m.material), m, ("cornell", i))
        same_quad(ds.quad(list(m.q), list(m.u), list(m.v), m.material), m, ("cornell numpy", i))
    with pytest.raises(rtx.RtxError):
        rtx.check(rtx.load().rtx_quad_init(None, None, None, 0, None), "rtx_quad_init")


def test_box_quads_is_box(built):
    """rtx_box_quads against the mirror's Box (hittables.go:200-216) in cornellBox (main.go:222-223): quads 6 .. 17
    of its World, byte for byte, the -0 components of Scale(dz, -1) and Scale(dx, -1) included; corners in either
    order give the same box."""
    _, _, quads, _, _ = rtx.HostScene("cornell_box", 1).world()
    assert len(quads) == 18
    for first, (a, b) in ((6, ((130, 0, 65), (295, 165, 230))), (12, ((265, 0, 295), (430, 330, 460)))):
        material = quads[first].material
        for corners in ((a, b), (b, a), ((a[0], b[1], a[2]), (b[0], a[1], b[2]))):
            got = rtx.box(*corners, material)
            assert words(got, 6, 20).tobytes() == words(quads, 18, 20)[first: first + 6].tobytes(), corners
    side = rtx.box((0, 0, 0), (1, 2, 3), 0)
    assert [np.signbit(x) for x in side[1].u] == [True, True, True] and list(side[1].u) == [0, 0, -3]
    assert [np.signbit(x) for x in side[2].u] == [True, True, True] and list(side[2].u) == [-1, 0, 0]
    with pytest.raises(rtx.RtxError):
        rtx.check(rtx.load().rtx_box_quads(None, None, 0, None), "rtx_box_quads")


def test_symbols_and_layouts(built, tmp_path):
    L = rtx.load()
    for name in ("rtx_scene_create_world", "rtx_quad_init", "rtx_box_quads"):
        assert name in rtx.RTX_SYMBOLS and hasattr(L, name)
    assert "rtxhost_scene_world" in rtx.RTXHOST_SYMBOLS and hasattr(rtx.load_host(), "rtxhost_scene_world")
    assert L.rtx_version() == 10
    fields = ["q", "material", "u", "d", "v", "pad0", "w", "pad1", "normal", "pad2"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtx.h"\nint main(void){\n'
                   'printf("%zu %zu\\n", sizeof(rtx_quad), sizeof(rtx_sphere));\n' +
                   "".join(f'printf("%zu\\n", offsetof(rtx_quad, {n}));\n' for n in fields) +
                   'printf("%d %d\\n", (int)RTX_REF_PRIM(RTX_PRIM_QUAD, 5), (int)RTX_REF_PRIM(RTX_PRIM_SPHERE, 0));\n'
                   "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:2] == [80, 32] == [ctypes.sizeof(rtx.Quad), ctypes.sizeof(rtx.Sphere)]
    assert out[2:12] == [getattr(rtx.Quad, n).offset for n in fields] == [0, 12, 16, 28, 32, 44, 48, 60, 64, 76]
    assert out[12:] == [rtx.ref_prim(rtx.RTX_PRIM_QUAD, 5), rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 0)] == [~(1 << 28 | 5), -1]


# ---- rtx_scene_create_world's refusals --------------------------------------------------------------------------
def test_create_world_refusals(built):
    """Each returns RTX_ERR_INVALID_ARG before a device call (this runs without a GPU) and leaves *out NULL.  The item
    count is checked before any item is read: 2^25 + 1 with an array of one."""
    L = rtx.load()
    spheres = sphere_table([((0, 0, 0), 1.0, 0), ((1, 0, 0), 1.0, 0)])
    quads = quad_table([((0, 0, 0), (1, 0, 0), (0, 1, 0), 0)])
    mats = (rtx.Material * 1)()
    texs = (rtx.Texture * 1)()
    S, Q = (lambda i: rtx.ref_prim(SPH, i)), (lambda i: rtx.ref_prim(QD, i))

    def create(items, n_items, out, sp=spheres, ns=2, qd=quads, nq=1, n_mats=1):
        arr = None if items is None else (ctypes.c_int32 * max(len(items), 1))(*items)
        return L.rtx_scene_create_world(arr, n_items, sp, ns, qd, nq, mats, n_mats, texs, 1, None, 0, 1, 0, out, None)

    assert create([S(0)], 1, None) == rtx.RTX_ERR_INVALID_ARG
    assert b"NULL" in L.rtx_last_error()
    h = ctypes.c_void_p()
    cases = [
        (dict(items=[S(0)], n_items=0), b"empty World"),
        (dict(items=None, n_items=0, ns=0, nq=0), b"empty World"),
        (dict(items=[S(0)], n_items=(1 << 25) + 1), b"too many items"),
        (dict(items=None, n_items=2), b"items is NULL"),                  # 2 spheres + 1 quad are 3
        (dict(items=None, n_items=4), b"items is NULL"),
        (dict(items=[S(0), 0], n_items=2), b"item 1: a node ref"),
        (dict(items=[S(0), 7], n_items=2), b"item 1: a node ref"),
        (dict(items=[rtx.ref_prim(rtx.RTX_PRIM_LIST, 0)], n_items=1), b"item 0: a nested World"),
        (dict(items=[Q(0), rtx.ref_prim(3, 0)], n_items=2), b"item 1: unknown primitive type 3"),
        (dict(items=[rtx.ref_prim(7, 1)], n_items=1), b"item 0: unknown primitive type 7"),
        (dict(items=[S(1), S(2)], n_items=2), b"item 1: sphere ref 2 out of range"),
        (dict(items=[Q(0), Q(1)], n_items=2), b"item 1: quad ref 1 out of range"),
        (dict(items=[S(0)], n_items=1, ns=0), b"item 0: sphere ref 0 out of range"),
        (dict(items=[Q(0)], n_items=1, nq=0), b"item 0: quad ref 0 out of range"),
        # what validate_tables refuses
        (dict(items=[S(0)], n_items=1, sp=None), b"spheres is NULL"),
        (dict(items=[S(0)], n_items=1, qd=None), b"quads is NULL"),
        (dict(items=[S(0)], n_items=1, n_mats=0), b"material 0 out of range"),
    ]
    for kw, word in cases:
        h.value = 0xDEAD
        assert create(out=ctypes.byref(h), **kw) == rtx.RTX_ERR_INVALID_ARG, word
        assert word in L.rtx_last_error(), (word, L.rtx_last_error())
        assert not h.value, word
    bad = sphere_table([((0, 0, 0), 1.0, 0), ((1, 0, 0), 1.0, 1)])  # material 1 of a table of one, named by no item
    h.value = 0xDEAD
    assert create([S(0)], 1, ctypes.byref(h), sp=bad) == rtx.RTX_ERR_INVALID_ARG
    assert b"sphere 1 material 1 out of range" in L.rtx_last_error() and not h.value
    mats[0].type = 9
    h.value = 0xDEAD
    assert create([S(0)], 1, ctypes.byref(h)) == rtx.RTX_ERR_INVALID_ARG
    assert b"material 0: unknown type 9" in L.rtx_last_error() and not h.value


# ---- the Go file ------------------------------------------------------------------------------------------------
GO = open(os.path.join(ROOT, "go", "internal", "render_gpu.go")).read()


def test_go_file_issues_the_world_build():
    """NewBVHFromWorldGPU's World of spheres and quads goes to rtx_scene_create_world with the items in Add order; a
    World of spheres alone keeps rtx_scene_create_spheres; anything else keeps the fallback."""
    assert GO.count("C.rtx_scene_create_world(") == 1 and GO.count("C.rtx_scene_create_spheres(") == 1
    body = GO[GO.index("if g, ok := world.(*gpuBVH); ok {"):GO.index("t, err := flatten(world)")]
    assert "primRef(C.RTX_PRIM_SPHERE, len(t.spheres)-1)" in body and "primRef(C.RTX_PRIM_QUAD, len(t.quads)-1)" in body
    assert "return nil, nil, errFallback" in body
    assert re.search(r"t\.sphereOf = append\(t\.sphereOf, ", body) and re.search(r"t\.quadOf = append\(t\.quadOf, ", body)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell_box", "quad_demo"])
def test_go_sequence_world_bvh(built, scene):
    """renderOnDevices for NewBVHFromWorldGPU(world) with quads: rtx_scene_create_world(items in Add order, spheres,
    quads, materials, textures, texels, seed, draw0 = 0, &scene, NULL) -> rtx_render_ppm -> rtx_scene_destroy.  The
    P3 bytes are those of rtx_scene_create over the independent reference's tree for the same seed and draw
    position."""
    import torch

    from test_go_binding import render_ppm

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    L = rtx.load()
    host = rtx.HostScene(scene, 1)
    items, spheres, quads, _, _ = host.world()
    d = host.desc.contents
    cam = host.camera(width=48, spp=2)
    h = ctypes.c_void_p()
    rtx.check(L.rtx_scene_create_world(items, len(items), spheres if len(spheres) else None, len(spheres), quads,
                                       len(quads), d.materials, d.n_materials, d.textures, d.n_textures, d.texels,
                                       d.n_texels, 2024, 0, ctypes.byref(h), None), "rtx_scene_create_world")
    dev = rtx.DeviceScene(handle=h)
    ref = rtx.DeviceScene(world_bvh_ref.build(items, spheres, quads, 2024, 0, tables=host.desc))
    try:
        assert dev.export() == ref.export()
        text = render_ppm(L, h, cam, 2024)
        assert text == render_ppm(L, ref.handle, cam, 2024) and text.startswith(b"P3\n48 ")
    finally:
        dev.close()
        ref.close()
