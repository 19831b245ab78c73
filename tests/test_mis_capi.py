"""Multiple importance sampling of the direct light on the CPU (rtx_prim_lights, rtx_emitter_weight*, rtx_accum_add_mis;
DESIGN.md §42): the record's layout, the checks every entry makes before it touches a device, the per-primitive
lookup against the emitter table, and the yardstick that needs no GPU: a float64 Monte Carlo of the contract's
estimator against the closed-form form factors."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import direct_ref
import direct_scenes as ds
import mis_ref
import rtx

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtx_prim_lights", "rtx_emitter_weight_device", "rtx_emitter_weight", "rtx_accum_add_mis")


def test_symbols_and_layouts(built, tmp_path):
    L = rtx.load()
    for name in NAMES:
        assert name in rtx.RTX_SYMBOLS and hasattr(L, name)
    structs = {"rtx_prim_light": (rtx.PrimLight, rtx.PRIM_LIGHT_DTYPE, 8),
               "rtx_emitter_weight_record": (rtx.EmitterWeight, rtx.EMITTER_WEIGHT_DTYPE, 16),
               "rtx_emitter_stats": (rtx.EmitterStats, None, 24)}
    fields = ("weight", "geom", "light", "flags")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtx.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in structs) +
                   "".join(f'printf("%zu\\n", offsetof(rtx_emitter_weight_record, {f}));\n' for f in fields) +
                   'printf("%zu %zu\\n", offsetof(rtx_prim_light, area), offsetof(rtx_prim_light, light));\n'
                   'printf("%u %u %u %d\\n", RTX_LIGHT_NONE, RTX_EMITTER_WEIGHTED, RTX_EMITTER_COUNTERS, RTX_ABI_VERSION);\n'
                   'return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    for (name, (cls, dt, size)), got in zip(structs.items(), out):
        assert int(got) == size == ctypes.sizeof(cls), name
        assert dt is None or dt.itemsize == size, name
    assert [int(x) for x in out[3:7]] == [0, 4, 8, 12]
    assert [rtx.EMITTER_WEIGHT_DTYPE.fields[f][1] for f in fields] == [0, 4, 8, 12]
    assert [getattr(rtx.EmitterWeight, f).offset for f in fields] == [0, 4, 8, 12]
    assert [int(x) for x in out[7:9]] == [0, 4] == [rtx.PRIM_LIGHT_DTYPE.fields[f][1] for f in ("area", "light")]
    assert [int(x) for x in out[9:]] == [rtx.RTX_LIGHT_NONE, rtx.RTX_EMITTER_WEIGHTED, rtx.RTX_EMITTER_COUNTERS, 10]
    assert L.rtx_version() == 10


# ---- argument checks (all before a device is touched) ----------------------------------------------------------
def test_emitter_weight_arguments(built):
    """NULL scene, unknown flags, n == 0, NULL and misaligned pointers (the scene handle below is never dereferenced:
    the checks that run before the lock reject the call)."""
    L = rtx.load()
    st = rtx.EmitterStats()
    buf = np.zeros(256, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    entries = ((L.rtx_emitter_weight_device, (None, None)), (L.rtx_emitter_weight, (None,)))
    for fn, tail in entries + ((L.rtx_emitter_weight_device, (None, ctypes.byref(st))),
                               (L.rtx_emitter_weight, (ctypes.byref(st),))):
        assert fn(None, a, a, 1, a, 0, *tail) == rtx.RTX_ERR_INVALID_ARG
        assert "NULL scene" in L.rtx_last_error().decode()
    fake = ctypes.c_void_p(a)  # a non-NULL "scene": every call below must fail before it is looked at
    for fn, tail in entries:
        assert fn(fake, a, a, 1, a, 2, *tail) == rtx.RTX_ERR_INVALID_ARG
        assert "flags" in L.rtx_last_error().decode()
        assert fn(fake, None, None, 0, None, 0, *tail) == rtx.RTX_OK  # n == 0: nothing to do, nothing read
        for args in ((None, a, a), (a, None, a), (a, a, None)):
            assert fn(fake, args[0], args[1], 1, args[2], 0, *tail) == rtx.RTX_ERR_INVALID_ARG
            assert "NULL" in L.rtx_last_error().decode()
        for args in ((a + 4, a, a), (a, a + 8, a), (a, a, a + 4)):
            assert fn(fake, args[0], args[1], 1, args[2], 0, *tail) == rtx.RTX_ERR_INVALID_ARG
            assert "aligned" in L.rtx_last_error().decode()
    for fn, tail in ((L.rtx_emitter_weight_device, (None, ctypes.byref(st))), (L.rtx_emitter_weight, (ctypes.byref(st),))):
        st.n = st.weighted = 7
        assert fn(fake, None, None, 0, None, rtx.RTX_EMITTER_COUNTERS, *tail) == rtx.RTX_OK
        assert (st.n, st.weighted) == (0, 0)  # n == 0 zeroes the stats


def test_add_mis_arguments(built):
    """The checks of rtx_accum_add_mis that need no accumulator's state: a NULL accumulator and a pass of 0 samples
    (the others need a live accumulator: tests/test_mis_gpu.py::test_accumulator_modes)."""
    L = rtx.load()
    st = rtx.Stats()
    for stats in (None, ctypes.byref(st)):
        assert L.rtx_accum_add_mis(None, 1, None, 0, stats) == rtx.RTX_ERR_INVALID_ARG
        assert "NULL accumulator" in L.rtx_last_error().decode()
    buf = np.zeros(256, np.uint8)
    assert L.rtx_accum_add_mis(ctypes.c_void_p(buf.ctypes.data), 0, None, 0, None) == rtx.RTX_ERR_INVALID_ARG
    assert "0 samples" in L.rtx_last_error().decode()


def test_prim_lights_arguments(built):
    L = rtx.load()
    ns, n = ctypes.c_uint32(), ctypes.c_uint32()
    host = rtx.HostScene("cornell_box", 1)
    assert L.rtx_prim_lights(None, None, 0, ctypes.byref(ns), ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    assert L.rtx_prim_lights(host.desc, None, 0, None, ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    assert L.rtx_prim_lights(host.desc, None, 0, ctypes.byref(ns), None) == rtx.RTX_ERR_INVALID_ARG
    bad = ds.world([ds.sphere((0, 0, 0), 1, 3)], [], [ds.material(ds.LIGHT, 0)], [ds.solid(1, 1, 1)])
    assert L.rtx_prim_lights(bad, None, 0, ctypes.byref(ns), ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    small = (rtx.PrimLight * 1)()
    assert L.rtx_prim_lights(host.desc, small, 1, ctypes.byref(ns), ctypes.byref(n)) == rtx.RTX_OK
    assert n.value == host.desc.contents.n_spheres + host.desc.contents.n_quads > 1
    assert small[0].area == 0.0 and small[0].light == 0  # too small a buffer is left alone


# ---- the per-primitive lookup ------------------------------------------------------------------------------------
def hand_scene():
    """Emitters the table excludes (a sphere of negative radius, one of radius 0, a quad of area 0, primitives never
    referenced) beside valid ones, and a quad and a sphere referenced twice."""
    texs = [ds.solid(0.5, 0.5, 0.5), ds.solid(3, 3, 3)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1)]
    spheres = [ds.sphere((0, -100, 0), 99, 0),   # 0: not a light
               ds.sphere((3, 1, 0), -0.5, 1),    # 1: negative radius
               ds.sphere((0, 1, 0), 0.5, 1),     # 2: a light, referenced twice
               ds.sphere((6, 1, 0), 0.5, 1),     # 3: never referenced
               ds.sphere((9, 1, 0), 0.0, 1),     # 4: radius 0
               ds.sphere((12, 1, 0), 0.25, 1)]   # 5: a light
    quads = [ds.quad((0, 5, 0), (1, 0, 0), (2, 0, 0), 1),    # 0: u parallel to v: area 0
             ds.quad((0, 4, 0), (1, 0, 0), (0, 0, 1), 1),    # 1: a light, referenced twice
             ds.quad((0, 6, 0), (1, 0, 0), (0, 0, 1), 1),    # 2: never referenced
             ds.quad((0, 0, 0), (1, 0, 0), (0, 0, 1), 0),    # 3: not a light
             ds.quad((0, 8, 0), (2, 0, 0), (0, 0, 3), 1)]    # 4: a light
    roots = [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in (5, 0, 2, 1, 4, 2)] + \
            [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in (4, 1, 0, 3, 1)]
    return ds.world(spheres, quads, mats, texs, roots=roots)


def check_lookup(desc):
    tab, ns = rtx.prim_lights(desc)
    want, want_ns = mis_ref.prim_lights(desc)
    assert ns == want_ns == desc.contents.n_spheres and tab.tobytes() == want.tobytes()
    lights = rtx.lights(desc)
    listed = tab["light"] != rtx.RTX_LIGHT_NONE
    # each emitter of the table exactly once, at its own primitive, with the table's area bit for bit
    assert sorted(tab["light"][listed]) == list(range(len(lights)))
    for k in np.nonzero(listed)[0]:
        prim = (rtx.RTX_PRIM_SPHERE << 28) | int(k) if k < ns else (rtx.RTX_PRIM_QUAD << 28) | int(k - ns)
        j = int(tab["light"][k])
        assert lights["prim"][j] == prim and lights["area"][j].tobytes() == tab["area"][k].tobytes()
    assert not tab["area"][~listed].view(np.uint32).any()
    return tab, ns


def test_lookup_of_the_reference_scenes(built):
    for name, kind in (("cornell_box", rtx.RTX_PRIM_QUAD), ("simple_light_demo", rtx.RTX_PRIM_SPHERE)):
        host = rtx.HostScene(name, 1)
        tab, ns = check_lookup(host.desc)
        k = int(np.nonzero(tab["light"] == 0)[0][0])
        assert (tab["light"] != rtx.RTX_LIGHT_NONE).sum() == 1 and (k >= ns) == (kind == rtx.RTX_PRIM_QUAD)
    tab, _ = rtx.prim_lights(rtx.HostScene("cornell_box", 1).desc)
    assert tab["area"].max() == F32(13650.0)
    tab, ns = rtx.prim_lights(rtx.HostScene("random_spheres", 1).desc)
    assert len(tab) == ns > 0 and (tab["light"] == rtx.RTX_LIGHT_NONE).all()


def test_lookup_of_the_hand_scene(built):
    tab, ns = check_lookup(hand_scene())
    assert ns == 6 and len(tab) == 11
    assert list(tab["light"]) == [rtx.RTX_LIGHT_NONE] * 2 + [0] + [rtx.RTX_LIGHT_NONE] * 2 + [1] + \
        [rtx.RTX_LIGHT_NONE, 2, rtx.RTX_LIGHT_NONE, rtx.RTX_LIGHT_NONE, 3]
    assert tab["area"][7] == F32(1.0) and tab["area"][10] == F32(6.0)
    assert tab["area"][2] == (F32(4) * F32(math.pi)) * (F32(0.5) * F32(0.5))


def test_reference_weights():
    """mis_ref on values worked by hand: wl + wb = 1 up to rounding, wl(0) = 1, wb of an infinite g * g is 1."""
    g = np.array([0.0, 1.0, 3.0, 1e30], F32)
    with np.errstate(over="ignore"):
        w = mis_ref.wl(g)
    assert list(w) == [1.0, 0.5, F32(1) / F32(10), 0.0]
    assert list(F32(1) - w) == [0.0, 0.5, F32(1) - F32(1) / F32(10), 1.0]


# ---- the yardstick: the contract's estimator is unbiased ---------------------------------------------------------
POINTS = ((0.0, 0.0), (0.3, -0.2), (-math.tan(math.radians(20)), math.tan(math.radians(20))), (0.9, 0.1))


def g_bound(light, x, z):
    """An upper bound from the geometry of g over the light's points, from the floor point (x, 0, z), one light
    (L = 1): direct_scenes.g_max's, for a point."""
    if light[0] == "quad":
        _, a0, a1, b0, b1, h = light
        rho2 = max(0.0, a0 - x, x - a1) ** 2 + max(0.0, b0 - z, z - b1) ** 2
        return h * h * (a1 - a0) * (b1 - b0) / (math.pi * (h * h + rho2) ** 2)
    _, c, r = light
    D = math.sqrt((c[0] - x) ** 2 + c[1] ** 2 + (c[2] - z) ** 2)
    return 4 * math.pi * r * r / (math.pi * (D - r) ** 2)


def mis_samples(light, x, z, n, rng):
    """n samples, in units of a * Le, of the depth-2 estimator at the floor point p = (x, 0, z) with normal +y under
    one light: a uniform area sample weighted g / (1 + g^2) when the light's point faces p, plus a cosine-distributed
    bounce weighted g^2 / (1 + g^2) at the emitter point it finds.  float64."""
    p = np.array([x, 0.0, z])
    if light[0] == "quad":
        _, a0, a1, b0, b1, h = light
        area = (a1 - a0) * (b1 - b0)
        q = np.stack([a0 + (a1 - a0) * rng.random(n), np.full(n, h), b0 + (b1 - b0) * rng.random(n)], axis=1)
        nl = np.broadcast_to(np.array([0.0, -1.0, 0.0]), q.shape)
    else:
        _, c, r = light
        area = 4 * math.pi * r * r
        v = rng.normal(size=(n, 3))
        nl = v / np.linalg.norm(v, axis=1, keepdims=True)
        q = np.array(c) + r * nl

    def geom(q, nl):
        w = q - p
        d2 = np.sum(w * w, axis=1)
        dist = np.sqrt(d2)
        cs, facing = w[:, 1] / dist, np.sum(nl * w, axis=1) / dist
        return cs * np.abs(facing) * area / (math.pi * d2), cs, facing

    g, cs, facing = geom(q, nl)
    # the shadow ray: nothing lies between the floor and a quad; a sphere's far side is hidden by its near side
    seen = (cs > 0) & (facing < 0 if light[0] == "sphere" else facing != 0)
    total = np.where(seen, g / (1 + g * g), 0.0)

    u1, u2 = rng.random(n), rng.random(n)  # the bounce: cosine-distributed about +y
    rad, phi = np.sqrt(u1), 2 * math.pi * u2
    d = np.stack([rad * np.cos(phi), np.sqrt(1 - u1), rad * np.sin(phi)], axis=1)
    if light[0] == "quad":
        t = h / d[:, 1]
        hq = p + d * t[:, None]
        found = (d[:, 1] > 0) & (hq[:, 0] >= a0) & (hq[:, 0] <= a1) & (hq[:, 2] >= b0) & (hq[:, 2] <= b1)
        hn = np.broadcast_to(np.array([0.0, -1.0, 0.0]), hq.shape)
    else:
        oc = p - np.array(c)
        bq = np.sum(oc * d, axis=1)
        disc = bq * bq - (np.sum(oc * oc) - r * r)
        found = disc > 0
        t = -bq - np.sqrt(np.where(found, disc, 0.0))
        found &= t > 0
        hq = p + d * t[:, None]
        hn = (hq - np.array(c)) / r
    gb, _, _ = geom(np.where(found[:, None], hq, q), np.where(found[:, None], hn, nl))
    return total + np.where(found, gb * gb / (1 + gb * gb), 0.0)


@pytest.mark.parametrize("kind", ["a", "c"])
def test_estimator_is_unbiased(kind):
    """The contract's estimator, stated here independently of the device code, against direct_scenes.form_factor at
    four fixed floor points.  A sample lies in [0, M] (units of a * Le) with M = (g_max <= 1 ? g_max / (1 + g_max^2) :
    1/2) + g_max^2 / (1 + g_max^2), so its variance is at most F (M - F) (Bhatia-Davis); N is the least power of two
    for which 6 sigma / sqrt(N) is at most 3 % of F, and the mean is held within 6 sigma / sqrt(N)."""
    _, _, lights = ds.floor_scene(kind)
    assert len(lights) == 1
    rng = np.random.default_rng(20240 + ord(kind))
    for x, z in POINTS:
        F = float(ds.form_factor(lights[0], x, z))
        gm = g_bound(lights[0], x, z)
        M = (gm / (1 + gm * gm) if gm <= 1 else 0.5) + gm * gm / (1 + gm * gm)
        var = F * (M - F)
        assert var > 0
        N = 1 << math.ceil(math.log2(var * (6 / (0.03 * F)) ** 2))
        assert N <= 1 << 22, N
        s = mis_samples(lights[0], x, z, N, rng)
        assert s.min() >= 0 and s.max() <= M * (1 + 1e-12), (s.max(), M)
        tol = 6 * math.sqrt(var / N)
        print(f"{kind} ({x:.3f}, {z:.3f}): F {F:.5f}, g_max {gm:.4f}, M {M:.4f}, N {N}, mean / F {s.mean() / F:.5f}, "
              f"bound {tol / F:.4f}")
        assert abs(s.mean() - F) <= tol, (kind, x, z, s.mean(), F, tol)
