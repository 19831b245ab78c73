"""Direct light sampling on the CPU (rtx_lights*, rtx_direct*): the emitter table (host only), the
checks every entry makes before it touches a device, the records' layouts, and the yardstick the GPU tests hold the
estimator to: the closed-form pixel values of the analytic scenes agree with a float64 quadrature over the light and
with the oracle's plain render."""
import ctypes
import os
import math

import numpy as np
import pytest

import direct_ref
import direct_scenes as ds
import oracle_binding as ob
import rtx

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtx_lights", "rtx_scene_lights", "rtx_direct_device", "rtx_direct", "rtx_accum_add_direct")


def test_symbols_and_layouts(built, tmp_path):
    import subprocess

    L = rtx.load()
    for name in NAMES:
        assert name in rtx.RTX_SYMBOLS and hasattr(L, name)
    structs = {"rtx_light": (rtx.Light, rtx.LIGHT_DTYPE, 8), "rtx_direct_sample": (rtx.DirectSample, rtx.DIRECT_DTYPE, 64),
               "rtx_direct_stats": (rtx.DirectStats, None, 40)}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtx.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", sizeof({n}));\n' for n in structs) +
                   'printf("%zu %zu %zu %zu\\n", offsetof(rtx_direct_sample, flags), offsetof(rtx_direct_sample, ray), '
                   'offsetof(rtx_direct_sample, light), offsetof(rtx_direct_sample, geom));\nreturn 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    for (name, (cls, dt, size)), got in zip(structs.items(), out):
        assert int(got) == size == ctypes.sizeof(cls), name
        assert dt is None or dt.itemsize == size, name
    assert [int(x) for x in out[3:]] == [12, 16, 48, 56]
    d = rtx.DIRECT_DTYPE
    assert [d.fields[f][1] for f in ("flags", "ray", "light", "rng_draws", "geom", "reserved")] == [12, 16, 48, 52, 56, 60]
    assert (rtx.RTX_DIRECT_SAMPLED, rtx.RTX_DIRECT_VISIBLE, rtx.RTX_DIRECT_COUNTERS) == (1, 2, 1)
    assert L.rtx_version() == 10


# ---- emitter tables -------------------------------------------------------------------------------------------
def test_cornell_box_has_one_quad_light_of_area_13650(built):
    host = rtx.HostScene("cornell_box", 1)
    tab = rtx.lights(host.desc)
    assert len(tab) == 1 and tab["prim"][0] >> 28 == rtx.RTX_PRIM_QUAD
    assert tab["area"][0] == F32(13650.0)  # 130 x 105 (main.go's light quad), exact in float32
    q = host.desc.contents.quads[int(tab["prim"][0] & 0x0FFFFFFF)]
    assert host.desc.contents.materials[q.material].type == rtx.RTX_MAT_DIFFUSE_LIGHT
    assert tab.tobytes() == direct_ref.lights(host.desc).tobytes()


def test_simple_light_demo_has_its_sphere_light(built):
    """main.go's simpleLightDemo holds ONE emitter, the sphere of radius 2 (it has no quad light): area (4 pi) 4."""
    host = rtx.HostScene("simple_light_demo", 1)
    tab = rtx.lights(host.desc)
    assert len(tab) == 1 and tab["prim"][0] >> 28 == rtx.RTX_PRIM_SPHERE
    s = host.desc.contents.spheres[int(tab["prim"][0] & 0x0FFFFFFF)]
    assert list(s.center) == [0.0, 7.0, 0.0] and s.radius == 2.0
    assert tab["area"][0] == (F32(4) * F32(math.pi)) * F32(4)
    assert tab.tobytes() == direct_ref.lights(host.desc).tobytes()


def test_random_spheres_has_no_emitter(built):
    host = rtx.HostScene("random_spheres", 1)
    assert len(rtx.lights(host.desc)) == 0 and len(direct_ref.lights(host.desc)) == 0


def test_spheres_come_before_quads(built):
    """Table order: spheres in sphere-table order, then quads in quad-table order, whatever the roots' order."""
    desc, _ = ds.five()
    tab = rtx.lights(desc)
    assert list(tab["prim"]) == [(rtx.RTX_PRIM_SPHERE << 28) | 0, (rtx.RTX_PRIM_QUAD << 28) | 1]
    assert tab["area"][0] == (F32(4) * F32(math.pi)) * (F32(0.5) * F32(0.5)) and tab["area"][1] == F32(4.0)
    d = desc.contents
    back = ds.world([d.spheres[i] for i in range(2)], [d.quads[i] for i in range(3)],
                    [d.materials[i] for i in range(d.n_materials)], [d.textures[i] for i in range(d.n_textures)],
                    roots=[d.roots[i] for i in reversed(range(d.n_roots))])
    assert rtx.lights(back).tobytes() == tab.tobytes() == direct_ref.lights(desc).tobytes()


def exclusion_scene():
    texs = [ds.solid(0.5, 0.5, 0.5), ds.solid(3, 3, 3)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1)]
    spheres = [ds.sphere((0, 1, 0), 0.5, 1),      # 0: a light
               ds.sphere((3, 1, 0), -0.5, 1),     # 1: negative radius
               ds.sphere((6, 1, 0), 0.5, 1),      # 2: never referenced
               ds.sphere((9, 1, 0), 0.0, 1),      # 3: radius 0
               ds.sphere((0, -100, 0), 99, 0)]    # 4: not a light
    quads = [ds.quad((0, 4, 0), (1, 0, 0), (0, 0, 1), 1),    # 0: a light
             ds.quad((0, 5, 0), (1, 0, 0), (2, 0, 0), 1),    # 1: u parallel to v: area 0
             ds.quad((0, 6, 0), (1, 0, 0), (0, 0, 1), 1),    # 2: never referenced
             ds.quad((0, 7, 0), (np.inf, 0, 0), (0, 0, 1), 1)]  # 3: area not finite
    roots = [rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i) for i in (4, 3, 1, 0)] + \
            [rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in (3, 1, 0, 0)]  # (quad 0 twice: it is one emitter)
    return ds.world(spheres, quads, mats, texs, roots=roots)


def test_exclusions(built):
    desc = exclusion_scene()
    tab = rtx.lights(desc)
    assert list(tab["prim"]) == [(rtx.RTX_PRIM_SPHERE << 28) | 0, (rtx.RTX_PRIM_QUAD << 28) | 0]
    assert tab["area"][1] == F32(1.0)
    assert tab.tobytes() == direct_ref.lights(desc).tobytes()


def test_lights_through_nodes_and_lists(built):
    """An emitter is found under a BVH node and in a nested World; the count query needs no buffer."""
    texs, mats = [ds.solid(1, 1, 1)], [ds.material(ds.LIGHT, 0)]
    spheres = [ds.sphere((0, 0, 0), 1, 0), ds.sphere((5, 0, 0), 2, 0), ds.sphere((9, 0, 0), 1, 0)]
    node = rtx.BvhNode()
    node.bmin[:], node.bmax[:] = [-1, -2, -2], [7, 2, 2]
    node.left, node.right = rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 1), rtx.ref_prim(rtx.RTX_PRIM_LIST, 0)
    desc = ds.world(spheres, [], mats, texs, roots=[0])
    d = desc.contents
    keep = ((rtx.BvhNode * 1)(node), (rtx.List * 1)(rtx.List(0, 1)),
            (ctypes.c_int32 * 1)(rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 0)))
    d.nodes, d.n_nodes, d.lists, d.n_lists, d.list_refs, d.n_list_refs = keep[0], 1, keep[1], 1, keep[2], 1
    tab = rtx.lights(desc)
    assert list(tab["prim"] & 0x0FFFFFFF) == [0, 1]  # sphere 2 is not referenced
    assert tab.tobytes() == direct_ref.lights(desc).tobytes()
    n = ctypes.c_uint32(99)
    small = (rtx.Light * 1)()
    assert rtx.load().rtx_lights(desc, small, 1, ctypes.byref(n)) == rtx.RTX_OK and n.value == 2
    assert small[0].prim == 0 and small[0].area == 0.0  # too small a buffer is left alone


# ---- argument checks (all before a device is touched) ----------------------------------------------------------
def test_light_table_arguments(built):
    L = rtx.load()
    n = ctypes.c_uint32()
    host = rtx.HostScene("cornell_box", 1)
    assert L.rtx_lights(None, None, 0, ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    assert L.rtx_lights(host.desc, None, 0, None) == rtx.RTX_ERR_INVALID_ARG
    assert L.rtx_scene_lights(None, None, 0, ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    bad = ds.world([ds.sphere((0, 0, 0), 1, 3)], [], [ds.material(ds.LIGHT, 0)], [ds.solid(1, 1, 1)])
    assert L.rtx_lights(bad, None, 0, ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG
    assert "material" in L.rtx_last_error().decode()
    empty = ds.world([ds.sphere((0, 0, 0), 1, 0)], [], [ds.material(ds.LIGHT, 0)], [ds.solid(1, 1, 1)], roots=[])
    assert L.rtx_lights(empty, None, 0, ctypes.byref(n)) == rtx.RTX_ERR_INVALID_ARG


def test_direct_arguments(built):
    """NULL scene, unknown flags, n == 0, NULL and misaligned pointers: rtx_shade's checks, none of which needs a
    device (the scene handle below is never dereferenced: the checks that run before the lock reject the call)."""
    L = rtx.load()
    st = rtx.DirectStats()
    buf = np.zeros(256, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    for fn, tail in ((L.rtx_direct_device, (None, None)), (L.rtx_direct, (None,)),
                     (L.rtx_direct_device, (None, ctypes.byref(st))), (L.rtx_direct, (ctypes.byref(st),))):
        assert fn(None, 1, a, a, 1, a, 0, *tail) == rtx.RTX_ERR_INVALID_ARG
        assert "NULL scene" in L.rtx_last_error().decode()
    fake = ctypes.c_void_p(a)  # a non-NULL "scene": every call below must fail before it is looked at
    for fn, tail in ((L.rtx_direct_device, (None, None)), (L.rtx_direct, (None,))):
        assert fn(fake, 1, a, a, 1, a, 2, *tail) == rtx.RTX_ERR_INVALID_ARG
        assert "flags" in L.rtx_last_error().decode()
        assert fn(fake, 1, None, None, 0, None, 0, *tail) == rtx.RTX_OK  # n == 0: nothing to do, nothing read
        for args in ((None, a, a), (a, None, a), (a, a, None)):
            assert fn(fake, 1, args[0], args[1], 1, args[2], 0, *tail) == rtx.RTX_ERR_INVALID_ARG
            assert "NULL" in L.rtx_last_error().decode()
        for args in ((a + 4, a, a), (a, a + 8, a), (a, a, a + 4)):
            assert fn(fake, 1, args[0], args[1], 1, args[2], 0, *tail) == rtx.RTX_ERR_INVALID_ARG
            assert "aligned" in L.rtx_last_error().decode()
    st.n = 7
    assert L.rtx_direct(fake, 1, None, None, 0, None, rtx.RTX_DIRECT_COUNTERS, ctypes.byref(st)) == rtx.RTX_OK
    assert st.n == 0  # n == 0 zeroes the stats


def test_add_direct_arguments(built):
    """The checks of rtx_accum_add_direct that need no accumulator's state: a NULL accumulator and a pass of 0 samples
    (checked before the accumulator is read).  The others (flags, the three modes) need a live accumulator and so a
    device: tests/test_direct_gpu.py::test_accumulator_modes; each returns before a device is touched."""
    L = rtx.load()
    st = rtx.Stats()
    for stats in (None, ctypes.byref(st)):
        assert L.rtx_accum_add_direct(None, 1, None, 0, stats) == rtx.RTX_ERR_INVALID_ARG
        assert "NULL accumulator" in L.rtx_last_error().decode()
    buf = np.zeros(64, np.uint8)
    assert L.rtx_accum_add_direct(ctypes.c_void_p(buf.ctypes.data), 0, None, 0, None) == rtx.RTX_ERR_INVALID_ARG
    assert "0 samples" in L.rtx_last_error().decode()


# ---- the yardstick, on the code as it stands --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_closed_forms_agree_with_quadrature(kind):
    """The form factors the GPU tests expect, against a float64 midpoint rule over the light's surface: 400 x 400
    cells (400 x 800 on the sphere), whose error on these smooth integrands is far below the 1e-4 relative asked."""
    _, cam, lights = ds.floor_scene(kind)
    x0, x1, z0, z1 = ds.footprints(cam)
    assert abs(x0.min() + math.tan(math.radians(20))) < 1e-5 and abs(z1.max() - math.tan(math.radians(20))) < 1e-5
    for x, z in ((0.0, 0.0), (0.3, -0.2), (x0.min(), z1.max()), (0.9, 0.1)):
        for l in lights:
            f, q = float(ds.form_factor(l, x, z)), ds.quadrature(l, x, z)
            assert abs(f - q) <= 1e-4 * q, (kind, l, x, z, f, q)


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_closed_forms_agree_with_the_oracle(built, kind):
    """The oracle's plain render of the analytic scenes (depth 2: a sample is a * Le when the bounce reaches a light,
    else 0) against a * Le * F.  With p = the image's mean F, a sample's variance is at most (a Le)^2 p (1 - p) <=
    (a Le)^2 p, so the image mean over P pixels x N samples has sigma <= a Le sqrt(p / (P N)); N is the least power of
    two with 6 sigma <= 3 % of a Le p."""
    desc, cam, lights = ds.floor_scene(kind)
    want, f = ds.expected_image(cam, lights)
    P, p = f.size, float(f.mean())
    need = (6 / 0.03) ** 2 / (P * p)
    cam.samples_per_pixel = 1 << math.ceil(math.log2(need))
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    img, _ = ob.render(desc, cam, 20241, reg, ob.ORDER_ITERATIVE)
    got, exp = img.astype(np.float64).mean(axis=(0, 1)), want.mean(axis=(0, 1))
    print(f"{kind}: spp {cam.samples_per_pixel}, mean F {p:.5f}, oracle / closed form {got / exp}")
    assert np.all(np.abs(got - exp) <= 0.03 * exp), (got, exp)
