"""The path building blocks' C-ABI on the CPU (include/rtx.h, "path building blocks"): the records'
layout against the ctypes and numpy mirrors, and the argument checks, all of which run before any device call."""
import ctypes
import os
import subprocess

import numpy as np

import oracle_binding as ob
import rtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = rtx.RTX_ERR_INVALID_ARG
P = ctypes.c_void_p

FIELDS = {
    "rtx_path_key": (rtx.PathKey, "KEY_DTYPE", 16, ["pixel", "sample", "event", "draws"]),
    "rtx_bounce": (rtx.Bounce, "BOUNCE_DTYPE", 64, ["attenuation", "flags", "emitted", "rng_draws", "ray"]),
    "rtx_shade_stats": (rtx.ShadeStats, None, 48, ["n", "hits", "scattered", "rng_draws", "texel_fetches", "kernel_ms"]),
    "rtx_ray": (rtx.TraceRay, "RAY_DTYPE", 32, ["origin", "tmin", "dir", "tmax"]),
}


def test_record_layout_matches_header(built, tmp_path):
    """sizeof and offsetof of every field as gcc sees the header, against ctypes and the numpy dtypes."""
    lines = []
    for name, (_, _, _, fields) in FIELDS.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));\n')
        lines += [f'printf("%zu\\n", offsetof({name}, {f}));\n' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\nint main(void){\n' + "".join(lines) +
                   'printf("%u %u %u\\n", RTX_BOUNCE_SCATTERED, RTX_BOUNCE_EMITS, RTX_SHADE_COUNTERS);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    nums = iter(int(x) for x in out[:-2])
    for name, (cls, dtype, size, fields) in FIELDS.items():
        assert next(nums) == size == ctypes.sizeof(cls), name
        dt = getattr(rtx, dtype) if dtype else None
        if dt is not None:
            assert dt.itemsize == size and list(dt.names) == fields, name
        for f in fields:
            off = next(nums)
            assert getattr(cls, f).offset == off, (name, f)
            if dt is not None:
                assert dt.fields[f][1] == off, (name, f)
    assert rtx.BOUNCE_DTYPE["ray"] == rtx.RAY_DTYPE
    assert [int(x) for x in out[-2].split()] == [rtx.RTX_BOUNCE_SCATTERED, rtx.RTX_BOUNCE_EMITS, rtx.RTX_SHADE_COUNTERS]


def failed(rc, word=None):
    msg = rtx.load().rtx_last_error()
    return rc == E and len(msg) > 0 and (word is None or word in msg)


def test_version_and_symbols(built):
    L = rtx.load()
    assert L.rtx_version() == 10
    for name in ("rtx_camera_rays_device", "rtx_camera_rays", "rtx_shade_device", "rtx_shade"):
        assert name in rtx.RTX_SYMBOLS and hasattr(L, name)


def test_shade_argument_validation(built):
    L = rtx.load()
    scene = ctypes.create_string_buffer(4096)  # stands for a scene: validation fails before it is looked at
    s = ctypes.cast(scene, P)
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    rays, hits, keys, out = a, a + 512, a + 1024, a + 2048
    st = rtx.ShadeStats()
    for fn, tail in ((L.rtx_shade_device, (None, None)), (L.rtx_shade, (None,)),
                     (L.rtx_shade_device, (None, ctypes.byref(st))), (L.rtx_shade, (ctypes.byref(st),))):
        assert failed(fn(None, 7, rays, hits, keys, 4, out, 0, *tail), b"scene")
        assert failed(fn(None, 7, None, None, None, 0, None, 0, *tail), b"scene")  # (even with nothing to do)
        for k in range(4):  # each pointer NULL, then off a 16-B boundary
            args = [rays, hits, keys, out]
            args[k] = None
            assert failed(fn(s, 7, args[0], args[1], args[2], 4, args[3], 0, *tail), b"NULL"), k
            args = [rays, hits, keys, out]
            args[k] += 4
            assert failed(fn(s, 7, args[0], args[1], args[2], 4, args[3], 0, *tail), b"aligned"), k
        for flags in (2, 4, 1 << 31, 0xFFFFFFFE):
            assert failed(fn(s, 7, rays, hits, keys, 4, out, flags, *tail), b"flags"), flags
        assert failed(fn(s, 7, rays, hits, keys, 0, out, 2, *tail), b"flags")  # unknown bits even with n == 0
        # n == 0 needs no device (and no pointers)
        st.n = st.hits = 99
        assert fn(s, 7, None, None, None, 0, None, 0, *tail) == rtx.RTX_OK
        assert fn(s, 7, rays, hits, keys, 0, out, rtx.RTX_SHADE_COUNTERS, *tail) == rtx.RTX_OK
        assert L.rtx_last_error() == b""
        if tail[-1] is not None:
            assert (st.n, st.hits, st.kernel_ms) == (0, 0, 0.0)  # zeroed


def test_camera_rays_argument_validation(built):
    L = rtx.load()
    cam = ob.rand_spheres_camera(48, 8, 50)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    buf = ctypes.create_string_buffer(4096)
    rays = (ctypes.addressof(buf) + 15) & ~15
    keys = rays + 2048
    c, r = ctypes.byref(cam), ctypes.byref(reg)
    for fn, tail in ((L.rtx_camera_rays_device, (None,)), (L.rtx_camera_rays, ())):
        assert failed(fn(None, 7, r, 0, 1, rays, keys, *tail), b"camera")
        assert failed(fn(c, 7, None, 0, 1, rays, keys, *tail), b"region")
        assert failed(fn(c, 7, r, 0, 1, None, keys, *tail), b"NULL")
        assert failed(fn(c, 7, r, 0, 1, rays + 8, keys, *tail), b"aligned")
        assert failed(fn(c, 7, r, 0, 1, rays, keys + 4, *tail), b"aligned")
        assert failed(fn(c, 7, r, 0, 1, rays + 4, None, *tail), b"aligned")
        # the checks of rtx_render_region_device: the camera, the region inside the image, the shard, the stripe
        assert failed(fn(c, 7, ctypes.byref(rtx.Region(40, 0, 16, 4, 0, 1)), 0, 1, rays, keys, *tail), b"outside")
        assert failed(fn(c, 7, ctypes.byref(rtx.Region(0, 0, 8, 8, 2, 2)), 0, 1, rays, keys, *tail), b"shard")
        assert failed(fn(c, 7, ctypes.byref(rtx.Region(0, 0, 8, 8, 0, 1, 3)), 0, 1, rays, keys, *tail), b"stripe")
        empty = ob.rand_spheres_camera(48, 8, 50)
        empty.image_width = 0
        assert failed(fn(ctypes.byref(empty), 7, r, 0, 1, rays, keys, *tail), b"empty")
        # the sample word is 32-bit: first_sample + count may reach 2^32 - 1 and not pass it
        for first, count in ((0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (0x80000000, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF)):
            assert failed(fn(c, 7, r, first, count, rays, keys, *tail), b"2^32"), (first, count)
        # nothing to do: count == 0 (up to the last sample), a shard without rows, a window without columns
        for first in (0, 5, 0xFFFFFFFF):
            assert fn(c, 7, r, first, 0, rays, keys, *tail) == rtx.RTX_OK
        assert fn(c, 7, r, 0, 0, None, None, *tail) == rtx.RTX_OK
        assert fn(c, 7, ctypes.byref(rtx.Region(0, 0, 8, 2, 3, 4)), 0, 4, rays, keys, *tail) == rtx.RTX_OK
        assert fn(c, 7, ctypes.byref(rtx.Region(3, 3, 0, 5, 0, 1)), 0, 4, rays, keys, *tail) == rtx.RTX_OK
        assert L.rtx_last_error() == b""
    assert (np.frombuffer(buf, np.uint8) == 0).all()  # and nothing was written
