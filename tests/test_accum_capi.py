"""The accumulator's C-ABI on the CPU (include/rtx.h, "progressive rendering"): argument validation, which runs
before any device call, and the test reference itself (accum_ref.py) held to the oracle's one-shot render."""
import ctypes

import numpy as np
import pytest

import accum_ref
import oracle_binding as ob
import rtx


def test_accum_argument_validation(built):
    L = rtx.load()
    E = rtx.RTX_ERR_INVALID_ARG
    scene = ctypes.create_string_buffer(4096)  # stands for a scene: validation fails before it is looked at
    s = ctypes.cast(scene, ctypes.c_void_p)
    cam = ob.rand_spheres_camera(48, 8, 50)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    h = ctypes.c_void_p()
    assert L.rtx_accum_create(None, ctypes.byref(cam), 7, ctypes.byref(reg), ctypes.byref(h)) == E
    assert L.rtx_accum_create(s, None, 7, ctypes.byref(reg), ctypes.byref(h)) == E
    assert b"camera" in L.rtx_last_error()
    assert L.rtx_accum_create(s, ctypes.byref(cam), 7, None, ctypes.byref(h)) == E
    assert b"region" in L.rtx_last_error()
    assert L.rtx_accum_create(s, ctypes.byref(cam), 7, ctypes.byref(reg), None) == E
    # the checks of rtx_render_region_device: the camera, the region inside the image, the shard
    bad = rtx.Region(40, 0, 16, 4, 0, 1)
    assert L.rtx_accum_create(s, ctypes.byref(cam), 7, ctypes.byref(bad), ctypes.byref(h)) == E
    assert b"outside" in L.rtx_last_error()
    bad = rtx.Region(0, 0, 8, 8, 2, 2)
    assert L.rtx_accum_create(s, ctypes.byref(cam), 7, ctypes.byref(bad), ctypes.byref(h)) == E
    empty = ob.rand_spheres_camera(48, 8, 50)
    empty.image_width = 0
    assert L.rtx_accum_create(s, ctypes.byref(empty), 7, ctypes.byref(reg), ctypes.byref(h)) == E
    assert not h.value
    # a NULL accumulator to every entry
    st = rtx.Stats()
    n = ctypes.c_uint64()
    buf = ctypes.create_string_buffer(64)
    assert L.rtx_accum_add(None, 4, None, 0, None) == E
    assert L.rtx_accum_add(None, 0, None, 0, ctypes.byref(st)) == E  # count == 0
    assert L.rtx_accum_samples(None) == 0
    assert L.rtx_accum_resolve_device(None, None, None, 0.1, None, None) == E
    assert L.rtx_accum_resolve(None, buf, None, 0.1, ctypes.byref(n)) == E
    assert L.rtx_accum_ppm(None, buf, 64, ctypes.byref(n)) == E
    assert L.rtx_accum_reset(None) == E
    assert b"accumulator" in L.rtx_last_error()
    L.rtx_accum_destroy(None)  # no-op


@pytest.mark.parametrize("width,spp,seed,region", [(48, 8, 7, None), (64, 7, 9, (5, 3, 17, 5))])
def test_reference_fold_equals_the_oracle_render(built, width, spp, seed, region):
    """The reference's S / n is the oracle's iterative render bit for bit, and at rel_tol = 0.1 some pixels, not all,
    are noisy: the count the GPU tests compare is neither trivial value."""
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=width, spp=spp, depth=50)
    reg = rtx.Region(*region, 0, 1) if region else rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    col = accum_ref.sample_colours(("random_spheres", 1, width, 50), scene.desc, cam, seed, reg, spp)
    S, Q = accum_ref.fold(col)
    rgb, var, noisy = accum_ref.resolve(S, Q, spp, 0.1)
    want, _ = ob.render(scene.desc, cam, seed, reg, ob.ORDER_ITERATIVE)
    assert np.array_equal(rgb, want)
    pixels = rgb.shape[0] * rgb.shape[1]
    assert 0 < noisy < pixels, (noisy, pixels)
    assert (var >= 0).all() and np.isfinite(var).all()
    # folding in two passes continues the same sums
    S2, Q2 = accum_ref.fold(col[3:], *accum_ref.fold(col[:3]))
    assert np.array_equal(S, S2) and np.array_equal(Q, Q2)
    if region is None:  # the cancellation rtx.h documents: negative before the clamp, on constant sky
        d = accum_ref.raw_variance(S, Q, spp)
        assert (d < 0).any() and (var[d < 0] == 0).all()
        print(f"negative before the clamp: {(d < 0).sum()} of {d.size}; noisy {noisy} of {pixels}")
