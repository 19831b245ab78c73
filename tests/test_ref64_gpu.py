"""The HIP kernel against the independent float64 reference (tests/ref64.py), directly.

No oracle here: the kernel's images come through parity.gpu_region (rtx_render_region_device) and
are compared with ref64's float64 colours on the samples ref64 itself keeps (its float32 and
float64 runs decide alike, no tie), within the tolerance ref64's own two precisions give
(tests/test_ref64.py states the rule).  Both kernels run on every case of tests/ref64_cases.py —
the timed one (the assembly walk bench.py measures) and the counting one (the C++ walk) — and
where a case leaves nothing out the counting kernel's segments, hits, rng draws and texel fetches
must equal ref64's own counts.  ref64 scans every primitive without a tree, so this also checks
whatever walk the scene takes (the caller's list or tree, a rebuilt tree, two tiers).
"""
import numpy as np
import pytest

import parity
import ref64_cases as rc
import rtx

pytestmark = pytest.mark.gpu

TOL_MAX = 1e-5
COUNTER_KEYS = ("samples", "segments", "hits", "rng_draws", "texel_fetches")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


def check_kernel(torch, b, flags=0):
    r = b.ref
    print("\n" + b.report())
    assert r.left_out <= b.cap and r.tol <= TOL_MAX and r.kept.any()
    dev = rtx.DeviceScene(b.desc)
    try:
        for kernel in ("timed", "counting"):
            img, st = parity.gpu_region(torch, dev, b.cam, b.seed, b.region, counters=(kernel == "counting"),
                                        flags=flags)
            assert img.shape == (b.window[3], b.window[2], 3)
            assert np.isfinite(img.reshape(-1, 3)[r.kept]).all(), kernel
            worst = r.worst(img)
            print(f"{kernel} kernel: max |delta| on kept pixels {worst:.3g}")
            assert worst <= r.tol, f"{b.name}: {kernel} kernel {worst} from ref64 on a kept pixel, tol {r.tol}"
            if kernel == "counting" and r.left_out == 0:
                assert {k: int(getattr(st, k)) for k in COUNTER_KEYS} == r.counters()
    finally:
        dev.close()


@pytest.mark.parametrize("name", rc.NAMES)
def test_kernel_against_ref64(torch_cuda, built, name):
    check_kernel(torch_cuda, rc.built(name))


@pytest.mark.parametrize("name", rc.NO_LDS_CASES)
def test_kernel_against_ref64_from_global_memory(torch_cuda, built, name):
    """RTX_FLAG_NO_LDS: the scene read from global memory instead of the LDS copy."""
    check_kernel(torch_cuda, rc.built(name), flags=rtx.RTX_FLAG_NO_LDS)
