"""The preview filter and the accumulator's previews on the GPU (rtx_denoise*, rtx_accum_preview*).

Exactness: the filter's arithmetic is the contract of include/rtx.h; tests/denoise_ref.py states it in numpy and the
kernels equal it bit for bit, NaN positions included.  Quality: on a window of the 1920 x 1080 randSpheres frame the
denoised 4-sample image must be closer to the converged one than the noisy image it was made from."""
import numpy as np
import pytest

import denoise_ref as dr
import rtx

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 7 * 12  # bytes after the image the call may write: they must keep their poison


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


def params(iterations=5, sigma_normal=0.45, sigma_depth=0.05, sigma_luminance=8.0):
    return rtx.DenoiseParams(iterations, sigma_normal, sigma_depth, sigma_luminance)


def denoise_dev(torch, rgb, var, guides, prm):
    """rtx_denoise_device on torch tensors: the output and the workspace poisoned with 0xFF, both longer than needed."""
    h, w = rgb.shape[:2]
    d = [to_device(torch, a) for a in (rgb, var, guides)]
    wb = rtx.denoise_workspace_bytes(w, h)
    out = torch.full((w * h * 12 + PAD,), 0xFF, dtype=torch.uint8, device="cuda")
    work = torch.full((wb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    rtx.denoise_device(*[t.data_ptr() for t in d], w, h, out.data_ptr(), work.data_ptr(), wb, prm, stream_of(torch))
    torch.cuda.synchronize()
    got, wk = out.cpu().numpy(), work.cpu().numpy()
    assert (got[w * h * 12:] == 0xFF).all() and (wk[wb:] == 0xFF).all(), "bytes past the end were written"
    for t, a in zip(d, (rgb, var, guides)):  # the inputs are read only
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    return got[: w * h * 12].view(F).reshape(h, w, 3)


def same(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:4], [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


# 1 x 1; 5 x 3; 17 x 9, smaller than the widest step; 70 x 37: two workgroups across and ten down, ragged in both;
# 129 x 5: just past two of the kernel's 64 x 4 workgroups in x and one in y
SIZES = [(1, 1, None), (5, 3, None), (17, 9, (4, 11)), (70, 37, (20, 33)), (129, 5, (2, 64))]


@pytest.mark.parametrize("w,h,nan_at", SIZES)
def test_filter_equals_the_reference(torch, w, h, nan_at):
    rgb, var, g = dr.synthetic(1000 * w + h, w, h, nan_at)
    assert (g["normal"] == 0).all(axis=2).any() == (w * h > 1) and (w * h == 1 or (var == 0).any())
    for it in range(1, 7):
        want = dr.denoise(rgb, var, g, iterations=it)
        assert np.isnan(want).any() == (nan_at is not None)
        same(denoise_dev(torch, rgb, var, g, params(it)), want)
    # other parameters; the host entry equals the device entry
    prm = params(4, 0.3, 0.2, 2.5)
    want = dr.denoise(rgb, var, g, 4, 0.3, 0.2, 2.5)
    same(denoise_dev(torch, rgb, var, g, prm), want)
    same(rtx.denoise(rgb, var, g, prm), want)
    same(rtx.denoise(rgb, var, g), dr.denoise(rgb, var, g))


def test_the_filter_smooths_and_keeps_edges(torch):
    """Not only equal to the reference: on the synthetic image without a NaN the output is finite and differs from the
    input (the edge-stopping properties are the reference's own, tests/test_denoise_capi.py)."""
    rgb, var, g = dr.synthetic(7, 70, 37)
    out = denoise_dev(torch, rgb, var, g, params())
    assert np.isfinite(out).all() and np.abs(out - rgb).max() > 0.01


_frame = {}


def frame(torch):
    """The 240 x 135 window at (840, 560) of the 1920 x 1080 randSpheres camera, seed 7: an accumulator at 4 samples
    with its resolved image and its preview.  Computed once and shared; test_the_filter_helps, the last test to use it,
    continues the accumulator."""
    if not _frame:
        host = rtx.HostScene("random_spheres", seed=1)
        cam = host.camera(width=1920, spp=4, depth=50)
        assert (cam.image_width, cam.image_height) == (1920, 1080)
        region = rtx.Region(840, 560, 240, 135, 0, 1)
        dev = rtx.DeviceScene(host.desc)
        acc = dev.accumulator(cam, 7, region)
        acc.add(4, stream=stream_of(torch))
        torch.cuda.synchronize()
        noisy, _, _ = acc.resolve()
        _frame.update(host=host, cam=cam, region=region, dev=dev, acc=acc, noisy=noisy, denoised=acc.preview(4))
    return _frame


def test_preview_equals_the_composed_calls(torch):
    f = frame(torch)
    acc, dev, cam, region = f["acc"], f["dev"], f["cam"], f["region"]
    assert acc.samples == 4
    w, h = region.width, region.height
    st = stream_of(torch)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    var = torch.zeros_like(rgb)
    acc.resolve_device(rgb.data_ptr(), var.data_ptr(), 0.0, st)
    guides = torch.zeros((w * h * 32,), dtype=torch.uint8, device="cuda")
    dev.guides_device(cam, 7, region, 0, 4, guides.data_ptr(), st)
    wb = rtx.denoise_workspace_bytes(w, h)
    work = torch.zeros((wb,), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(rgb)
    rtx.denoise_device(rgb.data_ptr(), var.data_ptr(), guides.data_ptr(), w, h, out.data_ptr(), work.data_ptr(), wb, None, st)
    prev = torch.full((w * h * 12 + PAD,), 0xFF, dtype=torch.uint8, device="cuda")
    acc.preview_device(prev.data_ptr(), 4, None, st)
    torch.cuda.synchronize()
    composed = out.cpu().numpy()
    got = prev.cpu().numpy()
    assert (got[w * h * 12:] == 0xFF).all()
    assert got[: w * h * 12].tobytes() == composed.tobytes()
    # and the composed calls equal the reference on the device's own resolve and guides
    g = guides.cpu().numpy().view(rtx.GUIDE_DTYPE).reshape(h, w)
    same(composed, dr.denoise(rgb.cpu().numpy(), var.cpu().numpy(), g))
    # guide_samples past n means n; fewer is another image; the host form and the PPM
    more = torch.zeros_like(rgb)
    acc.preview_device(more.data_ptr(), 9, rtx.DenoiseParams.defaults(), st)
    one = torch.zeros_like(rgb)
    acc.preview_device(one.data_ptr(), 1, None, st)
    torch.cuda.synchronize()
    assert more.cpu().numpy().tobytes() == composed.tobytes() and one.cpu().numpy().tobytes() != composed.tobytes()
    assert acc.preview(4).tobytes() == composed.tobytes()
    assert acc.preview_ppm(4) == b"P3\n%d %d\n255\n" % (w, h) + rtx.ppm_encode(composed)  # (the pixel lines: the host mirror's)
    with pytest.raises(rtx.RtxError) as e:
        acc.preview(0)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG
    assert f["denoised"].tobytes() == composed.tobytes() and f["noisy"].tobytes() == rgb.cpu().numpy().tobytes()


def test_preview_leaves_the_accumulator_alone(torch):
    """After a preview S, Q and n are unchanged: the resolve equals the one-shot render at 4 samples; and the
    previews' buffers are not scratch."""
    f = frame(torch)
    acc, dev, cam, region = f["acc"], f["dev"], f["cam"], f["region"]
    one_shot = torch.zeros((region.height, region.width, 3), dtype=torch.float32, device="cuda")
    dev.render_region(cam, 7, region, one_shot.data_ptr(), stream_of(torch))
    torch.cuda.synchronize()
    scratch = rtx.device_scratch_bytes(0)
    assert acc.preview(4).tobytes() == f["denoised"].tobytes()
    assert rtx.device_scratch_bytes(0) == scratch and acc.samples == 4
    rgb, var, _ = acc.resolve()
    assert rgb.tobytes() == f["noisy"].tobytes() == one_shot.cpu().numpy().tobytes()
    with pytest.raises(rtx.RtxError) as e:  # nothing accumulated yet
        dev.accumulator(cam, 7, rtx.Region(0, 0, 8, 8, 0, 1)).preview(4)
    assert e.value.code == rtx.RTX_ERR_INVALID_ARG


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.clip(a, 0, 1).astype(np.float64) - np.clip(ref, 0, 1)) ** 2)))


def test_the_filter_helps(torch):
    """RMSE(clip(denoised)) < RMSE(clip(noisy)) against the same accumulator continued to 1024 samples.  The bound
    is 1: the filter must help.  (Measured on the MI355X: 0.0836 noisy, 0.0355 denoised, ratio 0.425; the CPU prototype
    of the arithmetic measured 0.43 on this window.)"""
    f = frame(torch)
    acc = f["acc"]
    assert acc.samples == 4
    acc.add(1020, stream=stream_of(torch))
    torch.cuda.synchronize()
    assert acc.samples == 1024
    converged, _, _ = acc.resolve()
    noisy, denoised = rmse(f["noisy"], converged), rmse(f["denoised"], converged)
    print(f"RMSE against 1024 spp: noisy 4 spp {noisy:.4f}, denoised {denoised:.4f}, ratio {denoised / noisy:.3f}")
    assert np.isfinite(f["denoised"]).all()
    assert denoised < noisy


def test_zz_device_check_and_close(torch):
    """Last in the module: every call above left the device's sticky error word clean; free the module's scene."""
    rtx.device_check(0)
    if _frame:
        _frame.pop("acc").close()
        _frame.pop("dev").close()
        _frame.clear()
