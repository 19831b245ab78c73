"""The test reference of the denoised previews (include/rtx.h): the fold of first-hit samples into
guide images and the edge-avoiding a-trous filter, in numpy float32 exactly as rtx.h states them: every operation its
own correctly rounded float32 ufunc, no fused multiply-add, no square root, no exp.

Test infrastructure, imported by test_denoise_capi.py (CPU), test_guides_gpu.py and test_denoise_gpu.py."""
from __future__ import annotations

import numpy as np

F = np.float32
GUIDE_FIELDS = [("albedo", "<f4", (3,)), ("cover", "<f4"), ("normal", "<f4", (3,)), ("depth", "<f4")]
GUIDE = np.dtype(GUIDE_FIELDS)  # rtx_guide, 32 B
K3 = (1, 2, 1)
K5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
DEFAULTS = dict(iterations=5, sigma_normal=0.45, sigma_depth=0.05, sigma_luminance=8.0)


def fold_guides(a, n, t, hit):
    """rtx_guide of every pixel from its samples in k order.  a, n: float32 [count, ..., 3], the albedo and the normal
    of each sample ((1, 1, 1) and 0 on a miss); t: float32 [count, ...]; hit: bool [count, ...]."""
    a, n, t = np.asarray(a, F), np.asarray(n, F), np.asarray(t, F)
    hit = np.asarray(hit, bool)
    count, shape = a.shape[0], a.shape[1:-1]
    A, N = np.zeros(shape + (3,), F), np.zeros(shape + (3,), F)
    Z, c = np.zeros(shape, F), np.zeros(shape, np.uint32)
    with np.errstate(all="ignore"):
        for k in range(count):
            A = A + a[k]
            N = N + n[k]
            Z = np.where(hit[k], Z + t[k], Z).astype(F)
            c = c + hit[k].astype(np.uint32)
        inv = F(1.0) / F(count)
        out = np.zeros(shape, GUIDE)
        out["albedo"] = A * inv
        out["normal"] = N * inv
        out["cover"] = c.astype(F) * inv
        out["depth"] = np.where(c > 0, Z / np.where(c > 0, c, 1).astype(F), F(0.0))
    assert A.dtype == F and N.dtype == F and Z.dtype == F
    return out


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that lies in the image; inside: where it does."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _stop(x):
    y = F(1.0) - x
    return np.where(y > 0, y, F(0.0)).astype(F)


def prepare(rgb, var, guides):
    """(c [H, W, 3], v [H, W], a [H, W, 3]): the colour without its albedo, the summed variance, the floored albedo."""
    rgb, var = np.asarray(rgb, F), np.asarray(var, F)
    with np.errstate(all="ignore"):
        a = np.where(guides["albedo"] > F(0.01), guides["albedo"], F(0.01)).astype(F)
        c = rgb / a
        q = var / (a * a)
        v = (q[..., 0] + q[..., 1]) + q[..., 2]
    assert c.dtype == F and v.dtype == F
    return c, v, a


def level(c, v, guides, s: int, sigma_normal, sigma_depth, sigma_luminance):
    """One a-trous level at step s: (c, v) -> (c', v')."""
    n, z = np.asarray(guides["normal"], F), np.asarray(guides["depth"], F)
    sn, sd, sl = F(sigma_normal), F(sigma_depth), F(sigma_luminance)
    H, W = v.shape
    with np.errstate(all="ignore"):
        sv, sk = np.zeros((H, W), F), np.zeros((H, W), F)
        for b in (-1, 0, 1):
            for a in (-1, 0, 1):
                k = F(K3[b + 1] * K3[a + 1])
                vq, inside = _shift(v, a, b)
                sv = np.where(inside, sv + k * vq, sv).astype(F)
                sk = np.where(inside, sk + k, sk).astype(F)
        vb = sv / sk
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        dl = (sl * sl) * vb + F(1e-6)
        sn2 = sn * sn
        Wt, V, C = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                nq, inside = _shift(n, s * dx, s * dy)
                zq, _ = _shift(z, s * dx, s * dy)
                cq, _ = _shift(c, s * dx, s * dy)
                vq, _ = _shift(v, s * dx, s * dy)
                lq, _ = _shift(lum, s * dx, s * dy)
                dn = n - nq
                xn = ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) / sn2
                m = F(s * max(abs(dx), abs(dy)))
                zm = np.where(z > zq, z, zq).astype(F)
                tz = (sd * m) * zm
                dz = z - zq
                xz = (dz * dz) / (tz * tz + F(1e-6))
                d = lum - lq
                xl = (d * d) / dl
                w = (((K5[dy + 2] * K5[dx + 2]) * _stop(xn)) * _stop(xz)) * _stop(xl)
                take = inside & (w > 0)
                Wt = np.where(take, Wt + w, Wt).astype(F)
                C = np.where(take[..., None], C + w[..., None] * cq, C).astype(F)
                V = np.where(take, V + (w * w) * vq, V).astype(F)
        c2 = C / Wt[..., None]
        v2 = V / (Wt * Wt)
    for arr in (vb, dl, xn, xz, xl, w, c2, v2):
        assert arr.dtype == F
    return c2, v2


def denoise(rgb, var, guides, iterations=5, sigma_normal=0.45, sigma_depth=0.05, sigma_luminance=8.0, levels=None):
    """rtx_denoise: float32 [H, W, 3].  levels (a list): receives (c, v) after prepare and after every level."""
    assert 1 <= iterations <= 6 and guides.dtype == GUIDE
    c, v, a = prepare(rgb, var, guides)
    if levels is not None:
        levels.append((c, v))
    for i in range(iterations):
        c, v = level(c, v, guides, 1 << i, sigma_normal, sigma_depth, sigma_luminance)
        if levels is not None:
            levels.append((c, v))
    with np.errstate(all="ignore"):
        out = c * a
    assert out.dtype == F
    return out


def synthetic(seed: int, width: int, rows: int, nan_at=None):
    """Seeded (rgb, var, guides) of a width x rows image: a sky region (zero normal, depth 0, cover 0, albedo 1) in
    the top left, a sphere-like region with varying normals and depth elsewhere, a patch of zero variance, albedos on
    both sides of the 0.01 floor, and optionally one NaN pixel with variance 0 (what resolve writes for it)."""
    rs = np.random.default_rng(seed)
    g = np.zeros((rows, width), GUIDE)
    ys, xs = np.mgrid[0:rows, 0:width]
    sky = (xs + 2 * ys) < (width + rows) // 3
    nrm = rs.normal(size=(rows, width, 3)) * 0.05 + np.array([0.2, 0.3, 0.9])
    nrm[:, width // 2:] = rs.normal(size=(rows, width - width // 2, 3)) * 0.05 + np.array([-0.8, 0.1, 0.5])  # an edge
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    g["normal"] = np.where(sky[..., None], 0, nrm).astype(F)
    g["depth"] = np.where(sky, 0, 3 + 0.02 * xs + 0.01 * ys + 0.002 * rs.random((rows, width))).astype(F)
    g["cover"] = np.where(sky, 0, 1).astype(F)
    alb = rs.random((rows, width, 3)) * 0.9 + 0.05
    alb[rs.random((rows, width)) < 0.1] = 0.004  # below the floor
    g["albedo"] = np.where(sky[..., None], 1, alb).astype(F)
    rgb = (np.where(sky[..., None], [0.6, 0.7, 1.0], g["albedo"] * 0.8) * (1 + 0.3 * rs.normal(size=(rows, width, 3)))).astype(F)
    var = (0.02 * rs.random((rows, width, 3)) ** 2).astype(F)
    var[rows // 3: rows // 3 + 3, width // 4: width // 4 + 5] = 0  # zero variance
    if nan_at is not None:
        y, x = nan_at
        rgb[y, x] = np.nan
        var[y, x] = 0
    return rgb, var, g
