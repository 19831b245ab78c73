"""The test reference of the accumulator (rtx_accum, include/rtx.h): per-sample colours from the oracle
(oracle_binding.sample, iterative colour order, on the caller's tree), folded and resolved in numpy float32
exactly as rtx.h states — every operation its own correctly rounded float32 ufunc, no square root.

Test infrastructure, imported by test_accum_capi.py (CPU) and test_accum_gpu.py."""
from __future__ import annotations

import numpy as np

import oracle_binding as ob
import rtx

F = np.float32
_colours = {}


def shard_row(reg: rtx.Region, i: int) -> int:
    """rtx_region_row: the row (relative to y0) of shard row i."""
    s = max(int(reg.stripe), 1)
    return ((i // s) * reg.world + reg.rank) * s + i % s


def sample_colours(key, desc, cam, seed: int, reg: rtx.Region, n: int):
    """float32 [n, rows, width, 3]: the colour of sample k of every pixel of the region's shard.  Computed once per
    `key` (any hashable naming the scene and camera) and shared; never modified."""
    k = (key, seed, reg.x0, reg.y0, reg.width, reg.height, reg.rank, reg.world, reg.stripe)
    have = _colours.get(k)
    if have is not None and have.shape[0] >= n:
        return have[:n]
    rows = ob.region_rows(reg)
    out = np.zeros((n, rows, reg.width, 3), F)
    for i in range(rows):
        y = reg.y0 + shard_row(reg, i)
        for x in range(reg.width):
            for s in range(n):
                out[s, i, x] = ob.sample(desc, cam, seed, reg.x0 + x, y, s, ob.ORDER_ITERATIVE)[0]
    out.setflags(write=False)
    _colours[k] = out
    return out


def fold(colours, S=None, Q=None):
    """S = S + c; Q = Q + c * c in k order (the product rounded to float32 before the add)."""
    S = np.zeros(colours.shape[1:], F) if S is None else S.copy()
    Q = np.zeros(colours.shape[1:], F) if Q is None else Q.copy()
    for c in colours:
        S = S + c
        Q = Q + c * c
    assert S.dtype == F and Q.dtype == F
    return S, Q


def raw_variance(S, Q, n: int):
    """Q / n - mean^2 before the clamp (it cancels: small values of either sign on constant pixels)."""
    inv = F(1.0) / F(n)
    rgb = S * inv
    with np.errstate(invalid="ignore"):
        return Q * inv - rgb * rgb


def resolve(S, Q, n: int, rel_tol: float):
    """(rgb, var, noisy pixel count) of rtx_accum_resolve."""
    inv = F(1.0) / F(n)
    rgb = S * inv
    with np.errstate(invalid="ignore"):
        d = Q * inv - rgb * rgb
        v = np.where(d > 0, d, F(0.0)).astype(F)
        var = v * inv
        sv = (var[..., 0] + var[..., 1]) + var[..., 2]
        mb = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
        t = F(rel_tol) * np.where(mb > F(0.01), mb, F(0.01)).astype(F)
        noisy = sv > t * t
    assert rgb.dtype == F and var.dtype == F and sv.dtype == F and t.dtype == F
    return rgb, var, int(noisy.sum())


def after(colours, n: int, rel_tol: float):
    """resolve() after the first n samples."""
    S, Q = fold(colours[:n])
    return resolve(S, Q, n, rel_tol)
