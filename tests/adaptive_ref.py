"""The test reference of adaptive sampling (rtx_accum_add_adaptive, include/rtx.h "adaptive sampling"): the selection
per tile with resolve's float32 formula, the fold over the open tiles only, and the resolve at every pixel's own
sample count, in numpy float32 on accum_ref's per-sample colours — every operation its own correctly rounded ufunc.

Test infrastructure, imported by test_adaptive_capi.py (CPU) and test_adaptive_gpu.py."""
from __future__ import annotations

import numpy as np

import accum_ref
import oracle_binding as ob

F = np.float32
COUNT_KEYS = ("samples", "segments", "hits", "texel_fetches", "rng_draws", "node_visits", "prim_tests")
_counters = {}


def resolve(S, Q, n, rel_tol: float):
    """(rgb, var, noisy mask) of rtx_accum_resolve at n samples: a scalar, or a uint32 [rows, width] map of n_p."""
    inv = F(1.0) / np.asarray(n, np.uint32).astype(F)
    if inv.ndim:
        inv = inv[..., None]
    rgb = S * inv
    with np.errstate(invalid="ignore"):
        d = Q * inv - rgb * rgb
        v = np.where(d > 0, d, F(0.0)).astype(F)
        var = v * inv
        sv = (var[..., 0] + var[..., 1]) + var[..., 2]
        mb = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
        t = F(rel_tol) * np.where(mb > F(0.01), mb, F(0.01)).astype(F)
        noisy = sv > t * t  # (a NaN compares false: not noisy)
    assert rgb.dtype == F and var.dtype == F and sv.dtype == F and t.dtype == F
    return rgb, var, noisy


def tiles(rows: int, width: int, tile_shape):
    """The tiles of a rows x width shard as index slices, row-major: they start at the shard's first row and column, the
    last of a row or column may be partial."""
    tw, th = tile_shape
    return [(slice(y, min(y + th, rows)), slice(x, min(x + tw, width))) for y in range(0, rows, th) for x in range(0, width, tw)]


class Result:
    """counts: uint32 [rows, width], n_p; S, Q: the sums; passes: per pass (open_tiles, open_pixels, open mask)."""

    def __init__(self, counts, S, Q, passes, n):
        self.counts, self.S, self.Q, self.passes, self.n = counts, S, Q, passes, n

    def resolved(self, rel_tol: float):
        """(rgb, var, noisy count) of rtx_accum_resolve on the adaptive accumulator: every pixel at its own n_p."""
        rgb, var, noisy = resolve(self.S, self.Q, self.counts, rel_tol)
        return rgb, var, int(noisy.sum())


def simulate(colours, tile_shape, passes, rel_tol: float, min_samples: int) -> Result:
    """rtx_accum_add_adaptive(count, rel_tol, min_samples) for every count of `passes` on a new accumulator whose
    sample k of every pixel is colours[k] (float32 [n, rows, width, 3], accum_ref.sample_colours)."""
    rows, width = colours.shape[1:3]
    tl = tiles(rows, width, tile_shape)
    closed = np.zeros((rows, width), np.uint32)  # 0: open, else the n the pixel's tile closed at
    S = np.zeros((rows, width, 3), F)
    Q = np.zeros((rows, width, 3), F)
    n, per_pass = 0, []
    for count in passes:
        if n >= max(min_samples, 1):  # select
            noisy = resolve(S, Q, n, rel_tol)[2]
            for t in tl:
                if (closed[t] == 0).all() and not noisy[t].any():
                    closed[t] = n
        is_open = closed == 0
        S2, Q2 = accum_ref.fold(colours[n:n + count], S, Q)  # sample: the open tiles' sums alone move
        S = np.where(is_open[..., None], S2, S)
        Q = np.where(is_open[..., None], Q2, Q)
        n += count  # whether or not a tile was open
        per_pass.append((sum(1 for t in tl if is_open[t].all()), int(is_open.sum()), is_open))
    assert S.dtype == F and Q.dtype == F
    return Result(np.where(closed == 0, np.uint32(n), closed).astype(np.uint32), S, Q, per_pass, n)


def sample_counters(key, desc, cam, seed: int, reg, n: int):
    """uint64 [n, rows, width, len(COUNT_KEYS)]: the oracle's work counters of sample k of every pixel of the shard
    (oracle_binding.sample on desc's tree).  Computed once per key and shared, as accum_ref.sample_colours is."""
    k = (key, seed, reg.x0, reg.y0, reg.width, reg.height, reg.rank, reg.world, reg.stripe)
    have = _counters.get(k)
    if have is not None and have.shape[0] >= n:
        return have[:n]
    rows = ob.region_rows(reg)
    out = np.zeros((n, rows, reg.width, len(COUNT_KEYS)), np.uint64)
    for i in range(rows):
        y = reg.y0 + accum_ref.shard_row(reg, i)
        for x in range(reg.width):
            for s in range(n):
                cnt = ob.sample(desc, cam, seed, reg.x0 + x, y, s, ob.ORDER_ITERATIVE)[1]
                out[s, i, x] = [cnt[name] for name in COUNT_KEYS]
    out.setflags(write=False)
    _counters[k] = out
    return out


def pass_counters(counters, result: Result, passes):
    """Per pass: {name: sum over the pass's samples of its open pixels} from sample_counters' array."""
    out, n = [], 0
    for count, (_, _, is_open) in zip(passes, result.passes):
        tot = counters[n:n + count][:, is_open].sum(axis=(0, 1))
        out.append({name: int(v) for name, v in zip(COUNT_KEYS, tot)})
        n += count
    return out
