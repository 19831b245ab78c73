"""Inputs and strict float32 numpy references for tests/device_math_check.hip.

numpy's float32 `/` and `sqrt` are correctly rounded and an array expression rounds after every operation (no
contraction), so these references depend on neither the device compiler nor the host one.  Every generator is
deterministic; tests/test_device_math.py asserts, on the CPU, that the inputs reach the edges they are meant to reach.
"""
import itertools

import numpy as np

F = np.float32
U = np.uint32
INF = F(np.inf)
NAN = F(np.nan)


def fl(b):
    return np.asarray(b, U).view(F)


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def near(x, k=1):
    """x and its k neighbours on each side (bit patterns; x > 0 finite)."""
    b = int(np.array(x, F).view(U))
    return fl(np.arange(b - k, b + k + 1, dtype=np.int64).astype(U))


def same(a, b):
    """Bit equality of float32 arrays, NaN equal to NaN."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def pad64(a, fill):
    """a (n, w) padded with `fill` rows to whole waves of 64 records."""
    n = (-len(a)) % 64
    return np.concatenate([a, np.broadcast_to(np.asarray(fill, a.dtype), (n,) + a.shape[1:])]) if n else a


# ---- InBoundary / Aabb.Hit (bvh.go:52-61, 84-102) -------------------------------------------------------------------
def in_boundary(d, o, lo, hi, tmin, tmax):
    """InBoundary (bvh.go:84-102) in float32, elementwise."""
    with np.errstate(all="ignore"):
        inv = F(1) / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        sw = inv < 0
        t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
        tmin = np.where(t0 > tmin, t0, tmin)
        tmax = np.where(t1 < tmax, t1, tmax)
    return tmin < tmax, tmin, tmax


def aabb_hit(o, d, lo, hi, tmin, tmax):
    ok = np.ones(len(o), bool)
    tmin = np.full(len(o), tmin, F)
    tmax = np.full(len(o), tmax, F)
    for k in range(3):
        hit, a, b = in_boundary(d[:, k], o[:, k], lo[:, k], hi[:, k], tmin, tmax)
        tmin, tmax = np.where(ok, a, tmin), np.where(ok, b, tmax)
        ok &= hit
    return ok


def aabb_hit_detail(o, d, lo, hi, tmin, tmax):
    """(Aabb.Hit, undecided before the last axis, the final tmin, the final tmax)."""
    ok = np.ones(len(o), bool)
    tmin = np.array(np.broadcast_to(tmin, len(o)), F)
    tmax = np.array(np.broadcast_to(tmax, len(o)), F)
    before_last = ok
    for k in range(3):
        before_last = ok.copy()
        hit, a, b = in_boundary(d[:, k], o[:, k], lo[:, k], hi[:, k], tmin, tmax)
        tmin, tmax = np.where(ok, a, tmin), np.where(ok, b, tmax)
        ok &= hit
    return ok, before_last, tmin, tmax


# ---- the compiler's own forms ---------------------------------------------------------------------------------------
EDGE_FIELDS = (0, 1, 2, 31, 252, 253, 254, 255)


def forms_inputs():
    """Every 257th bit pattern, and every pattern within 64 of an exponent-field change at EDGE_FIELDS, both signs."""
    parts = [np.arange(0, 1 << 32, 257, dtype=np.int64)]
    for f in EDGE_FIELDS:
        for edge in (f << 23, (f + 1) << 23):  # where field f begins and where it ends
            w = np.arange(edge - 64, edge + 64, dtype=np.int64)
            w = w[(w >= 0) & (w < (1 << 31))]
            parts += [w, w | (1 << 31)]
    return pad64(np.concatenate(parts).astype(U)[:, None], U(0x3F800000))[:, 0]


def rcp_ref(x):
    with np.errstate(all="ignore"):
        return F(1) / np.asarray(x, F)


def sqrt_ref(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, F))


# ---- wave layouts for the votes -------------------------------------------------------------------------------------
def vote_layout(fast, slow, filler):
    """Records (n, w) inside a vote's fast domain and records outside it, laid out as 64-lane waves:
       whole fast waves (63 records and `filler`), then the same waves with the filler's lane given to a slow record —
       the lane moves from wave to wave —, then whole slow waves.
    Returns (records, index of each fast record in the fast waves, the same in the mixed waves)."""
    fast, slow = np.asarray(fast), np.asarray(slow)
    fast = np.concatenate([fast, np.broadcast_to(filler, ((-len(fast)) % 63,) + fast.shape[1:])])
    k = len(fast) // 63
    own = np.arange(64)[None, :] != (np.arange(k) * 5 % 64)[:, None]  # every lane but the outsider's
    a = np.empty((k, 64) + fast.shape[1:], fast.dtype)
    a[own] = fast  # row-major: wave i holds records 63 i .. 63 i + 62
    b = a.copy()
    a[~own] = filler
    b[~own] = slow[np.arange(k) % len(slow)]
    rec = np.concatenate([a.reshape((-1,) + fast.shape[1:]), b.reshape((-1,) + fast.shape[1:]), pad64(slow, slow[0])])
    idx = np.flatnonzero(own.reshape(-1))
    return rec, idx, idx + 64 * k


def wave_kinds(pred):
    """(whole waves inside, mixed waves, whole waves outside) of a per-lane predicate."""
    n = pred.reshape(-1, 64).sum(1)
    return int((n == 64).sum()), int(((n > 0) & (n < 64)).sum()), int((n == 0).sum())


def rcp_fast_pred(x):
    e = (bits(x) >> 23) & 0xFF
    return (e >= 2) & (e <= 252)


# sqrt_rn_fast(NEG_SUBNORMAL) is -0 (v_sqrt_f32 flushes it) where sqrt is NaN: the first GPU run of the exhaustive section
# found all 2^23 - 1 negative subnormals, after which sqrt_rn's vote went from 0 <= x < 2^-96 to |x| < 2^-96.
NEG_SUBNORMAL = fl(0x80607CE6)


def sqrt_slow_pred(x):
    """sqrt_rn's vote: a lane with |x| < 2^-96 sends its wave to the builtin."""
    return np.abs(np.asarray(x, F)) < F(2.0 ** -96)


def unit_fast_pred(q):
    q = np.asarray(q, F)
    return (q >= F(2.0 ** -96)) & (q < INF)


def _patterns(rng, n, lo_field, hi_field, signs=True):
    b = (rng.integers(lo_field, hi_field + 1, n).astype(U) << 23) | rng.integers(0, 1 << 23, n).astype(U)
    if signs:
        b |= rng.integers(0, 2, n).astype(U) << 31
    return fl(b)


def rcp_vote_inputs():
    rng = np.random.default_rng(11)
    edge = np.concatenate([near(2.0 ** -125, 3)[3:], near(2.0 ** 126, 3)[:3], [F(1), F(3), F(2.0 ** -125), F(2.0 ** 125)]])
    fast = np.concatenate([edge, -edge, _patterns(rng, 4000, 2, 252)]).astype(F)
    slow = np.concatenate([[F(0), F(-0.0), NAN, INF, -INF], near(2.0 ** -125, 3)[:3], near(2.0 ** 126, 3)[3:],
                           fl([1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF]), _patterns(rng, 100, 0, 1),
                           _patterns(rng, 100, 253, 255)]).astype(F)
    assert rcp_fast_pred(fast).all() and not rcp_fast_pred(slow).any()
    return vote_layout(fast[:, None], slow[:, None], F(1.5))


def sqrt_vote_inputs():
    rng = np.random.default_rng(12)
    fast = np.concatenate([near(2.0 ** -96, 3)[3:], [F(1), F(2), F(4), INF, F(3.4028235e38)],
                           _patterns(rng, 4000, 31, 254, signs=False), [F(-1), NAN, -INF], -near(2.0 ** -96, 3)[3:],
                           -_patterns(rng, 100, 31, 254, signs=False)]).astype(F)
    slow = np.concatenate([[F(0), F(-0.0), NEG_SUBNORMAL], near(2.0 ** -96, 3)[:3], -near(2.0 ** -96, 3)[:3],
                           fl([1, 0x007FFFFF, 0x00800000, 0x80000001, 0x807FFFFF, 0x80800000]),
                           _patterns(rng, 200, 0, 30)]).astype(F)
    assert not sqrt_slow_pred(fast).any() and sqrt_slow_pred(slow).all()
    return vote_layout(fast[:, None], slow[:, None], F(2.25))


def lensq_ref(v):
    with np.errstate(all="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def unit_ref(v):
    """v * (1 / sqrt(x*x + y*y + z*z)), float32, left to right (vec3.go:103-113)."""
    with np.errstate(all="ignore"):
        return v * (F(1) / np.sqrt(lensq_ref(v)))[:, None]


def unit_vote_inputs():
    rng = np.random.default_rng(13)
    n = 6000
    v = np.stack([_patterns(rng, n, 0, 190) for _ in range(3)], 1)  # subnormal .. 2^63
    same_scale = _patterns(rng, n, 0, 190)[:, None] * rng.uniform(-1, 1, (n, 3)).astype(F)
    axis = np.zeros((40, 3), F)
    axis[:10, 0] = np.concatenate([near(2.0 ** -48, 2), near(2.0 ** 64, 2)])  # q on both sides of 2^-96 and of inf
    axis[10:20, 1] = axis[:10, 0]
    axis[20:30, 2] = -axis[:10, 0]
    axis[30:33] = [[INF, 1, 1], [1, NAN, 1], [0, 0, -0.0]]
    axis[33:36] = [[1, 2, 2], [3e-30, 0, 0], [-INF, INF, 0]]
    axis[36:] = [[1e-45, 0, 0], [2.0 ** 63, 2.0 ** 63, 2.0 ** 63], [2.0 ** 63, 2.0 ** 63, -2.0 ** 63], [0, 1e-38, 0]]
    pool = np.concatenate([v, same_scale, axis]).astype(F)
    ok = unit_fast_pred(lensq_ref(pool))
    return vote_layout(pool[ok], pool[~ok], np.array([1, 2, 2], F))


# ---- trav_begin -----------------------------------------------------------------------------------------------------
def trav_ref(o, d):
    """(ix, iy, iz, ra, a, flags of trav_begin<false>, flags of trav_begin<true>), the documented predicates written out:
    safe = 1/dir and the origin finite and a in [2^-60, 2^60]; with FMA, |1/dir| <= 2^64 and |origin| <= 2^32 as well
    (which imply the finite tests).  flags = nx | ny << 1 | nz << 2 | safe << 3."""
    with np.errstate(all="ignore"):
        a = lensq_ref(d)
        inv = F(1) / d
        ra = F(1) / a
        neg = inv < 0
        a_ok = (a >= F(2.0 ** -60)) & (a <= F(2.0 ** 60))
        safe = np.isfinite(inv).all(1) & np.isfinite(o).all(1) & a_ok
        fma_ok = (np.abs(inv) <= F(2.0 ** 64)).all(1) & (np.abs(o) <= F(2.0 ** 32)).all(1)
    base = neg[:, 0].astype(U) | neg[:, 1].astype(U) << 1 | neg[:, 2].astype(U) << 2
    return inv, ra, a, base | safe.astype(U) << 3, base | (fma_ok & a_ok).astype(U) << 3, fma_ok


def trav_fast_pred(d):
    return rcp_fast_pred(d).all(1) & rcp_fast_pred(lensq_ref(d))


DIR_LIST = np.concatenate([
    [F(0), F(-0.0)], fl([1, 0x007FFFFF]), [F(2.0 ** -126)], near(2.0 ** -125), near(2.0 ** 125), near(2.0 ** 126),
    [F(3.4028235e38), INF, -INF, NAN], near(2.0 ** -64), -near(2.0 ** -64), [F(1), F(-0.3), F(7.5), F(-2.0 ** -125),
                                                                              F(-2.0 ** 126)]]).astype(F)
ORIGIN_LIST = np.concatenate([[F(0), F(1.5), F(-7)], near(2.0 ** 32), -near(2.0 ** 32), [INF, NAN, F(-0.0),
                                                                                        F(3e38)]]).astype(F)


def trav_inputs():
    """(o, d) rows: every triple of DIR_LIST with origins walking through ORIGIN_LIST, then rays whose a = lensq(d) is
    2^-60, 2^60 and their neighbours (d = s * (1, 2^-20, 2^-20): a = RN(s^2), every 1/d finite), ordinary origins."""
    d = np.array(list(itertools.product(DIR_LIST, repeat=3)), F)
    i = np.arange(len(d))
    m = len(ORIGIN_LIST)
    o = np.stack([ORIGIN_LIST[(i // 7) % m], ORIGIN_LIST[(i // 3 + 5) % m], ORIGIN_LIST[(i + 9) % m]], 1)
    o[i % 3 == 0] = [0.5, -1.0, 2.0]  # a third of the rays with a plain origin: `safe` then hangs on d alone
    s = np.concatenate([near(2.0 ** 30, 3), near(2.0 ** -30, 3), -near(2.0 ** 30, 3), near(2.0 ** 30 * 1.4142135, 2)])
    # the second component adds nothing, half an ulp or an ulp to s^2: a lands on the edge's direct neighbours too
    da = np.concatenate([np.stack([s, s * F(m), -s * F(2.0 ** -20)], 1) for m in (2.0 ** -20, 2.0 ** -12, 2.0 ** -11.5,
                                                                                 2.0 ** -11)]).astype(F)
    da = np.concatenate([da, da[:, (1, 2, 0)], da[:, (2, 0, 1)]])
    oa = np.tile(np.array([[0.5, -1.0, 2.0], [2.0 ** 32, 0, 0], [0, -(2.0 ** 32) * (1 + 2.0 ** -23), 0]], F),
                 (len(da) // 3 + 1, 1))[: len(da)]
    o, d = np.concatenate([o, oa]), np.concatenate([d, da])
    ok = trav_fast_pred(d)
    rec = np.concatenate([o, d], 1)
    return vote_layout(rec[ok], rec[~ok], np.array([0.5, -1, 2, 1, 2, -2], F))


# ---- box_hit --------------------------------------------------------------------------------------------------------
BOX_SEED = 7
BOX_N = 1 << 19


def box_inputs(seed=BOX_SEED, n=BOX_N):
    """(o, d, lo, hi, closest, tmin): the tie-rich lattice.  Box corners and origins on a 0.5 grid, +-0 faces, flat
    boxes; d = target - origin scaled by a power of two, some components tiny but with a finite 1/d, some exactly 0;
    closest = inf or on a 0.125 grid; tmin in {0.001, 2^-126, 0.5}."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(-4, 4, (n, 3)).astype(F) * F(0.5)
    hi = lo + rng.integers(0, 4, (n, 3)).astype(F) * F(0.5)  # a quarter of the axes flat
    z = rng.random((n, 3)) < 0.5
    lo = np.where(z & (lo == 0), F(-0.0), lo)
    hi = np.where(~z & (hi == 0), F(-0.0), hi)
    o = rng.integers(-6, 7, (n, 3)).astype(F) * F(0.5)
    o = np.where((rng.random((n, 3)) < 0.3) & (o == 0), F(-0.0), o)
    target = lo + rng.integers(0, 5, (n, 3)).astype(F) * F(0.25) * (hi - lo) + \
        rng.integers(-1, 2, (n, 3)).astype(F) * F(0.5) * (rng.random((n, 3)) < 0.2)
    d = (target - o).astype(F)
    d = d * F(2.0) ** rng.integers(-3, 4, (n, 1)).astype(F)
    tiny = rng.random((n, 3)) < 0.04
    d = np.where(tiny, rng.choice(np.array([2.0 ** -70, -2.0 ** -70, 2.0 ** -100, -2.0 ** -20], F), (n, 3)), d)
    zero = rng.random((n, 3)) < 0.02
    d = np.where(zero, rng.choice(np.array([0.0, -0.0], F), (n, 3)), d).astype(F)
    closest = np.where(rng.random(n) < 0.3, INF, rng.integers(1, 64, n).astype(F) * F(0.125)).astype(F)
    tmin = rng.choice(np.array([0.001, 2.0 ** -126, 0.5], F), n)
    return o, d, lo, hi, closest, tmin


def med3_plain(a, b, c):
    """The plain median of three (NaN sorted last): what a slab clamp gives without the reference's NaN rule."""
    return np.sort(np.stack([a, b, c]), 0)[1]


def box_med3_plain(o, d, lo, hi, closest, tmin):
    with np.errstate(all="ignore"):
        inv = F(1) / d
        ta, tb = (lo - o) * inv, (hi - o) * inv
        l, h = tmin, closest
        for k in range(3):
            l, h = med3_plain(l, ta[:, k], tb[:, k]), med3_plain(h, ta[:, k], tb[:, k])
    return l < h


# ---- sphere_test ----------------------------------------------------------------------------------------------------
def sphere_ref(o, d, c, r, closest, tmin):
    """(*Sphere).Hit, hittables.go:96-116, in float32: (hit, t, which) with which = 1 / 2 for the root taken, 0 for a
    negative discriminant, -1 for a miss by tmin (the later root is not past tmin), -2 for a miss by closest."""
    with np.errstate(all="ignore"):
        oc = o - c
        a = lensq_ref(d)
        hb = (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1]) + d[:, 2] * oc[:, 2]
        cc = lensq_ref(oc) - r * r
        disc = hb * hb - a * cc
        sq = np.sqrt(disc)
        r1, r2 = (-hb - sq) / a, (-hb + sq) / a
        in1 = (tmin < r1) & (r1 < closest)
        in2 = (tmin < r2) & (r2 < closest)
        has = disc >= 0
        which = np.where(~has, 0, np.where(in1, 1, np.where(in2, 2, np.where(tmin < r2, -2, -1))))
        t = np.where(which == 1, r1, np.where(which == 2, r2, closest)).astype(F)
    return which > 0, t, which, disc


def sphere_inputs():
    """(o, d, c, r, closest, tmin), every direction component non-zero:
       tangent rays (d = s * (1, 2, 2), the tangent point c + r * (2, -2, 1) / 3 with r = 3 * 2^j: disc is exactly 0),
       rays along (1, 2^-13, -2^-13) scaled so that a = 2^-60 .. 2^60, origins outside, inside and at the centre,
       radii 2^-20 .. 2^20; closest = inf, a root, its neighbours, half and twice it; tmin in {0.001, 2^-126}."""
    rows = []
    g = np.arange(-10, 11) * 0.125
    for j in (-20, -12, -5, -1, 0, 3, 9, 20):
        sc = 2.0 ** j
        c = np.array([0.5, -1.0, 1.5]) if abs(j) <= 5 else np.zeros(3)
        for e in (-30, -29, -3, 0, 2, 29, 30):  # a = 2^(2e) (1 + 2^-25) -> RN: 2^(2e)
            dd = np.array([1.0, 2.0 ** -13, -(2.0 ** -13)]) * 2.0 ** e
            for u in g:
                for v in g[::4]:
                    for x0 in (-4.0, -0.5, 0.0, 3.0):  # in front, inside, centre plane, behind
                        rows.append((c + sc * np.array([x0, u, v]), dd, c, sc))
            rows.append((c, dd, c, sc))  # at the centre
        for m in (1, 2, 3, 5, 8):  # tangent rays
            for s in (2.0 ** -30 / 3, 0.25, 1.0, 4.0, 2.0 ** 30 / 3):
                dd = np.array([1.0, 2.0, 2.0]) * s
                for n_ in (np.array([2.0, -2.0, 1.0]), np.array([-2.0, 1.0, 2.0]) * np.array([1, -1, 1])):
                    if abs(dd @ n_) > 0:
                        continue
                    rows.append((c + sc * (n_ - m * np.array([1.0, 2.0, 2.0])), dd, c, 3 * sc))
    o = np.array([r_[0] for r_ in rows], F)
    d = np.array([r_[1] for r_ in rows], F)
    c = np.array([r_[2] for r_ in rows], F)
    r = np.array([r_[3] for r_ in rows], F)
    n = len(o)
    out = []
    for tmin in (F(0.001), F(2.0 ** -126)):
        _, t, which, _ = sphere_ref(o, d, c, r, np.full(n, INF), np.full(n, tmin, F))
        root = np.where(which > 0, t, F(1))
        rb = bits(root).astype(np.int64)
        for cl in (np.full(n, INF), root, fl((rb - 1).astype(U)), fl((rb + 1).astype(U)), root * F(0.5), root * F(2)):
            cl = np.where(np.isfinite(cl) & (cl > 0), cl, INF).astype(F)
            out.append((o, d, c, r, cl, np.full(n, tmin, F)))
    return tuple(np.concatenate([p[k] for p in out]) for k in range(6))


# ---- own_box_pass, quad_own_box_pass --------------------------------------------------------------------------------
def new_aabb(a, b):
    return np.minimum(a, b), np.maximum(a, b)


def own_box_ref(o, d, closest, lo, hi):
    nxt = fl(bits(closest) + U(1))
    return aabb_hit(o, d, lo, hi, F(0.001), nxt)


def sphere_box(c, r):
    """NewAabb(c - r, c + r) as NewSphere makes it (hittables.go:85-94)."""
    with np.errstate(all="ignore"):
        return new_aabb(c + (r * F(-1))[:, None], c + r[:, None])


def quad_box(q, u, v):
    """NewAabb(Q, Q + u + v).GetPaddedAabb() (hittables.go:162, bvh.go:28-34, 63-84): axes thinner than 0.0001 padded."""
    eps = F(0.0001)
    lo, hi = new_aabb(q, (q + u) + v)
    thin = (hi - lo) < eps
    return np.where(thin, lo - eps, lo), np.where(thin, hi + eps, hi)


def ownbox_inputs(seed=3, n=1 << 15):
    """Sphere rows (kind 0) and quad rows (kind 1): lattice origins and directions as for the boxes (zero components
    included), +-0 coordinates, zero and negative radii, quads flat on an axis; closest on a 0.125 grid."""
    rng = np.random.default_rng(seed)
    o, d, _, _, closest, _ = box_inputs(seed, 2 * n)
    closest = np.where(np.isfinite(closest), closest, F(3.25)).astype(F)
    c = rng.integers(-4, 5, (n, 3)).astype(F) * F(0.5)
    c = np.where((rng.random((n, 3)) < 0.5) & (c == 0), F(-0.0), c)
    r = rng.choice(np.array([0.0, -0.0, 0.5, 1.0, -0.5, 0.25, 2.0 ** -20, 1.5], F), n)
    d[:n] = np.where(rng.random((n, 1)) < 0.8, (c + rng.integers(-1, 2, (n, 3)).astype(F) * r[:, None]) - o[:n], d[:n])
    q = rng.integers(-4, 5, (n, 3)).astype(F) * F(0.5)
    q = np.where((rng.random((n, 3)) < 0.5) & (q == 0), F(-0.0), q)
    u = rng.integers(-2, 3, (n, 3)).astype(F) * F(0.5)
    v = rng.integers(-2, 3, (n, 3)).astype(F) * F(0.5)
    flat = rng.integers(0, 4, n)  # axis 0..2 flat, 3: a general quad
    for k in range(3):
        u[flat == k, k] = rng.choice(np.array([0.0, -0.0, 2.0 ** -15], F), int((flat == k).sum()))
        v[flat == k, k] = rng.choice(np.array([0.0, -0.0], F), int((flat == k).sum()))
    d[n:] = np.where(rng.random((n, 1)) < 0.8, (q + u * F(0.5) + v * F(0.25)) - o[n:], d[n:])
    return o, d.astype(F), closest, (c, r), (q, u, v)


# ---- go_atan2, go_acos, go_sin, sphere_uv ---------------------------------------------------------------------------
def trig_inputs():
    """(op, a, b) float64 rows: op 0 atan2(a, b), 1 acos(a), 2 sin(a)."""
    rng = np.random.default_rng(21)
    inf, nan = np.inf, np.nan
    sp = [0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 1e-300, -1e-300, 0.66, 2.41421356237309504880, 0.5, 2.0, 1e300]
    rows = [(0.0, y, x) for y in sp for x in sp]
    rows += [(0.0, s * y, -x) for s in (1.0, -1.0) for y in (0.0, 5e-324, 1e-17) for x in (0.0, 1.0, 1e-3, 7.0)]  # the seam
    rows += [(0.0, np.sin(t), np.cos(t)) for t in np.arange(16) * (np.pi / 8)]  # octant boundaries
    rows += [(0.0, y, x) for y, x in rng.normal(size=(1 << 16, 2))]
    rows += [(1.0, x, 0.0) for x in (1.0, -1.0, 0.0, -0.0, 0.7, -0.7, np.nextafter(0.7, 1), 1.0000000001, nan, 0.5, 5e-324)]
    rows += [(1.0, x, 0.0) for x in rng.uniform(-1, 1, 1 << 16)]
    rows += [(2.0, x, 0.0) for x in (0.0, -0.0, inf, nan, np.pi / 4, np.pi / 2, np.pi, 2.0 ** 29, np.nextafter(2.0 ** 29, 0),
                                     1e22, -1e300, 5e-324)]
    rows += [(2.0, x, 0.0) for x in rng.uniform(-40, 40, 1 << 15)]
    rows += [(2.0, x, 0.0) for x in rng.uniform(-1, 1, 1 << 15) * 2.0 ** rng.integers(0, 80, 1 << 15)]
    return pad64(np.array(rows, np.float64), np.array([2.0, 1.0, 0.0]))


def uv_inputs():
    rng = np.random.default_rng(22)
    v = rng.normal(size=(1 << 16, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    sp = [(0, 1, 0), (0, -1, 0), (-1, 0, 0.0), (-1, 0, -0.0), (1, 0, 0), (0, 0, 1), (0, 0, -1), (-1, 0, 1e-30), (-1, 0, -1e-30),
          (0.0, 1, -0.0), (-0.0, -1, 0.0)]
    sp += [(np.cos(t), 0.0, np.sin(t)) for t in np.arange(16) * (np.pi / 8)]
    return pad64(np.concatenate([np.array(sp), v]).astype(F), np.array([1, 0, 0], F))
