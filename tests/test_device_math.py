"""The inputs of tests/test_device_math_gpu.py, judged on the CPU by the numpy references alone (device_math_ref):
they reach the ties, the NaN rule, every outcome of the sphere test and both sides of every vote, and the references
agree with float64.  A later change of a generator or a seed cannot quietly stop reaching those cases."""
from fractions import Fraction

import numpy as np

import device_math_ref as R

F = np.float32


def box_safe(o, d):
    _, _, _, flags, flags_fma, fma_ok = R.trav_ref(o, d)
    return (flags >> 3 & 1).astype(bool), fma_ok


def test_box_inputs_reach_ties_and_the_nan_rule():
    o, d, lo, hi, closest, tmin = R.box_inputs()
    safe, fma_ok = box_safe(o, d)
    ok, before_last, l, h = R.aabb_hit_detail(o, d, lo, hi, tmin, closest)
    n_safe = int(safe.sum())
    share = ok[safe].mean()
    ties = int((safe & before_last & (l == h)).sum())
    plain = R.box_med3_plain(o, d, lo, hi, closest, tmin)
    nan_rule = int((~safe & (plain != ok)).sum())
    print(f"boxes: {len(o)} cases, {n_safe} safe of which {share:.1%} pass, {ties} exact ties on the last axis; "
          f"{int((~safe).sum())} not safe, plain median differs on {nan_rule}; {int((~fma_ok).sum())} fail near_fma_ok")
    assert 0.05 < share < 0.95
    assert ties >= 10_000
    assert nan_rule >= 1_000
    assert not (plain != ok)[safe].any()  # on safe rays the clamps are the reference (the claim under test)
    assert (~fma_ok & safe).sum() >= 1_000 and (~fma_ok & ~safe).sum() >= 1_000
    for t in (0.001, 2.0 ** -126, 0.5):
        assert (tmin == F(t)).sum() > len(o) // 4


def test_sphere_inputs_reach_every_outcome():
    o, d, c, r, closest, tmin = R.sphere_inputs()
    safe, _ = box_safe(o, d)
    assert safe.all()
    hit, t, which, disc = R.sphere_ref(o, d, c, r, closest, tmin)
    counts = {k: int((which == k).sum()) for k in (1, 2, -1, -2, 0)}
    print(f"spheres: {len(o)} cases, outcomes {counts}, disc == 0 on {int((disc == 0).sum())}")
    for k in (1, 2, -1, -2):
        assert counts[k] >= 1_000, (k, counts)
    assert (disc == 0).sum() >= 100  # tangent rays
    a = R.lensq_ref(d)
    assert (a == F(2.0 ** -60)).sum() >= 100 and (a == F(2.0 ** 60)).sum() >= 100
    assert ((closest == t) & ~hit & (which == -2)).sum() >= 100  # closest equal to a root: a strict miss
    assert set(np.unique(np.log2(r[np.log2(r) % 1 == 0]))) >= {-20.0, 20.0}
    assert (np.abs(o - c).max(1) == 0).sum() >= 10  # origins at the centre
    for tm in (0.001, 2.0 ** -126):
        assert (tmin == F(tm)).sum() == len(o) // 2


def test_every_vote_has_whole_and_mixed_waves():
    rec, _, _ = R.rcp_vote_inputs()
    kinds = R.wave_kinds(R.rcp_fast_pred(rec[:, 0]))
    assert min(kinds) >= 3, kinds
    rec, _, _ = R.sqrt_vote_inputs()
    kinds = R.wave_kinds(~R.sqrt_slow_pred(rec[:, 0]))
    assert min(kinds) >= 3, kinds
    rec, _, _ = R.unit_vote_inputs()
    kinds = R.wave_kinds(R.unit_fast_pred(R.lensq_ref(rec)))
    assert min(kinds) >= 3, kinds
    rec, fi, mi = R.trav_inputs()
    pred = R.trav_fast_pred(rec[:, 3:])
    kinds = R.wave_kinds(pred)
    assert min(kinds) >= 3, kinds
    assert pred[fi].all() and np.array_equal(rec[fi].view(np.uint32), rec[mi].view(np.uint32))


def test_trav_inputs_bracket_every_guard():
    rec, fi, _ = R.trav_inputs()
    o, d = rec[:, :3], rec[:, 3:]
    inv, ra, a, flags, flags_fma, fma_ok = R.trav_ref(o, d)
    safe, safe_fma = flags >> 3 & 1, flags_fma >> 3 & 1
    assert safe.sum() > 1000 and (1 - safe).sum() > 1000 and (safe & ~safe_fma & 1).sum() > 100
    for edge in (2.0 ** -60, 2.0 ** 60):
        for x in R.near(edge):
            assert (a == x).sum() >= 3, x  # below, at and just above the edge
    for x in R.near(2.0 ** 32):
        assert (np.abs(o) == x).any(), x
    # 1/d at 2^64, just above it, and the closest a reciprocal comes from below (1 / next(2^-64), two ulps under)
    for x in (F(2.0 ** 64), R.near(2.0 ** 64)[2], F(1) / R.near(2.0 ** -64)[2]):
        assert (np.abs(inv) == x).any(), x
    # safe hangs on a alone, on 1/d alone and on the origin alone somewhere
    a_ok = (a >= F(2.0 ** -60)) & (a <= F(2.0 ** 60))
    fin = np.isfinite(inv).all(1)
    ofin = np.isfinite(o).all(1)
    assert (~a_ok & fin & ofin).sum() >= 10 and (a_ok & ~fin & ofin).sum() >= 10 and (a_ok & fin & ~ofin).sum() >= 10


def test_own_box_inputs_pass_and_fail():
    o, d, closest, (c, r), (q, u, v) = R.ownbox_inputs()
    n = len(c)
    s = R.own_box_ref(o[:n], d[:n], closest[:n], *R.sphere_box(c, r))
    qq = R.own_box_ref(o[n:], d[n:], closest[n:], *R.quad_box(q, u, v))
    for m in (s, qq, s[r <= 0], qq[((R.quad_box(q, u, v)[1] - R.quad_box(q, u, v)[0]) < F(0.00021)).any(1)]):
        assert m.sum() >= 500 and (~m).sum() >= 500, (m.sum(), len(m))


def as_fraction(x):
    return Fraction(float(x))


def round_to_f32(fr):
    """A rational correctly rounded to float32 (through a float64 is not enough in general: directly)."""
    if fr == 0:
        return F(0)
    sign = -1 if fr < 0 else 1
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    q = fr / Fraction(2) ** (e - 23)  # the significand in units of the last place
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    v = sign * n * 2.0 ** (e - 23)
    return F(np.inf) * sign if abs(v) >= 2.0 ** 128 else F(v)


def test_numpy_references_agree_with_float64():
    """1 / x in exact rationals rounded once, and sqrt in float64 rounded once (a float64 square root of a float32 is
    never close enough to a float32 tie to round twice), on the edge lists."""
    xs = np.concatenate([R.DIR_LIST, R.ORIGIN_LIST, R.near(2.0 ** -96, 3), R.near(2.0 ** -60, 3), R.near(2.0 ** 60, 3),
                         R.fl([1, 2, 3, 0x007FFFFF, 0x00800001, 0x7F7FFFFF]), R.forms_inputs()[-2200:].view(F)])
    xs = xs[np.isfinite(xs) & (xs != 0)]
    got = R.rcp_ref(xs)
    for x, g in zip(xs, got):
        want = round_to_f32(1 / as_fraction(x))
        assert R.bits(want) == R.bits(g), (x, g, want)
    pos = np.abs(xs)
    with np.errstate(all="ignore"):
        assert (R.bits(R.sqrt_ref(pos)) == R.bits(np.sqrt(pos.astype(np.float64)).astype(F))).all()
    # a few quotients as the sphere and box references form them
    rng = np.random.default_rng(1)
    n_, a_ = R.fl(rng.integers(0x30000000, 0x4F000000, 2000)), R.fl(rng.integers(0x30000000, 0x4F000000, 2000))
    for n1, a1, g in zip(n_, a_, n_ / a_):
        assert R.bits(round_to_f32(as_fraction(n1) / as_fraction(a1))) == R.bits(g)
