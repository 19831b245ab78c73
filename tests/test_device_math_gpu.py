"""The short float32 forms of csrc/rtx_device.h held to IEEE on their whole domains.

tests/device_math_check.hip includes the header and calls its own functions; it is built here with the library's
flags (as tests/test_coop_scatter_gpu.py builds its checker) and run as a child process, one section per test, so a
failure in one section hides no other.  Every section prints how many cases it checked and the test asserts that number.

Exhaustive sections run all 2^32 bit patterns on the device against the compiler's `1.0f / x` and `__builtin_sqrtf`;
the sampled sections dump raw outputs that are judged here against strict float32 numpy (tests/device_math_ref.py),
which also holds the compiler's two forms themselves on every 257th pattern and around the exponent edges.
tests/test_device_math.py shows on the CPU that the sampled inputs reach the edges.

Left out on purpose: box_hit<*, true> on rays that pass near_fma_ok.  The FMA slab form rounds once where the
reference rounds twice; it is not bit-equal by design (§15.5: the near tree's boxes carry the slack and the hit check
makes the walk exact), and the render tests hold it to the oracle's restatement of it.
"""
import os
import subprocess

import numpy as np
import pytest

import device_math_ref as R
import oracle_binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
TIMEOUT = 120


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("device_math") / "device_math_check")
    # the library's flags (raytracer-go_amd/Makefile): float32 without contraction
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unused-result", "-o", exe, os.path.join(ROOT, "tests", "device_math_check.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def exhaustive(checker, section):
    """{'checked', 'bad', 'first', 'extra'} of an exhaustive section; asserts that nothing failed."""
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=TIMEOUT)
    print(r.stdout.strip())
    w = r.stdout.splitlines()[0].split() if r.stdout else []
    assert r.returncode in (0, 1) and len(w) == 10 and w[0] == section, r.stdout + r.stderr
    res = dict(checked=int(w[2]), bad=int(w[4]), first=int(w[6], 16), extra=(int(w[8]), int(w[9])))
    assert res["bad"] == 0 and r.returncode == 0, f"{section}: {res['bad']} failures, the first at {res['first']:#010x}"
    return res


def sampled(checker, section, tmp_path, rec, out_words):
    """The section's raw output words (n, out_words) for the records rec (n, w) of 32-bit words."""
    rec = np.ascontiguousarray(rec)
    words = rec.view(U).reshape(len(rec), -1)
    assert len(words) % 64 == 0
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    words.tofile(inp)
    r = subprocess.run([checker, section, inp, outp], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [section, "records", str(len(words))], r.stdout
    out = np.fromfile(outp, U)
    os.remove(inp)
    os.remove(outp)
    assert out.size == len(words) * out_words
    return out.reshape(len(words), out_words)


def report(name, ok, *shown):
    """Asserts that every case agrees; a failure shows the first few inputs and outputs as bit patterns."""
    ok = np.asarray(ok)
    bad = np.flatnonzero(~ok)
    print(f"{name}: {ok.size} cases, {bad.size} differ")
    if bad.size:
        def words(a, i):  # floats as their bit patterns
            a = np.atleast_1d(np.asarray(a)[i])
            return [hex(int(w)) for w in (a.view(U) if a.dtype == F else a)]

        first = [(int(i), [words(s, i) for s in shown]) for i in bad[:5]]
        raise AssertionError(f"{name}: {bad.size} of {ok.size} differ; first (index, values): {first}")


# ---- exhaustive, counted on the device ------------------------------------------------------------------------------
def test_rcp_newton_on_its_whole_domain(checker):
    """rcp_fast_ok(x) <=> exponent field in 2..252, and there rcp_newton(x) == 1.0f / x."""
    res = exhaustive(checker, "rcp")
    assert res["checked"] == 1 << 32 and res["extra"] == (0, 2 * 251 << 23)


def test_sqrt_rn_fast_on_its_whole_domain(checker):
    """sqrt_rn_fast(x) == sqrtf(x) wherever sqrt_rn's vote lets it run — |x| >= 2^-96 (negatives: NaN), +-inf, NaN —
    and for -0.  Outside, it does differ: below 2^-96 without the pre-scaling, and on every negative subnormal
    (device_math_ref.NEG_SUBNORMAL), which is why the vote is on |x|."""
    res = exhaustive(checker, "sqrt_fast")
    assert res["checked"] == (1 << 32) - 2 * 0x0F800000 + 1
    assert res["extra"][0] >= (1 << 23) - 1  # the patterns left out that differ: the negative subnormals at the least


def test_sqrt_rn_everywhere(checker):
    """sqrt_rn(x) == sqrtf(x) for all x; the waves of |x| < 2^-96 took the builtin."""
    res = exhaustive(checker, "sqrt_rn")
    assert res["checked"] == 1 << 32 and res["extra"][0] == 2 * 0x0F800000


def test_unit_predicate_and_implied_vote(checker):
    """unit()'s predicate <=> 2^-96 <= q < inf, and there rcp_newton(sqrt_rn_fast(q)) == 1.0f / sqrtf(q): rcp_ieee's
    vote is implied."""
    res = exhaustive(checker, "unit")
    assert res["checked"] == 1 << 32 and res["extra"] == (0, 0x7F800000 - 0x0F800000)


def test_div_by_against_the_division(checker):
    """div_by(n, a, RN(1/a)) == n / a for every normal quotient, a over all 2^23 significands at 41 exponents of
    [-60, 60] with both ends; a non-normal quotient stays non-normal (zero, subnormal, inf or NaN).  The claim holds
    for 2^-102 <= |n| <= 2^65 (rtx_device.h; the sphere test stays inside): the sweep's quotients within 4 ulps of
    2^-126 and of 2^128 that lie outside are counted and printed, not asserted: of 7 960 789 002 such cases 48 937 595
    fail with |n| < 2^-102 and 10 446 020 with |n| > 2^65 (the first at a = 0x21c7f245), which is why the claim, once
    "every normal quotient", and the ray queries' tmin guard, once 2^-126, were narrowed."""
    res = exhaustive(checker, "div")
    inside, outside = res["checked"], res["extra"][1]
    assert inside + outside == 41 * (1 << 23) * (64 + 8 + 18 + 18)
    assert inside >= 41 * (1 << 23) * (64 + 8 + 10)  # the hashed numerators, those near tmin and 1, 5 + 5 at the ends
    assert res["extra"][0] > 1 << 23  # non-normal reference quotients inside the claim


# ---- sampled, judged by numpy ---------------------------------------------------------------------------------------
def test_compiler_division_and_sqrt(checker, tmp_path):
    """What the exhaustive sections lean on: the compiler's 1.0f / x and __builtin_sqrtf(x) against numpy."""
    x = R.forms_inputs()
    assert len(x) >= (1 << 32) // 257 + 2 * 2 * 8 * 100
    out = sampled(checker, "forms", tmp_path, x, 2).view(F)
    xf = x.view(F)
    report("1.0f / x", R.same(out[:, 0], R.rcp_ref(xf)), xf, out[:, 0])
    report("sqrtf(x)", R.same(out[:, 1], R.sqrt_ref(xf)), xf, out[:, 1])


def across(name, got, want, fi, mi, rec):
    report(name + " against numpy", R.same(got, want).reshape(len(got), -1).all(1), rec, got, want)
    report(name + " fast wave against mixed wave", R.same(got[fi], got[mi]).reshape(len(fi), -1).all(1), rec[fi], got[fi], got[mi])


def test_rcp_ieee_across_the_vote(checker, tmp_path):
    rec, fi, mi = R.rcp_vote_inputs()
    out = sampled(checker, "vote", tmp_path, rec, 2).view(F)
    across("rcp_ieee", out[:, :1], R.rcp_ref(rec), fi, mi, rec)


def test_sqrt_rn_across_the_vote(checker, tmp_path):
    rec, fi, mi = R.sqrt_vote_inputs()
    out = sampled(checker, "vote", tmp_path, rec, 2).view(F)
    across("sqrt_rn", out[:, 1:], R.sqrt_ref(rec), fi, mi, rec)


def test_unit_across_the_vote(checker, tmp_path):
    rec, fi, mi = R.unit_vote_inputs()
    out = sampled(checker, "unit3", tmp_path, rec, 3).view(F)
    across("unit", out, R.unit_ref(rec), fi, mi, rec)


@pytest.fixture(scope="module")
def trav_out(checker, tmp_path_factory):
    rec, fi, mi = R.trav_inputs()
    return rec, fi, mi, sampled(checker, "trav", tmp_path_factory.mktemp("trav"), rec, 12)


@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
def test_trav_begin(trav_out, fma):
    """ix, iy, iz, ra, a bit for bit, nx / ny / nz, and `safe` equal to the documented predicate, on directions that
    bracket every guard by one ulp, in whole fast waves and in mixed ones."""
    rec, fi, mi, out = trav_out
    out = out[:, 6:] if fma else out[:, :6]
    inv, ra, a, flags, flags_fma, _ = R.trav_ref(rec[:, :3], rec[:, 3:])
    want = np.concatenate([inv, ra[:, None], a[:, None]], 1)
    across("trav_begin reciprocals and a", out[:, :5].view(F), want, fi, mi, rec)
    want_flags = flags_fma if fma else flags
    report("trav_begin signs", (out[:, 5] & 7) == (want_flags & 7), rec, out[:, 5], want_flags)
    report("trav_begin safe", (out[:, 5] >> 3) == (want_flags >> 3), rec, out[:, 5], want_flags)
    assert np.array_equal(out[fi, 5], out[mi, 5])


@pytest.fixture(scope="module")
def box_out(checker, tmp_path_factory):
    o, d, lo, hi, closest, tmin = R.box_inputs()
    rec = np.concatenate([o, d, lo, hi, closest[:, None], tmin[:, None]], 1).astype(F)
    out = sampled(checker, "box", tmp_path_factory.mktemp("box"), rec, 1)[:, 0]
    ok = R.aabb_hit_detail(o, d, lo, hi, tmin, closest)[0]
    _, _, _, flags, flags_fma, fma_ok = R.trav_ref(o, d)
    return rec, out, ok, (flags >> 3).astype(bool), (flags_fma >> 3).astype(bool), fma_ok


def test_box_hit_predicates(box_out):
    rec, out, ok, safe, safe_fma, fma_ok = box_out
    assert len(rec) == R.BOX_N
    report("safe", (out >> 3 & 1) == safe, rec, out)
    report("safe (FMA)", (out >> 4 & 1) == safe_fma, rec, out)
    report("near_fma_ok", (out >> 5 & 1) == fma_ok, rec, out)


def test_box_hit_select_form(box_out):
    """box_hit<false, false> == Aabb.Hit on every ray of the lattice, NaN slab distances included."""
    rec, out, ok, *_ = box_out
    report("box_hit select", (out & 1) == ok, rec, out, ok)


def test_box_hit_med3_form_on_safe_rays(box_out):
    """box_hit<true, false> == Aabb.Hit on every safe ray: exact ties lo == hi, flat boxes, +-0 faces."""
    rec, out, ok, safe, *_ = box_out
    assert safe.sum() > R.BOX_N // 2
    report("box_hit med3", ((out >> 1 & 1) == ok)[safe], rec[safe], out[safe], ok[safe])


def test_box_hit_fma_select_form_outside_near_fma_ok(box_out):
    """box_hit<false, true> takes the reference's form, ray by ray, where near_fma_ok fails."""
    rec, out, ok, _, _, fma_ok = box_out
    assert (~fma_ok).sum() > 10_000
    report("box_hit FMA select", ((out >> 2 & 1) == ok)[~fma_ok], rec[~fma_ok], out[~fma_ok], ok[~fma_ok])


def test_sphere_test_safe_form(checker, tmp_path):
    """sphere_test<false, true> (div_by) == sphere_test<false, false> (the division) == Sphere.Hit in numpy: the hit
    word and the bits of closest, on tangent rays, origins inside and at the centre, a at both ends of its range,
    closest equal to a root and one ulp either side."""
    o, d, c, r, closest, tmin = R.sphere_inputs()
    rec = np.concatenate([o, d, c, r[:, None], closest[:, None], tmin[:, None]], 1).astype(F)
    rec = R.pad64(rec, rec[0])
    n = len(o)
    out = sampled(checker, "sphere", tmp_path, rec, 5)[:n]
    hit, t, _, _ = R.sphere_ref(o, d, c, r, closest, tmin)
    want_hit = np.where(hit, U(1), U(0xFFFFFFFF))
    assert (out[:, 4] == 1).all()  # every ray is safe
    for name, k in (("div_by", 0), ("division", 2)):
        report(f"sphere_test {name}: hit", out[:, k] == want_hit, rec[:n], out)
        report(f"sphere_test {name}: closest", out[:, k + 1] == R.bits(t), rec[:n], out, t)


def test_own_box_pass(checker, tmp_path):
    """own_box_pass == Aabb.Hit of NewAabb(c - r, c + r), quad_own_box_pass == Aabb.Hit of the padded quad box, on
    [0.001, the float after closest]: zero and negative radii, quads flat on an axis, +-0 coordinates."""
    o, d, closest, (c, r), (q, u, v) = R.ownbox_inputs()
    n = len(c)
    rec = np.zeros((2 * n, 17), F)
    rec[:, :3], rec[:, 3:6], rec[:, 6] = o, d, closest
    rec[:n, 8:11], rec[:n, 11] = c, r
    rec[n:, 8:11], rec[n:, 11:14], rec[n:, 14:17] = q, u, v
    words = rec.view(U).copy()
    words[n:, 7] = 1
    out = sampled(checker, "ownbox", tmp_path, words, 1)[:, 0]
    report("own_box_pass", out[:n] == R.own_box_ref(o[:n], d[:n], closest[:n], *R.sphere_box(c, r)), rec[:n], out[:n])
    report("quad_own_box_pass", out[n:] == R.own_box_ref(o[n:], d[n:], closest[n:], *R.quad_box(q, u, v)), rec[n:], out[n:])


def test_go_trig(checker, tmp_path, built):
    """go_atan2, go_acos, go_sin bit for bit in float64 against the oracle's restatement of Go's."""
    L = ob.load()
    L.oracle_go_atan2.restype = L.oracle_go_acos.restype = ob.ctypes.c_double
    L.oracle_go_atan2.argtypes = [ob.ctypes.c_double] * 2
    L.oracle_go_acos.argtypes = [ob.ctypes.c_double]
    rows = R.trig_inputs()
    out = sampled(checker, "trig", tmp_path, rows, 2).copy().view(np.uint64)[:, 0]
    want = np.array([L.oracle_go_atan2(a, b) if op == 0 else (L.oracle_go_acos(a) if op == 1 else L.oracle_go_sin(a))
                     for op, a, b in rows.tolist()], np.float64)
    for op, name in enumerate(("go_atan2", "go_acos", "go_sin")):
        m = rows[:, 0] == op
        assert m.sum() > 1 << 16
        ok = (out[m] == want[m].view(np.uint64)) | (np.isnan(want[m]) & np.isnan(out[m].view(np.float64)))
        report(name, ok, rows[m].view(np.uint64), out[m])


def test_sphere_uv(checker, tmp_path, built):
    """sphere_uv against hittables.go:122-126 formed from the oracle's Acos / Atan2 and float32 numpy."""
    L = ob.load()
    L.oracle_go_atan2.restype = L.oracle_go_acos.restype = ob.ctypes.c_double
    L.oracle_go_atan2.argtypes = [ob.ctypes.c_double] * 2
    L.oracle_go_acos.argtypes = [ob.ctypes.c_double]
    nrm = R.uv_inputs()
    out = sampled(checker, "uv", tmp_path, nrm, 2).view(F)
    pi32 = F(3.14159274101257324)
    theta = np.array([L.oracle_go_acos(-y) for y in nrm[:, 1].astype(np.float64).tolist()]).astype(F)
    phi = np.array([L.oracle_go_atan2(-z, x) + np.pi for x, z in nrm[:, (0, 2)].astype(np.float64).tolist()]).astype(F)
    with np.errstate(all="ignore"):
        want = np.stack([(phi + F(5) * pi32 / F(12)) / (F(2) * pi32), theta / pi32], 1)
    report("sphere_uv", R.same(out, want).all(1), nrm, out, want)
