"""The oracle against an independent float64 reference (tests/ref64.py) — CPU.

Every other correctness test holds the kernel to oracle/oracle.c, which its author also wrote
the kernel from: a shared misreading of the Go source passes them all.  tests/ref64.py is a second
reading (numpy, no BVH, its own Philox), and this file holds the oracle to it on the cases of
tests/ref64_cases.py; tests/test_ref64_gpu.py holds the kernel to it directly.

What is compared, decided from the reference alone:
  - a sample is KEPT when ref64's float32 and float64 runs take the same decisions (primitive,
    root, face, scatter branch, rejection attempts, checker parity, texel, Perlin cells) and meet
    no exact tie between two primitives; the share left out is capped (1 % probes, 3 % scenes);
  - every kept pixel must lie within tol = max(4 * max |ref32 - ref64|, 4 float32 ulps of the
    largest colour) of the float64 colour, and tol itself must not exceed 1e-5;
  - where a case leaves nothing out, segments, hits, rng draws and texel fetches are equal.
The factor 4: the iterative colour order and correctly rounded division / square root against
numpy's each move a colour by about an ulp per operation.  Each case prints its left-out share,
the reference's own spread and tol (pytest -s shows them; DESIGN.md §2 has the table).
"""
import json
import os

import numpy as np
import pytest

import oracle_binding as ob
import ref64
import ref64_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTER_KEYS = ("samples", "segments", "hits", "rng_draws", "texel_fetches")
TOL_MAX = 1e-5


def test_ref64_philox_known_answers():
    """ref64's own Philox4x32-10 against the published Random123 vectors."""
    with open(os.path.join(HERE, "golden", "philox4x32_10_kat.json")) as f:
        kat = json.load(f)
    assert len(kat) >= 3
    for v in kat:
        out = ref64.philox4x32_10(*v["ctr"], *v["key"])
        assert [int(x) for x in out] == v["out"]
    ctr = np.array([v["ctr"] for v in kat], np.uint64)  # vectorised: one block per row
    key = np.array([v["key"] for v in kat], np.uint64)
    out = np.stack(ref64.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    assert out.tolist() == [v["out"] for v in kat]


def test_ref64_is_independent():
    """ref64 computes with numpy alone: it names neither the oracle's binding nor a native library."""
    with open(os.path.join(HERE, "ref64.py")) as f:
        src = f.read()
    for word in ("oracle_binding", "liboracle", "librtxhost", "librtx.so", "CDLL", "load_host", "rtx.load"):
        assert word not in src, word


def check_reference(b):
    """The conditions a case must meet by itself, before anything is compared with it."""
    r = b.ref
    print("\n" + b.report())
    assert r.left_out <= b.cap, f"{b.name}: {r.left_out:.4f} of the samples left out, cap {b.cap}"
    assert r.tol <= TOL_MAX, f"{b.name}: the reference's own spread {r.spread} makes tol {r.tol} > {TOL_MAX}"
    assert r.kept.any()


@pytest.mark.parametrize("order", [ob.ORDER_ITERATIVE, ob.ORDER_REFERENCE], ids=["iterative", "reference"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_against_ref64(built, name, order):
    b = rc.built(name)
    r = b.ref
    check_reference(b)
    img, cnt = ob.render(b.desc, b.cam, b.seed, b.region, order)
    worst = r.worst(img)
    print(f"oracle: max |delta| on kept pixels {worst:.3g}")
    assert np.isfinite(img.reshape(-1, 3)[r.kept]).all()
    assert worst <= r.tol, f"{name}: oracle {worst} from ref64 on a kept pixel, tol {r.tol}"
    if r.left_out == 0:
        want = r.counters()
        assert {k: cnt[k] for k in COUNTER_KEYS} == want


def segments_of(res):
    """The signature as [sample, segment, column] (without the leading disk attempts)."""
    return res.sig[:, 1:].reshape(len(res.sig), -1, ref64.SIG_COLS)


def test_cases_reach_what_they_are_for(built):
    """From the reference alone: each probe takes the path it was made for (a probe that stopped
    reaching its edge would pass for nothing)."""
    seg = lambda n: segments_of(rc.built(n).ref.r64)  # noqa: E731
    first = lambda n: seg(n)[:, 0]  # noqa: E731
    hit = lambda n: first(n)[first(n)[:, 0] >= 0]  # noqa: E731

    assert (hit("sphere_image_outside")[:, 1] == 0).all() and (hit("sphere_image_outside")[:, 2] == 1).all()
    assert (first("sphere_image_inside")[:, 1] == 1).all() and (first("sphere_image_inside")[:, 2] == 0).all()
    assert (first("sphere_image_tmin_r0.01")[:, 1] == 1).all()  # the first root lies below tmin everywhere
    h = hit("sphere_image_tmin_r1000")
    assert (h[:, 1] == 1).sum() > 100 and (h[:, 1] == 0).sum() > 100 and len(h) < len(first("sphere_image_tmin_r1000"))
    assert rc.built("sphere_image_inside").ref.r64.sig[:, 0].max() > 1  # a rejected disk attempt
    for n in ("quad_image_front", "quad_image_back", "quad_image_grazing", "checker_quad"):
        f = first(n)
        assert (f[:, 0] != 0).all(), "the degenerate quad was hit"  # prim 0 = the degenerate quad (no spheres)
        assert (f[:, 0] == 1).sum() >= 20
    assert (hit("quad_image_front")[:, 2] == 1).all() and (hit("quad_image_back")[:, 2] == 0).all()
    for n in ("checker_sphere_r1000", "checker_quad"):
        assert set(np.unique(hit(n)[:, 5])) == {0, 1}
    assert len(np.unique(hit("noise_negative_sphere0.5_quad4")[:, 7])) > 10
    c = rc.built("closest_hit_order").ref
    assert c.r64.tie.any() and c.r32.tie.any() and set(np.unique(first("closest_hit_order")[:, 0])) >= set(range(6))
    branches = lambda n: set(np.unique(seg(n)[:, :, 3])) - {-1}  # noqa: E731
    assert branches("metal_sphere_quad_fuzz") == {ref64.BR_EMIT, ref64.BR_METAL, ref64.BR_ABSORBED}
    assert branches("dielectric_sphere") == {ref64.BR_EMIT, ref64.BR_REFLECT_SCHLICK, ref64.BR_REFRACT}
    glass = {ref64.BR_EMIT, ref64.BR_REFLECT_TIR, ref64.BR_REFLECT_SCHLICK, ref64.BR_REFRACT}
    assert branches("dielectric_sphere_inside") == glass and branches("dielectric_sheet_back") == glass
    crit = rc.built("dielectric_critical_angle").ref
    assert branches("dielectric_critical_angle") == glass
    assert (crit.r32.abs_used & crit.kept).sum() >= 2  # refract's math.Abs decides a kept sample's direction
    assert branches("lambertian_checker") == {ref64.BR_EMIT, ref64.BR_LAMBERT}
    border = 64 * 32  # the environment's border texel (u == 1 past phi = 19 pi / 12)
    assert any((seg(n)[:, :, 6] == border).any() for n in ("lambertian_checker", "dielectric_sheet_back"))
    four = rc.built("random_spheres_24x13x4").ref
    assert four.spp == 4 and np.array_equal(four.kept, four.sample_kept.reshape(-1, 4).all(axis=1))
    assert four.kept.sum() * 4 < four.sample_kept.sum()  # a pixel with one sample left out is left out whole


def test_reference_alone_stays_within_half_the_cap(built):
    """Seeds and geometry are chosen so that ref64's own two precisions leave out at most half of
    what a case may leave out; the kept set is a function of the case alone (a second build of the
    case gives the same one)."""
    for name in rc.NAMES:
        b = rc.built(name)
        assert b.ref.left_out <= b.cap / 2, (name, b.ref.left_out)
    b = rc.built("random_spheres_64x36")
    again = ref64.Case(b.desc, b.cam, b.seed, b.window, b.spp)
    assert np.array_equal(again.kept, b.ref.kept) and again.tol == b.ref.tol and b.ref.left_out > 0
