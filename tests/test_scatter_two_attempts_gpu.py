"""coop_scatter's round 0 with two own attempts, and the two-block Philox under it (csrc/rtx_device.h).

tests/scatter_two_attempts_check.hip is built here with hipcc (as tests/test_coop_scatter_gpu.py builds its checker)
and runs one 64-lane wave per case.  Every lane's (x, y, z, attempt, u0, draws) from coop_scatter must equal, bit for
bit, what the scalar loop rand_unit_on_sphere gives on the same counter; the program compares the two itself.  This
test re-derives every lane's attempt, u0 and draws on the CPU from the oracle's Philox, so the two device loops cannot
agree on something wrong.

Every case is CONSTRUCTED: a lane's counter (pixel, sample, event) is searched on the CPU, pixel by pixel from a start
that differs per case and lane, until the lane's first accepted attempt is what the case asks for.  A hit lane evaluates
attempts 0 and 1 itself; the owners (Lambertian or Metal hit lanes) that rejected both share the wave's 64 lanes in
cooperative rounds, K = 64 // pending attempts each, from attempt base = 2 on.  `schedule` replays those rounds on the
CPU and the cases assert the (pending, K, base) sequence they were built for.

The contract (first accepted attempt, u0 = word 0 of block (e, 0), draws = 3 * (attempt + 1)) does not depend on how
many attempts a lane makes itself, so the scatter cases also hold for a coop_scatter with one own attempt.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE, LAMB, METAL, DIEL, LIGHT, QUAD = -1, 0, 1, 2, 3, 4  # QUAD: a quad of a Lambertian material
OWNERS = (LAMB, METAL, QUAD)
SEED = 0x5EED00000000 + 41
KEY = (SEED & 0xFFFFFFFF, SEED >> 32)
OWN = 2  # attempts a hit lane makes itself before the cooperative rounds
f32 = np.float32


def signed_unit(w):  # RandF32N(-1, 1) of a Philox word (rtx_device.h signed_unit)
    return f32(-1.0) + f32(w >> 8) * f32(2.0 ** -24) * f32(2.0)


def attempt(pixel, sample, e, a):
    """(word 0, (x, y, z), accepted) of unit-sphere attempt a: words 0-2 of block (pixel, sample, e, a),
    accepted when lensq < 1 in float32."""
    b = ob.philox((pixel, sample, e, a), KEY)
    x, y, z = signed_unit(b[0]), signed_unit(b[1]), signed_unit(b[2])
    return b[0], (x, y, z), bool(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z)) < f32(1.0))


def first_accepted(pixel, sample, e, limit=200):
    for a in range(limit):
        if attempt(pixel, sample, e, a)[2]:
            return a
    raise AssertionError("no accepted attempt")


def find(ci, lane, want):
    """The lane's counter: the first pixel from the lane's start whose first accepted attempt satisfies `want`."""
    sample, e = (5 * lane + ci) % 11, 1 + (lane + ci) % 6
    for pixel in range(100000 * (ci + 1) + 1000 * lane, 100000 * (ci + 2)):
        # reject early: `want` is a set of attempts or a lower bound
        a = first_accepted(pixel, sample, e)
        if (a in want) if isinstance(want, (set, frozenset)) else a >= want:
            return pixel, sample, e, a
    raise AssertionError("no counter found")


ANY01 = frozenset((0, 1))


def _cases():
    """(name, quads, [(hit, want)] * 64): want = the set of first accepted attempts the lane may have, or a lower
    bound; None for a lane that draws no unit-sphere sample."""
    own = lambda i: (LAMB, METAL)[i & 1]
    c = []
    c.append(("all-accept-0", 0, [(own(i), {0}) for i in range(64)]))
    c.append(("all-accept-1", 0, [(own(i), {1}) for i in range(64)]))
    c.append(("one-pending", 0, [(own(i), 2 if i == 41 else ANY01) for i in range(64)]))
    # all pending, first accepted attempts 2..6 by lane: 64, 51, 38 pending -> K = 1 three times, then K = 2
    c.append(("all-pending", 0, [(own(i), {2 + i % 5}) for i in range(64)]))
    # 9 pending owners (K = 7): lane 3 accepts exactly the second round's first slot, lane 60 exactly attempt 2, the
    # other seven somewhere in the first round; the rest are owners done in round 0 and lanes without a hit
    nine = {3: {2 + 7}, 60: {2}, 9: {3}, 17: {4}, 22: {5}, 30: {6}, 38: {7}, 45: {8}, 52: {2, 3, 4, 5, 6, 7, 8}}
    c.append(("nine-pending", 0, [(own(i), nine[i]) if i in nine else ((own(i), ANY01) if i % 3 else (NONE, None))
                                  for i in range(64)]))
    mix = [(LAMB, {0}), (DIEL, None), (METAL, 2), (NONE, None), (LIGHT, None), (LAMB, {1}), (NONE, None), (METAL, {0}),
           (DIEL, None), (LAMB, 2), (METAL, {1})]
    c.append(("mixed", 0, [mix[i % 11] for i in range(64)]))
    quad = {7: (QUAD, 2)}
    c.append(("quad", 1, [quad.get(i, (own(i), ANY01) if i % 4 else (NONE, None)) for i in range(64)]))
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def lanes(built):
    """Per case and lane: (hit, pixel, sample, e, first accepted attempt or None)."""
    out = []
    for ci, (_, _, spec) in enumerate(CASES):
        row = []
        for lane, (hit, want) in enumerate(spec):
            if want is None:
                row.append((hit, 7000 + 64 * ci + lane, lane % 5, 1 + lane % 3, None))
            else:
                row.append((hit,) + find(ci, lane, want))
        out.append(row)
    return out


def schedule(atts):
    """The cooperative rounds of a wave whose owners' first accepted attempts are `atts`: [(pending, K, base)]."""
    pend = sorted(a for a in atts if a >= OWN)
    base, rounds = OWN, []
    while pend:
        K = 64 // len(pend)
        rounds.append((len(pend), K, base))
        pend = [a for a in pend if a >= base + K]
        base += K
    return rounds


def test_cases_are_what_they_claim(lanes):
    att = {name: [l[4] for l in lanes[ci] if l[4] is not None] for ci, (name, _, _) in enumerate(CASES)}
    assert len(att["all-accept-0"]) == 64 and set(att["all-accept-0"]) == {0} and schedule(att["all-accept-0"]) == []
    assert len(att["all-accept-1"]) == 64 and set(att["all-accept-1"]) == {1} and schedule(att["all-accept-1"]) == []
    one = att["one-pending"]
    assert len(one) == 64 and sum(a >= 2 for a in one) == 1 and lanes[2][41][4] >= 2
    assert schedule(one)[0] == (1, 64, 2)
    allp = att["all-pending"]
    assert len(allp) == 64 and min(allp) == 2
    assert schedule(allp)[:4] == [(64, 1, 2), (51, 1, 3), (38, 1, 4), (25, 2, 5)]
    nine = att["nine-pending"]
    assert schedule(nine) == [(9, 7, 2), (1, 64, 9)]
    ci = [n for n, _, _ in CASES].index("nine-pending")
    assert lanes[ci][3][4] == 2 + 7 and lanes[ci][60][4] == 2
    ci = [n for n, _, _ in CASES].index("mixed")
    hits = [l[0] for l in lanes[ci]]
    assert {NONE, DIEL, LIGHT, LAMB, METAL} == set(hits)
    assert {0, 1} < set(att["mixed"]) and max(att["mixed"]) >= 2
    ci = [n for n, _, _ in CASES].index("quad")
    assert [l[0] for l in lanes[ci]].count(QUAD) == 1 and lanes[ci][7][4] >= 2 and CASES[ci][1] == 1


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("scatter2") / "scatter_two_attempts_check")
    # the library's flags (raytracer-go_amd/Makefile): the acceptance test is float32 without contraction
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unused-result", "-o", exe, os.path.join(ROOT, "tests", "scatter_two_attempts_check.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_two_attempts_equal_the_scalar_loop(checker, lanes, tmp_path):
    inp = tmp_path / "cases.txt"
    lines = [f"{SEED} {len(CASES)}"]
    for ci, (_, quads, _) in enumerate(CASES):
        lines.append(str(quads))
        lines += ["%d %d %d %d" % l[:4] for l in lanes[ci]]
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([checker, "scatter", str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(rows) == 64 * len(CASES)
    for ci, lane, hit, x, y, z, att, u0, draws in rows:
        ci, lane = int(ci), int(lane)
        ehit, pixel, sample, e, eatt = lanes[ci][lane]
        name = f"{CASES[ci][0]} lane {lane}"
        assert int(hit) == ehit, name
        if ehit == NONE:  # draws nothing
            assert (int(u0, 16), int(att), int(draws)) == (0, -1, 0) and (x, y, z) == ("00000000",) * 3, name
            continue
        assert int(u0, 16) == attempt(pixel, sample, e, 0)[0], name  # word 0 of the lane's own block (e, 0)
        if ehit not in OWNERS:  # Dielectric, light: u0 and no unit-sphere draw
            assert (int(att), int(draws)) == (-1, 0) and (x, y, z) == ("00000000",) * 3, name
            continue
        assert int(att) == eatt and int(draws) == 3 * (eatt + 1), name
        v = np.array([int(x, 16), int(y, 16), int(z, 16)], np.uint32).view(np.float32).astype(np.float64)
        w = np.array(attempt(pixel, sample, e, eatt)[1], np.float64)  # the accepted attempt, normalised
        assert np.abs(v - w / np.sqrt((w * w).sum())).max() < 1e-6, name


def philox_blocks():
    """16 waves of 64 counter pairs (c0, c1, c2, c3 / c3b), one key per wave.  The Random123 known-answer vectors are
    lane 0 of the first waves, under their own keys; then the render's shape (c3 = 0, c3b = 1), equal counters, and
    counters drawn from a fixed generator."""
    kats = json.load(open(os.path.join(GOLDEN, "philox4x32_10_kat.json")))
    rng = np.random.default_rng(41)
    blocks = []
    for b in range(16):
        key = tuple(kats[b]["key"]) if b < len(kats) else tuple(int(v) for v in rng.integers(0, 2 ** 32, 2))
        rows = []
        for lane in range(64):
            c = [int(v) for v in rng.integers(0, 2 ** 32, 5)]
            if b < len(kats) and lane == 0:
                c = list(kats[b]["ctr"]) + [kats[b]["ctr"][3] ^ 1]
            elif lane % 4 == 1:  # the scatter's counters: (pixel, sample, event, 0 / 1)
                c = [c[0] % (1920 * 1080), c[1] % 500, 1 + c[2] % 50, 0, 1]
            elif lane % 4 == 2:  # both chains on one counter
                c[4] = c[3]
            elif lane % 16 == 3:  # all-ones words: the widest products and carries
                c = [0xFFFFFFFF] * 4 + [0]
            rows.append(c)
        blocks.append((key, rows))
    return kats, blocks


def test_philox_x2_equals_two_calls(checker, built, tmp_path):
    kats, blocks = philox_blocks()
    assert len(kats) >= 1 and len(blocks) == 16
    inp = tmp_path / "philox.txt"
    lines = [str(len(blocks))]
    for key, rows in blocks:
        lines.append("%d %d" % key)
        lines += ["%d %d %d %d %d" % tuple(c) for c in rows]
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([checker, "philox", str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr  # x2 against two calls of philox4x32_10, word for word
    rows = [ln.split() for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(rows) == 64 * len(blocks)
    for row in rows:
        b, lane = int(row[0]), int(row[1])
        got = [int(w, 16) for w in row[2:10]]
        key, c = blocks[b][0], blocks[b][1][lane]
        assert got[:4] == ob.philox(c[:4], key), (b, lane)
        assert got[4:] == ob.philox(c[:3] + [c[4]], key), (b, lane)
        if b < len(kats) and lane == 0:
            assert got[:4] == kats[b]["out"], b
