#!/usr/bin/env python3
"""Cooperative rounds per shading phase of coop_scatter (csrc/rtx_device.h), replayed on the CPU.

For phases of n owners (Lambertian or Metal hit lanes) with counters drawn from a fixed generator, every owner's first
accepted unit-sphere attempt is found with the oracle's Philox by the RNG contract; then the rounds of
the wave are replayed: the owners still rejecting after the lane's own attempts (`--own`: 1 and 2 are compared) share
the 64 lanes, K = 64 // pending attempts each per round.  Prints one JSON line per n: mean cooperative rounds per
phase, the share of phases that run a second round, mean pending owners after round 0.

The kernel records no hit masks, so n is a parameter here (a full phase of the headline scene has about 36 owners,
§33), not the distribution the render sees.

    python scripts/scatter_rounds.py --owners 24 36 48 64 --phases 2000
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))
import oracle_binding as ob  # noqa: E402

f32 = np.float32


def first_accepted(ctr, key):
    for a in range(1000):
        b = ob.philox((ctr[0], ctr[1], ctr[2], a), key)
        x, y, z = (f32(-1.0) + f32(w >> 8) * f32(2.0 ** -23) for w in b[:3])
        if f32(f32(f32(x * x) + f32(y * y)) + f32(z * z)) < f32(1.0):
            return a
    raise RuntimeError("no accepted attempt")


def rounds(atts, own):
    pend = [a for a in atts if a >= own]
    after0, base, n = len(pend), own, 0
    while pend:
        K = 64 // len(pend)
        pend = [a for a in pend if a >= base + K]
        base += K
        n += 1
    return n, after0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--owners", type=int, nargs="+", default=[36])
    ap.add_argument("--phases", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    key = (args.seed & 0xFFFFFFFF, args.seed >> 32)
    gen = np.random.default_rng(41)
    for n in args.owners:
        res = {1: [], 2: [], 3: []}
        for _ in range(args.phases):
            ctrs = zip(gen.integers(0, 1920 * 1080, n), gen.integers(0, 500, n), gen.integers(1, 8, n))
            atts = [first_accepted((int(p), int(s), int(e)), key) for p, s, e in ctrs]
            for own in res:
                res[own].append(rounds(atts, own))
        line = {"owners": n, "phases": args.phases}
        for own, r in res.items():
            k = np.array([x[0] for x in r])
            line[f"own{own}"] = {"rounds_mean": round(float(k.mean()), 4), "second_round": round(float((k >= 2).mean()), 4),
                                 "pending_after_round0": round(float(np.mean([x[1] for x in r])), 3)}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
