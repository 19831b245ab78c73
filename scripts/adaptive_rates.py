#!/usr/bin/env python3
"""What adaptive sampling costs and saves: writes profiles/adaptive_rates.json, which names the library
by hash.

    python scripts/adaptive_rates.py --parent-lib PATH/librtx.so [--variant-lib PATH/librtx.so] [--out ...]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up, ending in a synchronise; the sequence
stops at the first leg that fails.  random_spheres at 1920 x 1080, seed 2024, the library's own trees.
  headline  plain `python bench.py` on this build and on the parent's library (RTX_LIB), alternated, RUNS each; and on
            --variant-lib when given (this commit with the unit claim's indirection behind a runtime test of the
            pointer instead of the template flag).
  nothing   an adaptive pass in which nothing closes (min_samples above the frontier) against rtx_accum_add of the
            same count: 4 passes of 50 each, alternated.
  kernels   rocprofv3 --kernel-trace --stats, a run of its own, of that adaptive sequence: select_tiles and
            accumulate_listed, beside accumulate_samples in the uniform one.
  adaptive  to a frontier of 500 in passes of 50 at two tolerances (min_samples 50), nothing waited for in between: wall
            time from the first enqueue to the final synchronise against uniform 10 x 50, the share of the samples
            rendered, the histogram of n_p.
  rmse      the 240 x 135 window at (840, 560) of the frame, seed 7 (§35's): RMSE against its 1024 spp image of the
            adaptive result at both tolerances and of uniform 500.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))

W, SEED, COUNT, FRONTIER, MIN_SAMPLES = 1920, 2024, 50, 500, 50
TOLERANCES = (0.05, 0.02)
NEVER = 0xFFFFFFFF  # min_samples above any frontier: nothing closes


def setup(window=None, seed=SEED):
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=W, spp=FRONTIER, depth=50)
    dev = rtx.DeviceScene(scene.desc)
    reg = rtx.Region(*(window or (0, 0, cam.image_width, cam.image_height)), 0, 1)
    return torch, rtx, scene, dev, cam, reg, dev.accumulator(cam, seed, reg)


def summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def timed(torch, acc, n, one_pass):
    """A reset, then n passes enqueued back to back on one stream; wall ms from the first enqueue to the synchronise."""
    st = torch.cuda.current_stream().cuda_stream
    acc.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        one_pass(st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def leg_nothing(reps):
    torch, rtx, scene, dev, cam, reg, acc = setup()
    uniform = lambda st: acc.add(COUNT, st)
    adaptive = lambda st: acc.add_adaptive(COUNT, 0.05, NEVER, st, stats=False)
    ms = {"uniform_4x50_ms": [], "adaptive_4x50_ms": []}
    for fn in (uniform, adaptive):  # warm-up: allocations, layouts, code objects
        timed(torch, acc, 4, fn)
    for _ in range(reps):
        ms["uniform_4x50_ms"].append(timed(torch, acc, 4, uniform))
        ms["adaptive_4x50_ms"].append(timed(torch, acc, 4, adaptive))
    out = {k: summary(v) for k, v in ms.items()}
    out["adaptive_over_uniform"] = round(out["adaptive_4x50_ms"]["median"] / out["uniform_4x50_ms"]["median"], 4)
    out["uniform_spread_ms"] = round(max(ms["uniform_4x50_ms"]) - min(ms["uniform_4x50_ms"]), 3)
    a = acc.resolve(0.0)[0]
    timed(torch, acc, 4, uniform)
    out["bit_identical_to_uniform"] = bool((a == acc.resolve(0.0)[0]).all())
    acc.close()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0 if out["bit_identical_to_uniform"] else 1


def leg_trace(reps):
    """The sequences rocprofv3 traces: uniform 4 x 50, then adaptive 4 x 50 with nothing closing."""
    torch, rtx, scene, dev, cam, reg, acc = setup()
    timed(torch, acc, 4, lambda st: acc.add(COUNT, st))
    timed(torch, acc, 4, lambda st: acc.add_adaptive(COUNT, 0.05, NEVER, st, stats=False))
    acc.close()
    rtx.device_check(0)
    return 0


def leg_adaptive(reps):
    import numpy as np

    torch, rtx, scene, dev, cam, reg, acc = setup()
    n = FRONTIER // COUNT
    P = cam.image_width * cam.image_height
    out = {"workload": f"random_spheres:{W}x{cam.image_height}, frontier {FRONTIER} in passes of {COUNT}, "
                       f"min_samples {MIN_SAMPLES}", "reps": reps}
    legs = {"uniform": lambda st: acc.add(COUNT, st)}
    for tol in TOLERANCES:
        legs[f"rel_tol_{tol}"] = lambda st, tol=tol: acc.add_adaptive(COUNT, tol, MIN_SAMPLES, st, stats=False)
    for fn in legs.values():
        timed(torch, acc, n, fn)
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(torch, acc, n, fn))
    base = statistics.median(ms["uniform"])
    for k, fn in legs.items():
        timed(torch, acc, n, fn)
        counts = acc.sample_counts()
        v, c = np.unique(counts, return_counts=True)
        out[k] = {"wall_ms": summary(ms[k]), "over_uniform": round(statistics.median(ms[k]) / base, 4),
                  "share_of_samples": round(float(counts.sum(dtype=np.uint64)) / (P * FRONTIER), 4),
                  "pixels_by_n_p": {int(a): int(b) for a, b in zip(v, c)}}
    acc.close()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def leg_rmse(reps):
    import numpy as np

    window = (840, 560, 240, 135)
    torch, rtx, scene, dev, cam, reg, acc = setup(window, 7)
    st = torch.cuda.current_stream().cuda_stream
    ref = torch.empty((135, 240, 3), dtype=torch.float32, device="cuda")
    dev.render_region(scene.camera(width=W, spp=1024, depth=50), 7, reg, ref.data_ptr(), st)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy().astype(np.float64)
    out = {"window": list(window), "seed": 7, "reference_spp": 1024}
    legs = {"uniform_500": lambda st: acc.add(COUNT, st)}
    for tol in TOLERANCES:
        legs[f"rel_tol_{tol}"] = lambda st, tol=tol: acc.add_adaptive(COUNT, tol, MIN_SAMPLES, st, stats=False)
    for k, fn in legs.items():
        timed(torch, acc, FRONTIER // COUNT, fn)
        rgb = acc.resolve(0.0)[0].astype(np.float64)
        counts = acc.sample_counts()
        out[k] = {"rmse": round(float(np.sqrt(np.mean((rgb - ref) ** 2))), 5),
                  "share_of_samples": round(float(counts.sum(dtype=np.uint64)) / (counts.size * FRONTIER), 4)}
    acc.close()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def kernel_rows(trace_dir):
    """{kernel: (calls, total ns)} of the reductions and the selection from rocprofv3's kernel stats."""
    found = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                for k in ("select_tiles", "accumulate_listed", "accumulate_samples", "render_items", "render_drain"):
                    if k in row["Name"]:
                        c, t = found.get(k, (0, 0))
                        found[k] = (c + int(row["Calls"]), t + int(float(row["TotalDurationNs"])))
    return found


def run(cmd, limit, env=None, log=None):
    """One leg under its own time limit; a limit, a fault or an abort ends the whole sequence."""
    e = dict(os.environ, **(env or {}))
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=e, capture_output=True, text=True)
    if log:
        with open(log, "a") as f:
            f.write(f"$ {' '.join(cmd)}  (rc {r.returncode})\n{r.stdout}\n{r.stderr}\n")
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"leg failed (rc {r.returncode}): {' '.join(cmd)}")
    return r.stdout


def sha16(path):
    import hashlib

    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def last_json(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit("no JSON line in a leg's output")


LEGS = {"nothing": leg_nothing, "trace": leg_trace, "adaptive": leg_adaptive, "rmse": leg_rmse}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--variant-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated: headline, nothing, kernels, adaptive, rmse (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_rates.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "adaptive_rates"),
                    help="where the legs' logs and raw kernel traces go (not kept in git)")
    args = ap.parse_args()
    if args.leg:
        return LEGS[args.leg](args.reps)
    if not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    only = set(filter(None, args.only.split(","))) or {"headline", "nothing", "kernels", "adaptive", "rmse"}
    os.makedirs(args.work, exist_ok=True)
    log = os.path.join(args.work, "legs.log")
    py, me = sys.executable, os.path.abspath(__file__)
    out = {}
    if os.path.exists(args.out):  # (legs measured in an earlier call of the same visit are kept)
        with open(args.out) as f:
            out = json.load(f)
    out["what"] = ("adaptive sampling: headline against the parent, an adaptive pass in which nothing closes against a "
                   "uniform one, the selection and list kernels, adaptive against uniform to 500 samples, RMSE")
    out["librtx_sha256_16"] = {"this": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
                               "parent": sha16(args.parent_lib)}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if "headline" in only:
        libs = [("parent", {"RTX_LIB": os.path.abspath(args.parent_lib)}), ("this", {})]
        if args.variant_lib:
            libs.append(("runtime_test_variant", {"RTX_LIB": os.path.abspath(args.variant_lib)}))
            out["librtx_sha256_16"]["runtime_test_variant"] = sha16(args.variant_lib)
        ms = {who: [] for who, _ in libs}
        for i in range(args.runs):  # alternated, and the order alternates too: drift of the machine hits all alike
            for who, env in (libs if i % 2 == 0 else libs[::-1]):
                ms[who].append(last_json(run([py, "bench.py"], 240, env, log))["ms_per_step"])
        full = last_json(run([py, "bench.py", "--full", "--no-cpu"], 300, None, log))
        spread = max(ms["parent"]) - min(ms["parent"])
        med = {w: statistics.median(v) for w, v in ms.items()}
        out["headline"] = {"ms_per_step": ms, "median": med, "parent_spread_ms": round(spread, 4),
                           "medians_within_the_parents_spread": {w: abs(m - med["parent"]) <= spread
                                                                 for w, m in med.items() if w != "parent"},
                           "framebuffer_sha256_16": full.get("framebuffer_sha256_16")}
        print(json.dumps(out["headline"]), flush=True)
        save()
    for which in ("nothing", "adaptive", "rmse"):
        if which in only:
            out[which] = last_json(run([py, me, "--leg", which, "--reps", str(args.reps)], 400, None, log))
            print(which, json.dumps(out[which]), flush=True)
            save()
    if "kernels" in only:
        d = os.path.join(args.work, "trace")
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
             py, me, "--leg", "trace"], 300, None, log)
        rows = kernel_rows(d)
        if "select_tiles" not in rows or "accumulate_listed" not in rows:
            raise SystemExit(f"the adaptive pass's kernels are not in the kernel trace under {d}: {sorted(rows)}")
        out["kernels"] = {k: {"calls": c, "avg_us": round(ns / c / 1e3, 2), "total_ms": round(ns / 1e6, 3)}
                          for k, (c, ns) in sorted(rows.items())}
        print(json.dumps(out["kernels"]), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
