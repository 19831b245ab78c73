#!/usr/bin/env python3
"""What progressive rendering costs: writes profiles/accum_passes.json.

    python scripts/accum_passes.py --parent-lib PATH/librtx.so [--out profiles/accum_passes.json]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up, ending in a synchronise; the
sequence stops at the first leg that fails.
  headline  plain `python bench.py` on this build and on the parent's library (RTX_LIB), alternated, RUNS each:
            ms_per_step of both, the parent's spread, and the frame hash of `bench.py --full --no-cpu`.
  passes    1920x1080 random_spheres: 500 spp as one shot, as 10 x 50 and as 125 x 4 passes with a
            resolve_device after every pass; the time to the first resolved 4 spp image.
  kernels   a `rocprofv3 --kernel-trace --stats` run of the 125 x 4 and the 10 x 50 sequence each: the time of
            accumulate_samples and resolve_accum, and their bytes per second from the shapes (12 B per sample and
            48 B per slot per chunk; 24 B in and 12 B out per pixel).
The legs (`--leg passes`, `--leg trace N COUNT`) are this file run again.
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

W, SPP, SEED = 1920, 500, 2024
HBM_PEAK = 8.0e12  # B/s, the MI355X's HBM3E specification (6.3e12 achievable by a copy)


def scene_and_camera():
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=W, spp=SPP, depth=50)
    dev = rtx.DeviceScene(scene.desc)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    return torch, rtx, scene, dev, cam, reg


def run_passes(torch, acc, n, count, rgb, resolve=True):
    """n passes of count samples, a resolve_device after each, all enqueued on one stream; wall ms to the end."""
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        acc.add(count, st)
        if resolve:
            acc.resolve_device(rgb.data_ptr(), 0, 0.0, st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def leg_passes(reps):
    torch, rtx, scene, dev, cam, reg = scene_and_camera()
    H = cam.image_height
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    acc = dev.accumulator(cam, SEED, reg)
    out = {"workload": f"random_spheres:{W}x{H}x{SPP}", "reps": reps}

    def one_shot():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.render_region(cam, SEED, reg, rgb.data_ptr(), st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def first_image():
        acc.reset()
        return run_passes(torch, acc, 1, 4, rgb)

    def split(n, count):
        acc.reset()
        return run_passes(torch, acc, n, count, rgb)

    legs = {"one_shot_ms": one_shot, "passes_10x50_ms": lambda: split(10, 50), "passes_125x4_ms": lambda: split(125, 4),
            "first_4spp_image_ms": first_image}
    for fn in legs.values():  # warm-up: allocations, layouts, code objects
        fn()
    for name, fn in legs.items():
        t = [fn() for _ in range(reps)]
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    base = out["one_shot_ms"]["median"]
    for name in ("passes_10x50_ms", "passes_125x4_ms"):
        out[name]["over_one_shot"] = round(out[name]["median"] / base, 4)
    # the same bits either way
    acc.reset()
    run_passes(torch, acc, 125, 4, rgb)
    a = rgb.clone()
    dev.render_region(cam, SEED, reg, rgb.data_ptr(), st)
    torch.cuda.synchronize()
    out["bit_identical_to_one_shot"] = bool(torch.equal(a, rgb))
    acc.close()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0 if out["bit_identical_to_one_shot"] else 1


def leg_trace(n, count):
    """The sequence rocprofv3 traces: n passes of count samples with a resolve after each."""
    torch, rtx, scene, dev, cam, reg = scene_and_camera()
    rgb = torch.empty((cam.image_height, W, 3), dtype=torch.float32, device="cuda")
    acc = dev.accumulator(cam, SEED, reg)
    run_passes(torch, acc, n, count, rgb)
    acc.close()
    rtx.device_check(0)
    return 0


def run(cmd, limit, env=None, log=None):
    """One leg under its own time limit; (rc, stdout).  A limit, a fault or an abort ends the whole sequence."""
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


def kernel_rows(trace_dir):
    """{kernel name prefix: (calls, total ns)} of the two new kernels from rocprofv3's kernel stats."""
    found = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                for k in ("accumulate_samples", "resolve_accum", "render_items", "render_drain"):
                    if k in row["Name"]:
                        c, t = found.get(k, (0, 0))
                        found[k] = (c + int(row["Calls"]), t + int(float(row["TotalDurationNs"])))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs="+", default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_passes.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "accum_passes"),
                    help="where the legs' logs and raw kernel traces go (not kept in git)")
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] == "passes":
            return leg_passes(args.reps)
        return leg_trace(int(args.leg[1]), int(args.leg[2]))
    if not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    os.makedirs(args.work, exist_ok=True)
    log = os.path.join(args.work, "legs.log")
    py, me = sys.executable, os.path.abspath(__file__)
    out = {"what": "progressive rendering: headline against the parent, cost of passes, the two new kernels"}

    out["librtx_sha256_16"] = {"this": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
                               "parent": sha16(args.parent_lib)}
    ms = {"this": [], "parent": []}
    for _ in range(args.runs):  # alternated: drift of the machine hits both alike
        for who, env in (("parent", {"RTX_LIB": os.path.abspath(args.parent_lib)}), ("this", {})):
            j = last_json(run([py, "bench.py"], 240, env, log))
            ms[who].append(j["ms_per_step"])
    full = last_json(run([py, "bench.py", "--full", "--no-cpu"], 300, None, log))
    spread = max(ms["parent"]) - min(ms["parent"])
    out["headline"] = {
        "ms_per_step": ms, "median": {k: statistics.median(v) for k, v in ms.items()},
        "parent_spread_ms": round(spread, 4),
        "no_worse_than_parent_beyond_its_spread": statistics.median(ms["this"]) <= statistics.median(ms["parent"]) + spread,
        "framebuffer_sha256_16": full.get("framebuffer_sha256_16"),
        # bench.py ties the committed PMC summaries to the library they were measured on, by hash
        "roofline_stale": (full.get("roofline") or {}).get("stale"),
    }
    print(json.dumps(out["headline"]), flush=True)

    out["passes"] = last_json(run([py, me, "--leg", "passes", "--reps", str(args.reps)], 300, None, log))
    print(json.dumps(out["passes"]), flush=True)

    H = W * 9 // 16
    pixels = W * H
    slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
    out["kernels"] = {}
    for n, count in ((125, 4), (10, 50)):
        d = os.path.join(args.work, f"trace_{n}x{count}")
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
             py, me, "--leg", "trace", str(n), str(count)], 300, None, log)
        rows = kernel_rows(d)
        k = {}
        for name, per_call in (("accumulate_samples", slots * (12 * count + 48)), ("resolve_accum", pixels * 36)):
            calls, ns = rows.get(name, (0, 0))
            if not calls:
                raise SystemExit(f"{name} not in the kernel trace under {d}")
            us = ns / calls / 1e3
            bps = per_call / (ns / calls * 1e-9)
            k[name] = {"calls": calls, "avg_us": round(us, 2), "bytes_per_call": per_call,
                       "TB_per_s": round(bps / 1e12, 3), "share_of_hbm_peak": round(bps / HBM_PEAK, 3)}
        render_ns = sum(rows.get(r, (0, 0))[1] for r in ("render_items", "render_drain"))
        k["render_kernels_ms_total"] = round(render_ns / 1e6, 3)
        k["new_kernels_ms_total"] = round(sum(rows[r][1] for r in ("accumulate_samples", "resolve_accum")) / 1e6, 3)
        out["kernels"][f"{n}x{count}"] = k
    print(json.dumps(out["kernels"]), flush=True)

    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
