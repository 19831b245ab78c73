#!/usr/bin/env python3
"""What multiple importance sampling of the direct light costs and buys: writes
profiles/mis_rates.json, which names the library by hash.

    python scripts/mis_rates.py [--out profiles/mis_rates.json]

One GPU visit, every scene a process of its own under its own `timeout`, warmed up and ending in a synchronise; the
sequence stops at the first leg that fails.  For cornell_box (600 x 600) and simple_light_demo (400 x 225), with
scripts/direct_rates.py's window, reference and seeds:
  rmse        on the WINDOW x WINDOW window of the frame, against a plain render of REF_SPP samples with another seed:
              the RMSE and the largest pixel value of rtx_accum_add, rtx_accum_add_direct and rtx_accum_add_mis at 16
              and at 256 samples each (equal samples).
  time        the three passes on the WHOLE frame, N samples each (kernel time from the passes' stats, alternated,
              median of `reps`): ms per sample and the ratios.
  equal_time  the RMSE of a plain accumulator at the samples rtx_accum_add reaches in the MIS pass's time (N times the
              ratio) beside the MIS accumulator's at N.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))

SCENES = {"cornell_box": 600, "simple_light_demo": 400}
DEPTH, SEED, REF_SEED = 50, 2024, 77
WINDOW, REF_SPP, N, MANY = 64, 16384, 16, 256
PASSES = ("add_mis", "add_direct", "add")


def med(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def leg(name, reps):
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene(name, seed=1)
    cam = scene.camera(width=SCENES[name], spp=N, depth=DEPTH)
    dev = rtx.DeviceScene(scene.desc)
    st = torch.cuda.current_stream().cuda_stream
    x0, y0 = (cam.image_width - WINDOW) // 2, (cam.image_height - WINDOW) // 2
    reg = rtx.Region(x0, y0, WINDOW, WINDOW, 0, 1)
    full = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    img = torch.empty((WINDOW, WINDOW, 3), dtype=torch.float32, device="cuda")
    cam.samples_per_pixel = REF_SPP
    ref_ms = dev.render_region(cam, REF_SEED, reg, img.data_ptr(), st, timed=True).kernel_ms
    torch.cuda.synchronize()
    ref = img.double().cpu().numpy()
    cam.samples_per_pixel = N

    def window_image(which, spp):
        acc = dev.accumulator(cam, SEED, reg)
        getattr(acc, which)(spp, st)
        out = acc.resolve()[0].astype("float64")
        acc.close()
        return out

    def rmse(a):
        return float((((a - ref) ** 2).mean()) ** 0.5)

    table = {}
    for spp in (N, MANY):
        row = {}
        for which in PASSES:
            a = window_image(which, spp)
            row[which] = {"rmse": round(rmse(a), 5), "largest_pixel_value": round(float(a.max()), 3),
                          "mean": round(float(a.mean()), 5)}
        table[str(spp)] = row
    ms = {which: [] for which in PASSES}
    for k in range(reps + 1):  # the first round is the warm-up
        for which in PASSES:
            acc = dev.accumulator(cam, SEED, full)
            t = getattr(acc, which)(N, st, stats=True).kernel_ms
            acc.close()
            if k:
                ms[which].append(t)
    t = {which: statistics.median(ms[which]) for which in PASSES}
    n_eq = max(1, min(REF_SPP // 4, int(round(N * t["add_mis"] / t["add"]))))
    torch.cuda.synchronize()
    rtx.device_check(0)
    print(json.dumps({
        "window": f"{WINDOW}x{WINDOW} at ({x0}, {y0}) of {cam.image_width}x{cam.image_height}, depth {DEPTH}",
        "reference": {"spp": REF_SPP, "seed": REF_SEED, "megakernel_kernel_ms": round(ref_ms, 3),
                      "mean": round(float(ref.mean()), 5)},
        "equal_samples": table,
        "time": {"frame": f"{cam.image_width}x{cam.image_height}, depth {DEPTH}", "spp": N, "reps": reps,
                 "kernel_ms": {which: med(ms[which]) for which in PASSES},
                 "ms_per_sample": {which: round(t[which] / N, 5) for which in PASSES},
                 "add_mis_over_add_direct": round(t["add_mis"] / t["add_direct"], 4),
                 "add_mis_over_add": round(t["add_mis"] / t["add"], 3)},
        "equal_time": {"what": "a plain accumulator at the samples rtx_accum_add reaches in the MIS pass's time",
                       "add_spp": n_eq, "rmse_add": round(rmse(window_image("add", n_eq)), 5),
                       "rmse_add_mis": table[str(N)]["add_mis"]["rmse"]}}), flush=True)
    return 0


def run(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"leg failed (rc {r.returncode}): {' '.join(cmd)}")
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit("no JSON line in a leg's output")


def sha16(path):
    import hashlib

    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, metavar="SCENE")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mis_rates.json"))
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args.reps)
    py, me = sys.executable, os.path.abspath(__file__)
    out = {"what": "multiple importance sampling of the direct light: rtx_accum_add_mis beside rtx_accum_add_direct and "
                   "rtx_accum_add at equal samples, their pass times, and MIS against the plain pass at equal time",
           "librtx_sha256_16": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so"))}
    for name in SCENES:
        out[name] = run([py, me, "--leg", name, "--reps", str(args.reps)], 300)
        print(json.dumps(out[name]), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
