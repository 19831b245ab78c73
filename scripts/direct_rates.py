#!/usr/bin/env python3
"""What direct light sampling costs and buys: writes profiles/direct_rates.json, which names the
library by hash.

    python scripts/direct_rates.py [--out profiles/direct_rates.json]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up and ending in a synchronise; the
sequence stops at the first leg that fails.  For cornell_box (600 x 600) and simple_light_demo (400 x 225):
  block      rtx_direct_device (rtx_direct_stats.kernel_ms) on the hits of the frame's camera rays, SPP samples a pixel
             (event 1) and on the hits of their bounces (event 2): records per second, and the sampled / visible shares.
  estimator  on a WINDOW x WINDOW window of the frame, against a plain render of REF_SPP samples with another seed:
             the RMSE of the plain render and of wavefront.render(direct=True) at N samples each (equal samples), the
             wall time of both loops and the megakernel's time for the same plain image, and the RMSE of the plain
             megakernel render at the sample count it reaches in the direct loop's time (equal time).
             Its `fused_pass` part is the feature itself: rtx_accum_add_direct beside rtx_accum_add, N samples of the
             WHOLE frame each (kernel time from the passes' stats, alternated, median): ms per sample and their ratio;
             on the window the RMSE of both accumulators' resolved images at N samples, and of a plain accumulator
             at the samples rtx_accum_add reaches in the fused pass's time (N times that ratio): equal time.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))

SCENES = {"cornell_box": 600, "simple_light_demo": 400}
SPP, DEPTH, SEED, REF_SEED = 4, 50, 2024, 77
WINDOW, REF_SPP, N = 64, 16384, 16


def med(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def setup(name):
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene(name, seed=1)
    cam = scene.camera(width=SCENES[name], spp=SPP, depth=DEPTH)
    return torch, rtx, scene, rtx.DeviceScene(scene.desc), cam


def leg_block(name, reps):
    torch, rtx, scene, dev, cam = setup(name)
    st = torch.cuda.current_stream().cuda_stream
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    n = SPP * cam.image_width * cam.image_height
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    keys = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hits = torch.empty((n, 12), dtype=torch.int32, device="cuda")
    bounce = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    light = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    out = {"records": n, "lights": int(len(dev.lights()))}
    rtx.camera_rays_device(cam, SEED, reg, 0, SPP, rays.data_ptr(), keys.data_ptr(), st)
    for event in (1, 2):
        dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), rtx.RTX_TRACE_UV, st)
        dev.shade_device(SEED, rays.data_ptr(), hits.data_ptr(), keys.data_ptr(), n, bounce.data_ptr(), 0, st)
        ms = [dev.direct_device(SEED, hits.data_ptr(), keys.data_ptr(), n, light.data_ptr(), 0, st, stats=True).kernel_ms
              for _ in range(reps + 1)][1:]  # the first is the warm-up
        c = dev.direct_device(SEED, hits.data_ptr(), keys.data_ptr(), n, light.data_ptr(), rtx.RTX_DIRECT_COUNTERS, st,
                              stats=True)
        m = statistics.median(ms)
        out[f"event{event}"] = {"kernel_ms": med(ms), "M_records_per_s": round(n / m / 1e3, 1),
                                "sampled_share": round(c.sampled / n, 4), "visible_share": round(c.visible / n, 4),
                                "rng_draws_per_sampled": round(c.rng_draws / max(c.sampled, 1), 3),
                                "counting_kernel_ms": round(c.kernel_ms, 4)}
        rays = bounce[:, 8:16].contiguous()
        keys[:, 2] += 1
    torch.cuda.synchronize()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def leg_estimator(name, reps):
    torch, rtx, scene, dev, cam = setup(name)
    import wavefront

    st = torch.cuda.current_stream().cuda_stream
    x0, y0 = (cam.image_width - WINDOW) // 2, (cam.image_height - WINDOW) // 2
    reg = rtx.Region(x0, y0, WINDOW, WINDOW, 0, 1)
    img = torch.empty((WINDOW, WINDOW, 3), dtype=torch.float32, device="cuda")

    def plain(spp, seed):
        cam.samples_per_pixel = spp
        s = dev.render_region(cam, seed, reg, img.data_ptr(), st, timed=True)
        torch.cuda.synchronize()
        return img.clone(), s.kernel_ms

    def rmse(a, ref):
        return float(((a.double() - ref.double()) ** 2).mean().sqrt())

    ref, ref_ms = plain(REF_SPP, REF_SEED)
    mega_img, _ = plain(N, SEED)
    mega_ms = [plain(N, SEED)[1] for _ in range(reps)]
    cam.samples_per_pixel = N
    walls = {"plain": [], "direct": []}
    imgs = {}
    for k in range(reps + 1):
        for which in ("plain", "direct"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs[which] = wavefront.render(dev, cam, SEED, reg, compact=True, direct=which == "direct")
            torch.cuda.synchronize()
            if k:
                walls[which].append((time.perf_counter() - t0) * 1e3)
    t_direct, t_mega = statistics.median(walls["direct"]), statistics.median(mega_ms)
    n_equal = max(1, min(REF_SPP // 4, int(N * t_direct / t_mega)))
    eq_img, eq_ms = plain(n_equal, SEED)
    # the fused pass: ms per sample of add_direct beside add on the whole frame; RMSE of both on the window
    full = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    fused_ms, plain_ms = [], []
    for k in range(reps + 1):  # the first is the warm-up
        for which, sink in (("direct", fused_ms), ("plain", plain_ms)):
            acc = dev.accumulator(cam, SEED, full)
            ms = (acc.add_direct(N, st, stats=True) if which == "direct" else acc.add(N, st, stats=True)).kernel_ms
            acc.close()
            if k:
                sink.append(ms)
    t_fused, t_plain = statistics.median(fused_ms), statistics.median(plain_ms)

    def window_image(direct, spp):
        acc = dev.accumulator(cam, SEED, reg)
        (acc.add_direct if direct else acc.add)(spp, st)
        out = torch.from_numpy(acc.resolve()[0]).cuda()
        acc.close()
        return out

    fused_img, add_img = window_image(True, N), window_image(False, N)
    n_fused_eq = max(1, min(REF_SPP // 4, int(round(N * t_fused / t_plain))))
    fused = {"frame": f"{cam.image_width}x{cam.image_height}, depth {DEPTH}", "spp": N,
             "add_direct_kernel_ms": med(fused_ms), "add_kernel_ms": med(plain_ms),
             "ms_per_sample": {"add_direct": round(t_fused / N, 5), "add": round(t_plain / N, 5)},
             "add_direct_over_add": round(t_fused / t_plain, 3),
             "window_rmse": {"add_direct": round(rmse(fused_img, ref), 5), "add": round(rmse(add_img, ref), 5),
                             "largest_add_direct_pixel_value": round(float(fused_img.max()), 3)},
             "equal_time": {"add_spp": n_fused_eq, "rmse_add": round(rmse(window_image(False, n_fused_eq), ref), 5),
                            "rmse_add_direct": round(rmse(fused_img, ref), 5)}}
    # convergence: both estimators again at 16 N samples (an unbiased one's RMSE falls to a quarter; the means agree)
    many_plain, _ = plain(16 * N, SEED)
    cam.samples_per_pixel = 16 * N
    many_direct = wavefront.render(dev, cam, SEED, reg, compact=True, direct=True)
    torch.cuda.synchronize()
    rtx.device_check(0)
    print(json.dumps({
        "window": f"{WINDOW}x{WINDOW} at ({x0}, {y0}) of {cam.image_width}x{cam.image_height}, depth {DEPTH}",
        "reference": {"spp": REF_SPP, "seed": REF_SEED, "megakernel_kernel_ms": round(ref_ms, 3),
                      "mean": round(float(ref.double().mean()), 5)},
        "equal_samples": {"spp": N, "rmse_plain": round(rmse(imgs["plain"], ref), 5),
                          "rmse_plain_megakernel": round(rmse(mega_img, ref), 5),
                          "rmse_direct": round(rmse(imgs["direct"], ref), 5),
                          "mean_plain": round(float(imgs["plain"].double().mean()), 5),
                          "mean_direct": round(float(imgs["direct"].double().mean()), 5),
                          "largest_direct_pixel_value": round(float(imgs["direct"].max()), 3)},
        "sixteen_times_the_samples": {"spp": 16 * N, "rmse_plain": round(rmse(many_plain, ref), 5),
                                      "rmse_direct": round(rmse(many_direct, ref), 5),
                                      "mean_plain": round(float(many_plain.double().mean()), 5),
                                      "mean_direct": round(float(many_direct.double().mean()), 5),
                                      "largest_direct_pixel_value": round(float(many_direct.max()), 3)},
        "fused_pass": fused,
        "ms": {"wavefront_plain_wall": med(walls["plain"]), "wavefront_direct_wall": med(walls["direct"]),
               "megakernel_plain_kernel": med(mega_ms)},
        "equal_time": {"what": "the plain megakernel render at the samples it reaches in the direct loop's wall time "
                               f"(at most {REF_SPP // 4})",
                       "plain_spp": n_equal, "plain_kernel_ms": round(eq_ms, 3), "rmse_plain": round(rmse(eq_img, ref), 5),
                       "rmse_direct": round(rmse(imgs["direct"], ref), 5)}}), flush=True)
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
    ap.add_argument("--leg", nargs=2, default=None, metavar=("KIND", "SCENE"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_rates.json"))
    args = ap.parse_args()
    if args.leg:
        return (leg_block if args.leg[0] == "block" else leg_estimator)(args.leg[1], args.reps)
    py, me = sys.executable, os.path.abspath(__file__)
    out = {"what": "direct light sampling: the block's records per second; wavefront.render(direct=True) against the "
                   "plain render at equal samples and at equal time",
           "librtx_sha256_16": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
           "bytes_per_record": 128, "samples_per_pixel_of_the_block_legs": SPP}
    for name in SCENES:
        out[name] = {"block": run([py, me, "--leg", "block", name, "--reps", str(args.reps)], 240)}
        print(json.dumps(out[name]["block"]), flush=True)
        out[name]["estimator"] = run([py, me, "--leg", "estimator", name, "--reps", "3"], 300)
        print(json.dumps(out[name]["estimator"]), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
