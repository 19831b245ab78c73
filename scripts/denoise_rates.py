#!/usr/bin/env python3
"""What a denoised preview costs: writes profiles/denoise_rates.json, which names the library by hash.

    python scripts/denoise_rates.py --parent-lib PATH/librtx.so [--out profiles/denoise_rates.json]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up; the sequence stops at the first leg
that fails.  random_spheres at 1920 x 1080, 4 samples, seed 2024, the library's own trees.
  guides    rays per second of the guides kernel (rtx_guide_stats.kernel_ms: HIP events around the launch), its A/B
            knobs alternated in one process: a wave's 64 pixels as 8 x 8 or 64 x 1, the fold threshold at 64, 48, 32
            and 16 parked lanes; beside rtx_trace_device on the very same rays (rtx_camera_rays_device's, sample-major).
  preview   wall time to the first denoised 4-sample preview (a pass of 4, then rtx_accum_preview_device), beside the
            undenoised first image (a pass of 4, then rtx_accum_resolve_device), alternated.
  kernels   rocprofv3 --kernel-trace --stats, a run of its own: the guides kernel, and every level of the filter
            against the bytes it must move: 32 B read (c, v and n, z) + 16 B written per pixel (prepare: 24 B + 16 B
            read, 16 B written; the last level writes 12 B and reads the albedo again), beside a plain copy's 6.3 TB/s.
  headline  plain `python bench.py` on this build and on the parent's library (RTX_LIB), alternated, RUNS each.
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

W, SPP, SEED = 1920, 4, 2024
COPY_TBS = 6.3
VARIANTS = [("8x8_refill48", 3, 48), ("64x1_refill48", 6, 48), ("8x8_refill64", 3, 64), ("8x8_refill32", 3, 32),
            ("8x8_refill16", 3, 16), ("16x4_refill48", 4, 48)]


def setup():
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=W, spp=SPP, depth=50)
    dev = rtx.DeviceScene(scene.desc)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    return torch, rtx, scene, dev, cam, reg


def summary(t):
    return {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def leg_guides(reps):
    torch, rtx, scene, dev, cam, reg = setup()
    P = cam.image_width * cam.image_height
    n = P * SPP
    st = torch.cuda.current_stream().cuda_stream
    guides = torch.empty((P * 32,), dtype=torch.uint8, device="cuda")
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    rtx.camera_rays_device(cam, SEED, reg, 0, SPP, rays.data_ptr(), 0, st)
    flags = rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam))

    def guides_ms(tile, refill):
        os.environ.update(RTX_GUIDES_TILE_W_LOG2=str(tile), RTX_GUIDES_REFILL=str(refill))
        return dev.guides_device(cam, SEED, reg, 0, SPP, guides.data_ptr(), st, stats=True).kernel_ms

    def trace_ms():
        return dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), flags, st, stats=True).kernel_ms

    ms = {name: [] for name, _, _ in VARIANTS}
    ms["trace_same_rays"] = []
    want = None
    for name, tile, refill in VARIANTS:  # warm-up: layouts, code objects; and every variant writes the same bytes
        guides_ms(tile, refill)
        got = guides.clone()
        want = got if want is None else want
        assert torch.equal(got, want), name
    trace_ms()
    for _ in range(reps):
        for name, tile, refill in VARIANTS:
            ms[name].append(guides_ms(tile, refill))
        ms["trace_same_rays"].append(trace_ms())
    for k in ("RTX_GUIDES_TILE_W_LOG2", "RTX_GUIDES_REFILL"):
        os.environ.pop(k, None)
    c = dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), flags | rtx.RTX_TRACE_COUNTERS, st, stats=True)
    out = {"rays": n, "hits": int(c.hits), "node_visits_per_ray": round(c.node_visits / n, 2),
           "prim_tests_per_ray": round(c.prim_tests / n, 2), "scene_placement": int(c.scene_placement)}
    for name, t in ms.items():
        out[name] = {"kernel_ms": summary(t), "Grays_per_s": round(n / statistics.median(t) / 1e6, 3)}
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def leg_preview(reps):
    torch, rtx, scene, dev, cam, reg = setup()
    H = cam.image_height
    st = torch.cuda.current_stream().cuda_stream
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    acc = dev.accumulator(cam, SEED, reg)

    def first(preview):
        acc.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.add(SPP, st)
        if preview:
            acc.preview_device(rgb.data_ptr(), SPP, None, st)
        else:
            acc.resolve_device(rgb.data_ptr(), 0, 0.0, st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def preview_alone():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.preview_device(rgb.data_ptr(), SPP, None, st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):  # warm-up: allocations (the accumulator's preview buffers), layouts, code objects
        first(True)
        first(False)
    ms = {"first_4spp_preview_ms": [], "first_4spp_image_ms": [], "preview_after_the_pass_ms": []}
    for _ in range(reps):
        ms["first_4spp_preview_ms"].append(first(True))
        ms["first_4spp_image_ms"].append(first(False))
        ms["preview_after_the_pass_ms"].append(preview_alone())
    out = {k: summary(v) for k, v in ms.items()}
    out["workload"] = f"random_spheres:{W}x{H}x{SPP}"
    out["finite"] = bool(torch.isfinite(rgb).all())
    acc.close()
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def leg_trace(reps):
    """The sequence rocprofv3 traces: previews of a 4-sample accumulator."""
    torch, rtx, scene, dev, cam, reg = setup()
    st = torch.cuda.current_stream().cuda_stream
    rgb = torch.empty((cam.image_height, W, 3), dtype=torch.float32, device="cuda")
    acc = dev.accumulator(cam, SEED, reg)
    acc.add(SPP, st)
    for _ in range(reps + 2):
        acc.preview_device(rgb.data_ptr(), SPP, None, st)
    torch.cuda.synchronize()
    acc.close()
    rtx.device_check(0)
    return 0


def kernel_times(trace_dir, skip):
    """{kernel: [ns per dispatch, in dispatch order]} of the preview's kernels from rocprofv3's kernel trace, the
    first `skip` previews (warm-up) left out.  The filter's levels are told apart by their order within a preview."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    out, level, previews = {}, 0, 0
    for t0, t1, name in rows:
        if "resolve_accum" in name:  # a preview's first kernel
            key, previews = "resolve_accum", previews + 1
        elif "guide_images" in name:
            key = "guide_images"
        elif "denoise_prepare" in name:
            key, level = "denoise_prepare", 0
        elif "atrous_level" in name:
            key, level = f"atrous_level_{level}", level + 1
        else:
            continue
        if previews > skip:
            out.setdefault(key, []).append(t1 - t0)
    return out


def run(cmd, limit, env=None, log=None):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rates.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "denoise_rates"),
                    help="where the legs' logs and raw kernel traces go (not kept in git)")
    args = ap.parse_args()
    if args.leg:
        return {"guides": leg_guides, "preview": leg_preview, "trace": leg_trace}[args.leg](args.reps)
    if not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    os.makedirs(args.work, exist_ok=True)
    log = os.path.join(args.work, "legs.log")
    py, me = sys.executable, os.path.abspath(__file__)
    parent = {"RTX_LIB": os.path.abspath(args.parent_lib)}
    out = {"what": "denoised previews: the guides kernel against rtx_trace_device on the same rays, the filter's levels "
                   "against their compulsory bytes, the first preview against the first image, headline against the parent",
           "librtx_sha256_16": {"this": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
                                "parent": sha16(args.parent_lib)},
           "copy_TB_per_s": COPY_TBS}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for which in ("guides", "preview"):
        out[which] = last_json(run([py, me, "--leg", which, "--reps", str(args.reps)], 300, None, log))
        print(which, json.dumps(out[which]), flush=True)
        save()
    g = out["guides"]
    g["guides_over_trace"] = {k: round(v["Grays_per_s"] / g["trace_same_rays"]["Grays_per_s"], 3)
                              for k, v in g.items() if isinstance(v, dict) and k != "trace_same_rays"}

    d = os.path.join(args.work, "trace")
    run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
         py, me, "--leg", "trace", "--reps", str(args.reps)], 300, None, log)
    H = W * 9 // 16
    P = W * H
    times = kernel_times(d, 2)
    if "guide_images" not in times or "atrous_level_4" not in times:
        raise SystemExit(f"the preview's kernels are not in the kernel trace under {d}: {sorted(times)}")
    k = {}
    for name, t in sorted(times.items()):
        us = statistics.median(t) / 1e3
        k[name] = {"calls": len(t), "median_us": round(us, 2), "min_us": round(min(t) / 1e3, 2)}
        per_pixel = {"denoise_prepare": 24 + 16 + 16, "resolve_accum": 24 + 24, "guide_images": None}.get(
            name, 32 + 16 + (12 if name == "atrous_level_4" else 0))
        if per_pixel:
            tbs = P * per_pixel / (us * 1e-6) / 1e12
            k[name].update(compulsory_bytes_per_pixel=per_pixel, TB_per_s=round(tbs, 3), share_of_copy=round(tbs / COPY_TBS, 3))
        else:
            k[name]["Grays_per_s"] = round(P * SPP / us / 1e3, 3)
    k["filter_total_us"] = round(sum(v["median_us"] for n, v in k.items() if n.startswith(("denoise", "atrous"))), 2)
    out["kernels"] = k
    print(json.dumps(k), flush=True)
    save()

    ms = {"this": [], "parent": []}
    sha = None
    for i in range(args.runs):  # alternated, and who goes first alternates too: drift of the machine hits both alike
        pair = (("parent", parent), ("this", {}))
        for who, env in (pair if i % 2 == 0 else pair[::-1]):
            ms[who].append(last_json(run([py, "bench.py"], 240, env, log))["ms_per_step"])
    full = last_json(run([py, "bench.py", "--full", "--no-cpu"], 300, None, log))
    sha = full.get("framebuffer_sha256_16")
    lo, hi = min(ms["parent"]), max(ms["parent"])
    med = statistics.median(ms["this"])
    out["headline"] = {"ms_per_step": ms, "median": {w: statistics.median(v) for w, v in ms.items()},
                       "parent_range_ms": [lo, hi], "this_median_inside_the_parents_range": lo <= med <= hi,
                       "this_median_no_slower_than_the_parents_slowest": med <= hi, "framebuffer_sha256_16": sha}
    print(json.dumps(out["headline"]), flush=True)
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
