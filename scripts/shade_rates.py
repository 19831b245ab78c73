#!/usr/bin/env python3
"""What the path building blocks cost: writes profiles/shade_rates.json, which names the library by hash.

    python scripts/shade_rates.py --parent-lib PATH/librtx.so [--out profiles/shade_rates.json]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up and ending in a synchronise; the
sequence stops at the first leg that fails.
  blocks    random_spheres' camera at 1920x1080, 8 samples: rtx_camera_rays_device (HIP events around the call), and
            rtx_shade_device (rtx_shade_stats.kernel_ms) on the hits of those rays (event 1) and on the hits of their
            bounce rays (event 2: materials and misses mixed within the waves).
  kernels   the same sequence under `rocprofv3 --kernel-trace --stats`, a run of its own: the kernels' own durations.
            48 B per camera ray (32 + 16 out) and 160 B per shade record (32 + 48 + 16 in, 64 out) over that time,
            against the 6.3 TB/s a plain copy reaches on this part and the 8 TB/s HBM specification.
  loop      wavefront.render(compact=True) of the frame at depth 50 beside rtx_render_region_device: how much the
            megakernel buys (default scene, the pixels that differ counted).  On the caller's tree with every box
            test the two images must be equal bit for bit, or the leg fails.
  headline  plain `python bench.py` on this build and on the parent's library (RTX_LIB), alternated, RUNS each, and
            the frame hash of `bench.py --full`.
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

W, SPP, DEPTH, SEED = 1920, 8, 50, 2024
COPY_BW, HBM_PEAK = 6.3e12, 8.0e12  # B/s: a plain float4 copy on this part; the HBM3E specification
RAY_BYTES, SHADE_BYTES = 48, 160


def med(ms):
    m = statistics.median(ms)
    return {"median": round(m, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def rate(n, ms, bytes_each):
    bps = n * bytes_each / (ms * 1e-3)
    return {"G_per_s": round(n / ms / 1e6, 3), "TB_per_s": round(bps / 1e12, 3),
            "share_of_copy_6.3TBs": round(bps / COPY_BW, 3), "share_of_hbm_peak_8TBs": round(bps / HBM_PEAK, 3)}


def setup():
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=W, spp=SPP, depth=DEPTH)
    dev = rtx.DeviceScene(scene.desc)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    return torch, rtx, scene, dev, cam, reg


def leg_blocks(reps, timed):
    """timed: report the events' times; else the bare sequence for the kernel trace."""
    torch, rtx, scene, dev, cam, reg = setup()
    st = torch.cuda.current_stream().cuda_stream
    n = SPP * cam.image_width * cam.image_height
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    keys = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hits = torch.empty((n, 12), dtype=torch.int32, device="cuda")
    bounce = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    out = {"records": n}
    cam_ms = []
    for k in range(reps + 1):  # the first is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rtx.camera_rays_device(cam, SEED, reg, 0, SPP, rays.data_ptr(), keys.data_ptr(), st)
        e1.record()
        e1.synchronize()
        if k:
            cam_ms.append(e0.elapsed_time(e1))
    out["camera_rays"] = {"kernel_ms": med(cam_ms), **rate(n, statistics.median(cam_ms), RAY_BYTES),
                          "draws_per_ray": round(float(keys[:, 3].double().mean()), 4)}
    octant = rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam))
    for event in (1, 2):
        dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), rtx.RTX_TRACE_UV | octant, st)
        ms = [dev.shade_device(SEED, rays.data_ptr(), hits.data_ptr(), keys.data_ptr(), n, bounce.data_ptr(), 0, st,
                               stats=True).kernel_ms for _ in range(reps + 1)][1:]
        c = dev.shade_device(SEED, rays.data_ptr(), hits.data_ptr(), keys.data_ptr(), n, bounce.data_ptr(),
                             rtx.RTX_SHADE_COUNTERS, st, stats=True)
        out[f"shade_event{event}"] = {"kernel_ms": med(ms), **rate(n, statistics.median(ms), SHADE_BYTES),
                                      "hits": int(c.hits), "scattered": int(c.scattered),
                                      "rng_draws_per_hit": round(c.rng_draws / max(c.hits, 1), 3),
                                      "counting_kernel_ms": round(c.kernel_ms, 4)}
        rays = bounce[:, 8:16].contiguous()
        keys[:, 2] += 1
    torch.cuda.synchronize()
    rtx.device_check(0)
    print(json.dumps(out if timed else {"records": n, "reps": reps}), flush=True)
    return 0


def leg_loop(reps):
    torch, rtx, scene, dev, cam, reg = setup()
    import wavefront

    st = torch.cuda.current_stream().cuda_stream
    img = torch.empty((cam.image_height, cam.image_width, 3), dtype=torch.float32, device="cuda")
    mega, wave = [], []
    for k in range(reps + 1):
        s = dev.render_region(cam, SEED, reg, img.data_ptr(), st, timed=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = wavefront.render(dev, cam, SEED, reg, compact=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k:
            mega.append(s.kernel_ms)
            wave.append((t1 - t0) * 1e3)
    differ = int((got.view(torch.int32) != img.view(torch.int32)).any(dim=2).sum())
    # the contract: on the caller's tree with every box test, where rtx_trace walks what the reference walks, the
    # loop is the render on every pixel (on the library's own trees a trace may resolve a grazing hit of a trapped
    # path differently from the render's guarded walk, DESIGN.md §12, §34: reported, not required)
    ref = rtx.DeviceScene(scene.desc, reference_bvh=True, every_box=True)
    ref.render_region(cam, SEED, reg, img.data_ptr(), st, timed=True)
    got = wavefront.render(ref, cam, SEED, reg, compact=True)
    torch.cuda.synchronize()
    same = bool(torch.equal(got.view(torch.int32), img.view(torch.int32)))
    rtx.device_check(0)
    print(json.dumps({"frame": f"{cam.image_width}x{cam.image_height}x{SPP}, depth {DEPTH}",
                      "megakernel_kernel_ms": med(mega), "wavefront_compact_wall_ms": med(wave),
                      "megakernel_buys": round(statistics.median(wave) / statistics.median(mega), 1),
                      "pixels_differing_on_the_library_trees": differ,
                      "bit_identical_on_the_callers_tree": same}), flush=True)
    return 0 if same else 1


def run(cmd, limit, env=None, log=None):
    """One leg under its own time limit; its stdout.  A limit, a fault or an abort ends the whole sequence."""
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


def kernel_times(trace_dir, reps):
    """Durations (ms) of the new kernels' dispatches from rocprofv3's kernel trace, in dispatch order: the camera
    kernel's, and the shade kernel's split into event 1 and event 2 (reps + 2 calls each: warm-up, reps, counting)."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"],
                             (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    rows.sort()
    cam = [ms for _, name, ms in rows if "camera_rays" in name]
    timed = [ms for _, name, ms in rows  # the timed instantiation, demangled or not
             if "shade_hits" in name and "shade_hits<true" not in name and "shade_hitsILb1" not in name]
    if len(cam) != reps + 1 or len(timed) != 2 * (reps + 1):
        raise SystemExit(f"kernel trace under {trace_dir}: {len(cam)} camera and {len(timed)} shade dispatches, "
                         f"expected {reps + 1} and {2 * (reps + 1)}")
    return cam[1:], timed[1: reps + 1], timed[reps + 2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs="+", default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_rates.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "shade_rates"),
                    help="where the legs' logs and raw kernel traces go (not kept in git)")
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] == "loop":
            return leg_loop(args.reps)
        return leg_blocks(args.reps, args.leg[0] == "blocks")
    if not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    os.makedirs(args.work, exist_ok=True)
    log = os.path.join(args.work, "legs.log")
    py, me = sys.executable, os.path.abspath(__file__)
    parent = {"RTX_LIB": os.path.abspath(args.parent_lib)}
    out = {"what": "path building blocks: camera rays and shade records per second, the loop against the megakernel, "
                   "the headline against the parent",
           "librtx_sha256_16": {"this": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
                                "parent": sha16(args.parent_lib)},
           "bytes": {"camera_ray": RAY_BYTES, "shade_record": SHADE_BYTES}}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["events"] = last_json(run([py, me, "--leg", "blocks", "--reps", str(args.reps)], 300, None, log))
    print(json.dumps(out["events"]), flush=True)
    save()

    d = os.path.join(args.work, "trace")
    run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
         py, me, "--leg", "kernels", "--reps", str(args.reps)], 300, None, log)
    cam, e1, e2 = kernel_times(d, args.reps)
    n = out["events"]["records"]
    out["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own",
                      "camera_rays": {"kernel_ms": med(cam), **rate(n, statistics.median(cam), RAY_BYTES)},
                      "shade_event1": {"kernel_ms": med(e1), **rate(n, statistics.median(e1), SHADE_BYTES)},
                      "shade_event2": {"kernel_ms": med(e2), **rate(n, statistics.median(e2), SHADE_BYTES)}}
    print(json.dumps(out["kernels"]), flush=True)
    save()

    out["loop"] = last_json(run([py, me, "--leg", "loop", "--reps", "2"], 420, None, log))
    print(json.dumps(out["loop"]), flush=True)
    save()

    ms = {"this": [], "parent": []}
    for k in range(args.runs):  # alternated, and who goes first alternates too: drift of the machine hits both alike
        pair = (("parent", parent), ("this", {}))
        for who, env in (pair if k % 2 == 0 else pair[::-1]):
            ms[who].append(last_json(run([py, "bench.py"], 240, env, log))["ms_per_step"])
    full = last_json(run([py, "bench.py", "--full", "--no-cpu"], 300, None, log))
    lo, hi = min(ms["parent"]), max(ms["parent"])
    mine = statistics.median(ms["this"])
    out["headline"] = {"ms_per_step": ms, "median": {k: statistics.median(v) for k, v in ms.items()},
                       "parent_range_ms": [lo, hi], "this_median_within_parent_range": lo <= mine <= hi,
                       "framebuffer_sha256_16": full.get("framebuffer_sha256_16"),
                       # bench.py ties the committed PMC summaries to the library they were measured on, by hash
                       "roofline_stale": (full.get("roofline") or {}).get("stale")}
    print(json.dumps(out["headline"]), flush=True)
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
