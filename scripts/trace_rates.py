#!/usr/bin/env python3
"""What a ray query costs: writes profiles/trace_rates.json, which names the library by hash.

    python scripts/trace_rates.py --parent-lib PATH/librtx.so [--out profiles/trace_rates.json]

One GPU visit, every leg a process of its own under its own `timeout`, warmed up, timed by HIP events around the
launches (rtx_trace_stats.kernel_ms: the call synchronises); the sequence stops at the first leg that fails.
  headline   plain `python bench.py` on this build and on the parent's library (RTX_LIB), alternated, RUNS each.
  yardstick  the PARENT's megakernel on random_spheres 1920x1080 at max_depth = 1, 8 spp: one segment per sample, so
             samples / stats.kernel_ms is its closest-hit rate on camera rays, shading and sample sums included.
  primary    rays per second of rtx_trace_device on the same camera's rays: 1920x1080, 8 jittered rays per pixel,
             in 8x8 tiles (64 consecutive rays are one tile's pixels of one sample), (0.001, inf).
  incoherent the same count: origins uniform in the box of the scene's small spheres, uniform directions.
  big        tests' build_scene(3, 1500, 0): 2999 entries, read from HBM; 4 M incoherent rays.
Each ray-set leg times the plain form (blocks of 64 rays, RTX_TRACE_REFILL=64) against the refill at 48, 40 and
32 parked lanes, alternated in one process, and closest hit against RTX_TRACE_ANY.  The copy bound: 32 B in and 48 B
out per ray at the 6.3 TB/s a plain copy reaches on this part is 78.75 Gray/s.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))

W, SPP, SEED = 1920, 8, 2024
COPY_BOUND_GRAYS = 6.3e12 / 80 / 1e9
REFILLS = (64, 48, 40, 32)


def tile_order(torch, width, height, spp):
    """(x, y) of every ray, in 8x8 tiles, sample-major within a tile: the megakernel's item order."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    t = torch.arange(tx * ty, device="cuda")
    p = torch.arange(64, device="cuda")
    x = ((t % tx) * 8)[:, None, None] + (p % 8)[None, None, :]
    y = ((t // tx) * 8)[:, None, None] + (p // 8)[None, None, :]
    x, y = x.expand(-1, spp, -1).reshape(-1), y.expand(-1, spp, -1).reshape(-1)
    keep = (x < width) & (y < height)
    return x[keep], y[keep]


def camera_rays(torch, cam):
    """GetRay's direction for jittered pixel centres (camera.go:265-299), no lens: 8 floats per ray (rtx_ray)."""
    g = torch.Generator(device="cuda").manual_seed(SEED)
    x, y = tile_order(torch, cam.image_width, cam.image_height, SPP)
    n = x.numel()
    v = lambda a: torch.tensor(list(a), dtype=torch.float32, device="cuda")  # noqa: E731
    jit = torch.rand((n, 2), generator=g, device="cuda") - 0.5
    pc = v(cam.pixel00)[None] + v(cam.pixel_du)[None] * (x.float() + jit[:, 0])[:, None] + \
        v(cam.pixel_dv)[None] * (y.float() + jit[:, 1])[:, None]
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = v(cam.center)[None]
    rays[:, 3] = 0.001
    rays[:, 4:7] = pc - v(cam.center)[None]
    rays[:, 7] = float("inf")
    return rays


def incoherent_rays(torch, n, lo, hi):
    g = torch.Generator(device="cuda").manual_seed(SEED + 1)
    lo, hi = (torch.tensor(a, dtype=torch.float32, device="cuda") for a in (lo, hi))
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    rays[:, 0:3] = lo[None] + (hi - lo)[None] * torch.rand((n, 3), generator=g, device="cuda")
    d = torch.randn((n, 3), generator=g, device="cuda")
    rays[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    rays[:, 3] = 0.001
    rays[:, 7] = float("inf")
    return rays


def time_variants(torch, rtx, dev, rays, reps, flags=0):
    """kernel_ms of every variant, alternated: {name: [ms]}; and the hit count."""
    n = rays.shape[0]
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    variants = [(f"refill_{r}", {"RTX_TRACE_REFILL": str(r)}, flags) for r in REFILLS]
    variants.append(("any_hit", {"RTX_TRACE_REFILL": "64"}, flags | rtx.RTX_TRACE_ANY))
    ms = {name: [] for name, _, _ in variants}

    def run(env, fl):
        os.environ.update(env)
        return dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), fl, st, stats=True)

    for _, env, fl in variants:  # warm-up: layouts, code objects
        run(env, fl)
    for _ in range(reps):
        for name, env, fl in variants:
            ms[name].append(run(env, fl).kernel_ms)
    os.environ.pop("RTX_TRACE_REFILL", None)
    c = run({}, flags | rtx.RTX_TRACE_COUNTERS)
    out = {"rays": n, "hits": int(c.hits), "node_visits_per_ray": round(c.node_visits / n, 2),
           "prim_tests_per_ray": round(c.prim_tests / n, 2), "walk_layout": int(c.walk_layout),
           "scene_placement": int(c.scene_placement)}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"kernel_ms": {"median": round(med, 4), "min": round(min(t), 4), "max": round(max(t), 4)},
                     "Grays_per_s": round(n / med / 1e6, 3)}
    return out


def leg_rays(which, reps):
    import torch

    import rtx

    torch.cuda.set_device(0)
    if which == "big":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ctypes

        from test_random_scenes import build_scene

        d = build_scene(3, 1500, 0)
        dev = rtx.DeviceScene(ctypes.pointer(d))
        rays = incoherent_rays(torch, 4 << 20, (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))
        out = time_variants(torch, rtx, dev, rays, reps)
    else:
        scene = rtx.HostScene("random_spheres", seed=1)
        cam = scene.camera(width=W, spp=SPP, depth=1)
        dev = rtx.DeviceScene(scene.desc)
        rays = camera_rays(torch, cam)
        if which == "incoherent":  # main.go's small spheres: centres within 11 of the axis, on the ground
            rays = incoherent_rays(torch, rays.shape[0], (-11.0, 0.0, -11.0), (11.0, 2.0, 11.0))
        out = time_variants(torch, rtx, dev, rays, reps, rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam)))
    rtx.device_check(0)
    print(json.dumps(out), flush=True)
    return 0


def leg_yardstick(reps):
    """The megakernel at depth 1: one segment per sample."""
    import torch

    import rtx

    torch.cuda.set_device(0)
    scene = rtx.HostScene("random_spheres", seed=1)
    cam = scene.camera(width=W, spp=SPP, depth=1)
    dev = rtx.DeviceScene(scene.desc)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    out = torch.empty((cam.image_height, cam.image_width, 3), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        dev.render_region(cam, SEED, reg, out.data_ptr(), st, timed=True)
    ms = [dev.render_region(cam, SEED, reg, out.data_ptr(), st, timed=True).kernel_ms for _ in range(reps)]
    c = dev.render_region(cam, SEED, reg, out.data_ptr(), st, counters=True)
    n = cam.image_width * cam.image_height * SPP
    assert c.segments == n, (c.segments, n)
    med = statistics.median(ms)
    rtx.device_check(0)
    print(json.dumps({"segments": n, "kernel_ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
                      "Gsegments_per_s": round(n / med / 1e6, 3), "node_visits_per_segment": round(c.node_visits / n, 2),
                      "prim_tests_per_segment": round(c.prim_tests / n, 2), "walk_layout": int(c.walk_layout)}), flush=True)
    return 0


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
    ap.add_argument("--leg", nargs="+", default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_rates.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "out", "trace_rates"), help="the legs' logs (not kept in git)")
    args = ap.parse_args()
    if args.leg:
        return leg_yardstick(args.reps) if args.leg[0] == "yardstick" else leg_rays(args.leg[0], args.reps)
    if not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    os.makedirs(args.work, exist_ok=True)
    log = os.path.join(args.work, "legs.log")
    py, me = sys.executable, os.path.abspath(__file__)
    parent = {"RTX_LIB": os.path.abspath(args.parent_lib)}
    out = {"what": "ray queries: rays per second against the parent's megakernel at depth 1; headline against the parent",
           "librtx_sha256_16": {"this": sha16(os.path.join(ROOT, "raytracer-go_amd", "librtx.so")),
                                "parent": sha16(args.parent_lib)},
           "copy_bound_Grays_per_s": round(COPY_BOUND_GRAYS, 2)}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["yardstick_parent_megakernel_depth1"] = last_json(run([py, me, "--leg", "yardstick", "--reps", str(args.reps)], 240,
                                                              parent, log))
    print(json.dumps(out["yardstick_parent_megakernel_depth1"]), flush=True)
    for which in ("primary", "incoherent", "big"):
        out[which] = last_json(run([py, me, "--leg", which, "--reps", str(args.reps)], 300, None, log))
        print(which, json.dumps(out[which]), flush=True)
        save()
    y = out["yardstick_parent_megakernel_depth1"]["Gsegments_per_s"]
    out["primary_over_megakernel_depth1"] = {k: round(out["primary"][k]["Grays_per_s"] / y, 3)
                                             for k in out["primary"] if k.startswith("refill_")}
    save()

    ms = {"this": [], "parent": []}
    for k in range(args.runs):  # alternated, and who goes first alternates too: drift of the machine hits both alike
        pair = (("parent", parent), ("this", {}))
        for who, env in (pair if k % 2 == 0 else pair[::-1]):
            ms[who].append(last_json(run([py, "bench.py"], 240, env, log))["ms_per_step"])
    spread = max(ms["parent"]) - min(ms["parent"])
    out["headline"] = {"ms_per_step": ms, "median": {k: statistics.median(v) for k, v in ms.items()},
                       "parent_spread_ms": round(spread, 4),
                       "no_worse_than_parent_beyond_its_spread":
                           statistics.median(ms["this"]) <= statistics.median(ms["parent"]) + spread}
    print(json.dumps(out["headline"]), flush=True)
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
