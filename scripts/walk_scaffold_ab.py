#!/usr/bin/env python3
"""A/B of the kernels that walk a trace layout, this build against another build of librtx.so.

    python scripts/walk_scaffold_ab.py --parent-lib PATH [--alternations 5] [--reps 5]

Every leg is a fresh process under its own timeout, with RTX_LIB naming its library, and times by the stats' kernel_ms
(HIP events around the launches) with the default knobs, on the workloads the rates scripts define:

  trace_camera, trace_incoherent   trace_rays on randSpheres' camera rays and on the incoherent set (trace_rates.py)
  guides                           guide_images at 1920 x 1080 x 4 (denoise_rates.py)
  direct_block, add_direct         direct_lights on cornell_box's first hits and the fused pass of 16 samples on its
                                   frame (direct_rates.py)

One alternation is three legs: this build, the parent, the parent again.  Per kernel the result is the median over
the alternations of new / parent beside the range of parent / parent; the sequence stops at the first leg that fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ("trace_camera", "trace_incoherent", "guides", "direct_block", "add_direct")


def leg(reps):
    import torch

    import denoise_rates
    import direct_rates
    import rtx
    import trace_rates

    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    ms = {}

    def timed(call):
        call()  # warm-up: layouts, code objects
        return [call().kernel_ms for _ in range(reps)]

    # trace_rays and guide_images on random_spheres
    scene = rtx.HostScene("random_spheres", seed=1)
    dev = rtx.DeviceScene(scene.desc)
    cam = scene.camera(width=trace_rates.W, spp=trace_rates.SPP, depth=1)
    flags = rtx.RTX_TRACE_OCTANT(rtx.camera_octant(cam))
    rays = trace_rates.camera_rays(torch, cam)
    n = rays.shape[0]
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    ms["trace_camera"] = timed(lambda: dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), flags, st, stats=True))
    rays = trace_rates.incoherent_rays(torch, n, (-11.0, 0.0, -11.0), (11.0, 2.0, 11.0))
    ms["trace_incoherent"] = timed(lambda: dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), flags, st, stats=True))
    del rays, hits
    cam = scene.camera(width=denoise_rates.W, spp=denoise_rates.SPP, depth=50)
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    guides = torch.empty((cam.image_width * cam.image_height * 32,), dtype=torch.uint8, device="cuda")
    ms["guides"] = timed(lambda: dev.guides_device(cam, denoise_rates.SEED, reg, 0, denoise_rates.SPP, guides.data_ptr(), st,
                                                   stats=True))
    dev.close()

    # direct_lights and direct_paths on cornell_box
    _, rtx, scene, dev, cam = direct_rates.setup("cornell_box")
    reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    spp, seed = direct_rates.SPP, direct_rates.SEED
    n = spp * cam.image_width * cam.image_height
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    keys = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hits = torch.empty((n, 12), dtype=torch.int32, device="cuda")
    light = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    rtx.camera_rays_device(cam, seed, reg, 0, spp, rays.data_ptr(), keys.data_ptr(), st)
    dev.trace_device(rays.data_ptr(), n, hits.data_ptr(), rtx.RTX_TRACE_UV, st)
    ms["direct_block"] = timed(lambda: dev.direct_device(seed, hits.data_ptr(), keys.data_ptr(), n, light.data_ptr(), 0, st,
                                                         stats=True))

    def fused():
        acc = dev.accumulator(cam, seed, reg)
        s = acc.add_direct(direct_rates.N, st, stats=True)
        acc.close()
        return s

    ms["add_direct"] = timed(fused)
    torch.cuda.synchronize()
    rtx.device_check(0)
    print(json.dumps({k: round(statistics.median(v), 4) for k, v in ms.items()}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_scaffold_ab.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.reps)
    from trace_rates import last_json, run, sha16

    new_lib = os.path.join(ROOT, "raytracer-go_amd", "librtx.so")
    parent = os.path.abspath(a.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(a.reps)]
    rows = []
    for k in range(a.alternations):
        row = {name: last_json(run(cmd, 300, env={"RTX_LIB": lib}))
               for name, lib in (("new", new_lib), ("parent", parent), ("parent_again", parent))}
        rows.append(row)
        print(k, json.dumps(row), flush=True)
    out = {"new_lib_sha16": sha16(new_lib), "parent_lib_sha16": sha16(parent), "reps_per_leg": a.reps,
           "kernel_ms_medians_per_alternation": rows, "kernels": {}}
    ok = True
    for name in KERNELS:
        np_ = [r["new"][name] / r["parent"][name] for r in rows]
        pp = [r["parent_again"][name] / r["parent"][name] for r in rows]
        inside = min(pp) <= statistics.median(np_) <= max(pp)
        ok = ok and (inside or statistics.median(np_) < min(pp))
        out["kernels"][name] = {"new_over_parent": {"median": round(statistics.median(np_), 4), "min": round(min(np_), 4),
                                                    "max": round(max(np_), 4)},
                                "parent_over_parent": {"median": round(statistics.median(pp), 4), "min": round(min(pp), 4),
                                                       "max": round(max(pp), 4)},
                                "parent_kernel_ms": round(statistics.median(r["parent"][name] for r in rows), 4),
                                "new_median_within_parent_spread": inside}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernels"], indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
