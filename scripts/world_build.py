#!/usr/bin/env python3
"""Build time of the GPU BVH build for whole Worlds -> profiles/world_build.json.

  python scripts/world_build.py --parent-lib PATH/librtx.so [--runs 5] [--out profiles/world_build.json]

stress_100k's World (100 001 spheres) is built through rtx_scene_create_spheres with the parent's library and through
rtx_scene_create_world (items == NULL) with this tree's, alternating, `runs` times each; then through this tree's
rtx_scene_create_spheres (which forwards to the same build), and a mixed World of the same item count in which every
fifth sphere is replaced by a square quad of its size.  Every build runs in a fresh child process (one library per
process), after one small build that initialises the device and loads the code object; build_ms is the library's own
wall time of the build (rtx_bvh.hip).  The host mirror does not expose the time of its NewBVH: not measured here.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-go_amd"))


def child(mode: str) -> None:
    import rtx

    L = rtx.load()
    host = rtx.HostScene("stress_100k", 1)
    arr, n, draw0, seed = host.world_spheres()
    d = host.desc.contents
    tabs = (d.materials, d.n_materials, d.textures, d.n_textures, d.texels, d.n_texels)
    h, ms = ctypes.c_void_p(), ctypes.c_double()
    rtx.check(L.rtx_scene_create_spheres(arr, 64, *tabs, seed, draw0, ctypes.byref(h), None), "warm-up")
    L.rtx_scene_destroy(h)
    n_quads = 0
    if mode == "spheres":
        rtx.check(L.rtx_scene_create_spheres(arr, n, *tabs, seed, draw0, ctypes.byref(h), ctypes.byref(ms)), mode)
    elif mode == "world":
        rtx.check(L.rtx_scene_create_world(None, n, arr, n, None, 0, *tabs, seed, draw0, ctypes.byref(h), ctypes.byref(ms)), mode)
    else:  # mixed: every fifth item a quad in the sphere's place
        items = (ctypes.c_int32 * n)()
        quads = (rtx.Quad * (n // 5 + 1))()
        for i in range(n):
            if i % 5 == 4:
                s = arr[i]
                c, r = list(s.center), s.radius
                quads[n_quads] = rtx.quad((c[0] - r, c[1], c[2] - r), (2 * r, 0, 0), (0, 0, 2 * r), s.material)
                items[i] = rtx.ref_prim(rtx.RTX_PRIM_QUAD, n_quads)
                n_quads += 1
            else:
                items[i] = rtx.ref_prim(rtx.RTX_PRIM_SPHERE, i)
        rtx.check(L.rtx_scene_create_world(items, n, arr, n, quads, n_quads, *tabs, seed, draw0, ctypes.byref(h),
                                           ctypes.byref(ms)), mode)
    entries = int(L.rtx_scene_export(h, None, 0)) // 32
    L.rtx_scene_destroy(h)
    print(json.dumps({"mode": mode, "items": n, "quads": n_quads, "entries": entries, "build_ms": ms.value}))


def run(mode: str, lib) -> dict:
    env = dict(os.environ)
    env.pop("RTX_LIB", None)
    if lib:
        env["RTX_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env, capture_output=True,
                       text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"{mode} with {lib or 'this tree'} failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def summary(rows):
    ms = [r["build_ms"] for r in rows]
    return {"build_ms": ms, "median": statistics.median(ms), "min": min(ms), "max": max(ms), "items": rows[0]["items"],
            "quads": rows[0]["quads"], "entries": rows[0]["entries"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_build.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's librtx.so")
    parent, world = [], []
    for _ in range(a.runs):  # alternated
        parent.append(run("spheres", a.parent_lib))
        world.append(run("world", None))
    forward = [run("spheres", None) for _ in range(a.runs)]
    mixed = [run("mixed", None) for _ in range(a.runs)]
    out = {"scene": "stress_100k", "runs": a.runs,
           "parent_create_spheres": summary(parent), "create_world_items_null": summary(world),
           "create_spheres_forwarding": summary(forward), "create_world_mixed_fifth_quads": summary(mixed),
           "host_mirror_build_ms": None, "host_mirror_note": "the mirror does not expose the time of its NewBVH: not measured"}
    p, w = out["parent_create_spheres"], out["create_world_items_null"]
    out["yardstick"] = {"bound_ms": p["max"] + (p["max"] - p["min"]), "new_median_ms": w["median"],
                        "within": w["median"] <= p["max"] + (p["max"] - p["min"])}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
