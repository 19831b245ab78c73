"""The census of the render kernels: every render_items / render_drain instantiation librtx.so contains is on a
committed list (tests/render_kernels.txt), and every one the dispatch can reach is launched against the oracle with
evidence that it did work.

  test_list_matches_library   CPU: the library's kernel symbols and the list are the same set.
  test_family[<family>]       GPU: one child process each (RTX_WATCHDOG_S=10, its own time limit).  A family walks a
                              product of the knobs that reach the dispatch on one or two scenes and runs every
                              combination through the project's checks — parity.check_scene (bit-identical to the
                              oracle on the walked tree, the seven work counters the oracle's) and
                              test_adaptive_gpu.run_adaptive (the ADAPT instantiations: only an adaptive pass launches
                              them).  With RTX_DEBUG_LAUNCH=1 every launch prints "rtx launch: <mangled name>"; the
                              child attributes the names to the call that launched them and to that call's rtx_stats.
  test_every_reachable_kernel_ran   the names seen with evidence are the list minus UNREACHABLE, and no name of
                              UNREACHABLE was ever launched.  UNREACHABLE is empty: the dispatch compiles no kernel it
                              cannot launch, so every listed kernel is seen with evidence.

Evidence, per kernel class (the call's own stats; the call belongs to a combination all of whose checks passed):
  TIER 0            the image is the oracle's
  TIER 1, drain     and deferred_paths > 0; the drain: its "rtx tiered:" line says "drain 1"
  TIER 2            deferred_paths > 0 (the far pass's own launch: RTX_DRAIN=0, or a launch without drain)
  TIER 3            redo_chunks >= 1 (a queue too small on purpose); a redo kernel that only returned does not count
  CLK               bit-identical to the oracle and to the same render without RTX_FLAG_TIMING; trav_cycles > 0,
                    shade_cycles > 0, and the four shade_split_cycles sum to at most shade_cycles (rtx.h: a split)
  COUNT             the seven work counters are the oracle's (check_scene; the first adaptive pass, every tile open,
                    against the oracle's counters of a render of that many samples).  The redo combinations compare the
                    five path counters, as test_tier_queue_overflow_redo does: a sample rendered again walks the
                    guarded tree from its camera ray, which changes the box and primitive tests, not a path.

If a child ends by a signal, its time limit or a HIP error, no further child is started (STOPPED).
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = os.path.join(ROOT, "tests", "render_kernels.txt")
LIB = os.path.join(ROOT, "raytracer-go_amd", "librtx.so")

ITEMS = re.compile(r"^_ZN4rtxd12render_itemsILb([01])ELb([01])ELb([01])ELb([01])ELi(\d+)ELi(\d+)ELb([01])ELb([01])"
                   r"ELi([0-3])ELb([01])ELb([01])ELb([01])EEEvNS_6ParamsE$")
DRAIN = re.compile(r"^_ZN4rtxd12render_drainILb([01])ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])ELb([01])"
                   r"EEEvNS_9DrainArgsE$")
KERNEL = re.compile(r"^_ZN4rtxd12render_(items|drain)I")
ITEM_ARGS = ("COUNT", "USE_LDS", "QUADS", "NOISE", "WAVES", "MINW", "HYB", "CLK", "TIER", "POOL", "ST", "ADAPT")
DRAIN_ARGS = ("USE_LDS", "WAVES", "MINW", "HYB", "POOL", "ST", "QUADS", "ADAPT")


def parse(name: str) -> dict:
    """The template arguments of a mangled render kernel name, and kind = "items" / "drain"."""
    m = ITEMS.match(name)
    if m:
        return dict(zip(ITEM_ARGS, (int(v) for v in m.groups())), kind="items")
    m = DRAIN.match(name)
    assert m, f"not a render kernel: {name}"
    return dict(zip(DRAIN_ARGS, (int(v) for v in m.groups())), kind="drain", COUNT=0, CLK=0, TIER=1, NOISE=0)


def items_name(**a) -> str:
    b = lambda k: f"Lb{a[k]}E"  # noqa: E731
    return ("_ZN4rtxd12render_itemsI" + b("COUNT") + b("USE_LDS") + b("QUADS") + b("NOISE") + f"Li{a['WAVES']}E" +
            f"Li{a['MINW']}E" + b("HYB") + b("CLK") + f"Li{a['TIER']}E" + b("POOL") + b("ST") + b("ADAPT") + "EEvNS_6ParamsE")


def listed() -> list:
    with open(LIST) as f:
        return [ln.split("\t")[0] for ln in f.read().splitlines() if ln and not ln.startswith("#")]


# kernel name -> the dispatch condition that excludes it for every scene, flag, region and environment knob.  Empty: the
# launchers take the placement as a template argument and name only the kernels they launch, so every
# listed kernel needs evidence.  (items_name builds a name for a future entry.)
UNREACHABLE = {}


# ---- the CPU test ---------------------------------------------------------------------------------------------------
def library_kernels(path: str = LIB, KERNEL=KERNEL) -> set:
    """The render kernels' handle symbols of the library (weak objects named as the kernels are); KERNEL: the pattern of
    another set of kernels (tests/test_block_census.py)."""
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {r[-1] for r in rows if len(r) >= 3 and r[-2] in ("V", "v", "B", "D") and KERNEL.match(r[-1])}
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = subprocess.run([readelf, "--dyn-syms", "-W", path], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[-1] for r in rows if len(r) >= 8 and r[3] == "OBJECT" and r[6] != "UND" and KERNEL.match(r[-1])}


def test_list_matches_library(built):
    """tests/render_kernels.txt and librtx.so name the same render kernels: an instantiation added without a line, or a
    line whose instantiation is gone, fails here.  Every name parses, and UNREACHABLE names listed kernels only."""
    want, have = listed(), library_kernels()
    assert len(want) == len(set(want)), "a kernel is listed twice"
    assert not have - set(want), f"in librtx.so, not in render_kernels.txt: {sorted(have - set(want))}"
    assert not set(want) - have, f"in render_kernels.txt, not in librtx.so: {sorted(set(want) - have)}"
    for name in want:
        parse(name)
    assert not set(UNREACHABLE) - set(want), sorted(set(UNREACHABLE) - set(want))


# ---- the children ---------------------------------------------------------------------------------------------------
KNOBS = ("RTX_HOT_ENTRIES", "RTX_CAM_POOL", "RTX_DRAIN", "RTX_ITEM_WAVES", "RTX_TIER_QUADS", "RTX_DEFER_CAP", "RTX_REDO_CAP")
EXIT_HIP = 3  # the child's exit status after a HIP error (RTX_ERR_HIP: a fault, or the watchdog)
MARK = "CENSUS "
TIMING = 1 << 20
NO_LDS = 4


class Launch:
    """One C-ABI call that launched render kernels: their names, the call's launch lines and its stats."""

    def __init__(self, names, lines, st):
        self.names, self.lines, self.st = names, lines, st


class Recorder:
    """fd 2 into a file, so that the library's launch lines can be read back call by call."""

    def __init__(self):
        self.file = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        self.pos = 0
        self.calls = []  # of the running combination

    def take(self) -> str:
        sys.stderr.flush()
        self.file.seek(self.pos)
        data = self.file.read()
        self.pos += len(data)
        return data.decode(errors="replace")

    def wrap(self, fn, stats_of):
        def call(*a, **kw):
            self.take()
            out = fn(*a, **kw)
            lines = self.take().splitlines()
            names = [ln[len("rtx launch: "):] for ln in lines if ln.startswith("rtx launch: ")]
            if names:
                self.calls.append(Launch(names, lines, stats_of(out)))
            return out
        return call

    def close(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        self.file.seek(0)
        os.write(2, self.file.read()[-200_000:])


def evidence(k: dict, call: Launch):
    """None when `call` shows that kernel k worked (module docstring), else what is missing."""
    st = call.st
    if st is None:
        return "no stats"
    if k["kind"] == "drain" and not any(ln.startswith("rtx tiered:") and "drain 1" in ln for ln in call.lines):
        return "no 'drain 1' line"
    if k["TIER"] in (1, 2) and not st.deferred_paths > 0:
        return "deferred_paths == 0"
    if k["TIER"] == 3 and not st.redo_chunks >= 1:
        return "redo_chunks == 0"
    if k["CLK"]:
        if not (st.trav_cycles > 0 and st.shade_cycles > 0):
            return "no cycles"
        if sum(st.shade_split_cycles) > st.shade_cycles:
            return "the split exceeds shade_cycles"
    if k["COUNT"] and not st.samples > 0:
        return "no samples counted"
    return None


class Census:
    """The child's state: the scenes, the cached oracle results, the calls of the running combination."""

    def __init__(self, family):
        import numpy as np
        import torch

        import parity
        import rtx
        import test_adaptive_gpu

        self.np, self.torch, self.parity, self.rtx, self.tag = np, torch, parity, rtx, test_adaptive_gpu
        self.family = family
        self.rec = Recorder()
        self.seen, self.launched, self.missing, self.failures, self.combos = {}, set(), {}, [], 0
        self.oracle, self.okey, self.plain, self.devs = {}, None, {}, {}
        rtx.DeviceScene.render_region = self.rec.wrap(rtx.DeviceScene.render_region, lambda st: st)
        rtx.Accumulator.add_adaptive = self.rec.wrap(rtx.Accumulator.add_adaptive, lambda out: out[0])
        orig = parity.oracle_checks

        def cached(desc, walk, cam, seed, reg, skip=None, tier=None):
            key = (self.okey, tier is not None, cam.samples_per_pixel, cam.image_width, seed, reg.x0, reg.y0, reg.width,
                   reg.height, reg.rank, reg.world, reg.stripe)
            if key not in self.oracle:
                self.oracle[key] = orig(desc, walk, cam, seed, reg, skip, tier)
            return self.oracle[key]

        parity.oracle_checks = cached  # check_scene's oracle renders, once per (scene, walk, camera, seed, region)

    def dev(self, scene, **how):
        """The scene's DeviceScene for these creation-time knobs (the caller has set the environment)."""
        key = (scene.name, tuple(sorted(how.items())), os.environ.get("RTX_HOT_ENTRIES"), os.environ.get("RTX_TIER_QUADS"))
        if key not in self.devs:
            self.devs[key] = self.rtx.DeviceScene(scene.desc, **how)
        return self.devs[key]

    def combo(self, label, env, fn):
        """Run one combination under `env`; its calls count only when every check of fn passed."""
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        self.rec.calls = []
        self.combos += 1
        try:
            fn()
        except self.rtx.RtxError as e:
            if e.code == self.rtx.RTX_ERR_HIP:
                raise
            self.failures.append(f"{label}: {e}")
            return
        except Exception as e:  # a failed check; anything that names a HIP error ends the child
            if "HIP error" in str(e) or "hipError" in str(e):
                raise
            self.failures.append(f"{label}: {type(e).__name__}: {str(e)[:300]}")
            return
        for call in self.rec.calls:
            for name in call.names:
                self.launched.add(name)
                why = evidence(parse(name), call)
                if why is None:
                    self.seen.setdefault(name, label)
                else:
                    self.missing.setdefault(name, f"{label}: {why}")

    # -- the checks ---------------------------------------------------------------------------------------------------
    def one_shot(self, scene, dev, reg, mode, flags, key):
        """check_scene by the timed, the counting or the CLK kernel (the last also against the render without the flag)."""
        P, np = self.parity, self.np
        cam = scene.cam_of(scene.spp)
        self.okey = scene.name
        if mode == "clk":
            img, _, _ = P.check_scene(self.torch, dev, scene.desc, cam, scene.seed, reg, flags=flags | TIMING, kernels=("timed",))
            plain, _ = P.gpu_region(self.torch, dev, cam, scene.seed, reg, counters=False, flags=flags)
            assert np.array_equal(img, plain), "RTX_FLAG_TIMING changes the image"
        else:
            P.check_scene(self.torch, dev, scene.desc, cam, scene.seed, reg, flags=flags,
                          kernels=("counting",) if mode == "count" else ("timed",))

    def adaptive(self, scene, dev, reg, mode, flags, key):
        """run_adaptive by the ADAPT instantiations; counting: the first pass (every tile open) has the oracle's seven
        work counters; CLK: the same image as without the flag."""
        import accum_ref

        P, np = self.parity, self.np
        passes, tol, min_samples = scene.adapt
        col = accum_ref.sample_colours(scene.key, scene.desc, scene.cam_of(sum(passes)), scene.seed, reg, sum(passes))
        n0 = len(self.rec.calls)
        out = self.tag.run_adaptive(self.torch, dev, scene.cam_of, scene.seed, reg, passes, tol, min_samples, col,
                                    counting=(mode == "count"), flags=flags | (TIMING if mode == "clk" else 0))
        assert out[4][0][0] > 0, "no tile was open in the first pass"
        if mode == "count":
            first = next(c for c in self.rec.calls[n0:] if any(parse(n).get("ADAPT") for n in c.names))
            cam = scene.cam_of(passes[0])
            self.okey = scene.name
            tier = P.tier_of(dev, scene.desc, cam)
            walk, skip, tw = tier if tier is not None else (*P.walk_of(dev, scene.desc, cam), None)
            _, cnt, _ = P.oracle_checks(scene.desc, walk, cam, scene.seed, reg, skip, tw)
            P.assert_counters_equal(first.st, cnt)
        if mode == "timed":
            self.plain[key] = out[1]
        if mode == "clk":
            assert np.array_equal(out[1], self.plain[key]), "RTX_FLAG_TIMING changes the adaptive image"

    def redo(self, scene, dev, reg, mode, flags, key):
        """A queue too small on purpose (the combination's RTX_DEFER_CAP / RTX_REDO_CAP): the redo pass renders the samples
        that did not fit again; the image is still the oracle's, the path counters too."""
        P, np = self.parity, self.np
        cam = scene.cam_of(scene.spp)
        self.okey = scene.name
        tier = P.tier_of(dev, scene.desc, cam)
        assert tier is not None, "the scene does not walk in tiers"
        it, cnt, _ = P.oracle_checks(scene.desc, tier[0], cam, scene.seed, reg, tier[1], tier[2])
        got, st = P.gpu_region(self.torch, dev, cam, scene.seed, reg, counters=(mode == "count"), flags=flags)
        assert st.walk_layout & self.rtx.RTX_LAYOUT_TIERED and st.redo_chunks >= 1, (st.walk_layout, st.redo_chunks)
        assert np.array_equal(got, it), f"redo: {int((got != it).any(axis=2).sum())} pixels differ from the oracle"
        if mode == "count":
            P.assert_counters_equal(st, cnt, P.PATH_KEYS)

    def report(self):
        self.rtx.device_check(0)
        return {"family": self.family, "combos": self.combos, "seen": self.seen, "launched": sorted(self.launched),
                "missing": {k: v for k, v in self.missing.items() if k not in self.seen}, "failures": self.failures}


class Scene:
    def __init__(self, name, desc, cam_of, window, seed, key, adapt, spp=4, keep=None):
        self.name, self.desc, self.cam_of, self.window, self.seed, self.key = name, desc, cam_of, window, seed, key
        self.adapt, self.spp, self.keep = adapt, spp, keep


def host_scene(name, width, window, depth=0, adapt=((4, 4, 4), 0.3, 4), seed=23):
    import rtx

    s = rtx.HostScene(name, 1)
    return Scene(name, s.desc, lambda n: s.camera(width=width, spp=n, depth=depth), window, seed, (name, 1, width, depth),
                 adapt, keep=s)


def big_scene(name, adapt):
    import big_scenes as bs
    from test_big_scenes import SEED

    b = bs.scene(name)
    return Scene(name, b.desc, lambda n: bs.camera(name, spp=n), bs.window(name), SEED, ("big_scenes." + name, bs.SEED, bs.CAM_SEED),
                 adapt, keep=b)


def spheres():  # test_adaptive_gpu's case 1: 24, 21, 13 and 9 of the 24 tiles open in the four passes
    return host_scene("random_spheres", 48, (0, 0, 48, 27), 50, ((4, 4, 4, 4), 0.3, 4), seed=7)


def regions(rtx, scene, striped=(False, True)):
    """[(ST, region)]: the whole window, and the second of two shards of 8-row stripes (the ST instantiations)."""
    out = []
    for st in striped:
        reg = rtx.Region(*scene.window, 1, 2, 8) if st else rtx.Region(*scene.window, 0, 1)
        assert 0 < rtx.region_rows(reg) <= reg.height and (not st or reg.height >= 16)
        out.append((int(st), reg))
    return out


def untiered(c: Census, scene, placements, modes=("timed", "count", "clk"), striped=(False, True), **how):
    """placements x ST x mode x (one-shot, adaptive) on a scene that walks one tree."""
    for (pname, env, flags), (st, reg), mode, adapt in itertools.product(placements, regions(c.rtx, scene, striped), modes,
                                                                         (False, True)):
        if mode == "clk" and env.get("RTX_ITEM_WAVES") == "4":
            continue  # launch_render_t: RTX_FLAG_TIMING is for item_waves != 4 (the 4-wave set has no CLK kernels)
        label = f"{scene.name} {pname} st={st} {mode}" + (" adaptive" if adapt else "")
        key = (scene.name, pname, st, adapt)
        run = c.adaptive if adapt else c.one_shot
        c.combo(label, env, lambda: run(scene, c.dev(scene, **how), reg, mode, flags, key))


def tiered(c: Census, scene, placements, modes=("timed", "count", "clk"), striped=(False, True), **how):
    """placements x drain x ST x mode x (one-shot, adaptive), then the redo pass, on a scene that walks in tiers."""
    for (pname, env, flags), drain, (st, reg), mode, adapt in itertools.product(
            placements, ("1", "0"), regions(c.rtx, scene, striped), modes, (False, True)):
        if drain == "0" and mode != "timed":
            continue  # launch_tiered's CAN_DRAIN: only the timed kernels drain, RTX_DRAIN changes nothing for the others
        label = f"{scene.name} tiered {pname} drain={drain} st={st} {mode}" + (" adaptive" if adapt else "")
        key = (scene.name, pname, drain, st, adapt)
        run = c.adaptive if adapt else c.one_shot
        c.combo(label, dict(env, RTX_DRAIN=drain), lambda: run(scene, c.dev(scene, **how), reg, mode, flags, key))
    for (pname, env, flags), (st, reg), mode, caps in itertools.product(
            placements, regions(c.rtx, scene, striped), ("timed", "count"), (("0", "100"), ("0", "0"))):
        label = f"{scene.name} tiered {pname} st={st} {mode} redo cap={caps[0]}/{caps[1]}"
        c.combo(label, dict(env, RTX_DEFER_CAP=caps[0], RTX_REDO_CAP=caps[1]),
                lambda: c.redo(scene, c.dev(scene, **how), reg, mode, flags, None))


SMALL = [("lds-pool", {}, 0), ("lds", {"RTX_CAM_POOL": "0"}, 0), ("hbm", {}, NO_LDS),
         ("lds-4w", {"RTX_ITEM_WAVES": "4"}, 0), ("hbm-4w", {"RTX_ITEM_WAVES": "4"}, NO_LDS)]
BIG = [("cache-12w", {}, 0), ("cache-8w", {"RTX_HOT_ENTRIES": "832"}, 0), ("hbm", {"RTX_HOT_ENTRIES": "0"}, 0),
       ("cache-4w", {"RTX_ITEM_WAVES": "4"}, 0), ("hbm-4w", {"RTX_ITEM_WAVES": "4", "RTX_HOT_ENTRIES": "0"}, 0)]


def family_spheres_untiered(c):
    untiered(c, spheres(), SMALL, no_tier=True)


def family_spheres_tiered(c):
    tiered(c, spheres(), SMALL[:3])


def family_big_spheres(c):
    s = big_scene("big_ties", ((4, 4), 0.5, 4))
    untiered(c, s, BIG, no_tier=True)
    tiered(c, s, BIG[:1], modes=("timed", "count"))


def family_quads_untiered(c):
    untiered(c, host_scene("cornell_box", 600, (280, 296, 24, 20), adapt=((4, 4, 4), 0.8, 4)), SMALL)


def with_quads(name, base: Scene) -> Scene:
    """A sphere scene with two free-standing quads under a new root beside its tree.  The Cornell box and quad_demo walk in
    tiers with RTX_TIER_QUADS=1, but no path of theirs leaves the near region (it holds every quad), so their near, far
    and drain kernels would only be launched; here the paths off the far ground are deferred as randSpheres' are."""
    import ctypes

    import numpy as np

    import ref64_cases as rc
    import rtx

    t = rc.Tables()
    t.quad((2.5, 0.0, 1.5), (1.2, 0.0, 0.6), (0.0, 1.4, 0.0), 1)
    t.quad((5.0, 0.0, -1.0), (0.3, 0.0, -1.0), (0.0, 0.9, 0.2), 2)
    d = base.desc.contents
    assert d.n_roots == 1 and d.roots[0] >= 0, "one tree (a scene with several roots does not walk in tiers)"
    F = np.float32
    boxes = []
    for q in t.quads:  # NewQuad's box: Q and Q + u + v, an axis thinner than 1e-4 padded by as much
        a, b = np.array(list(q.q), F), (np.array(list(q.q), F) + np.array(list(q.u), F)) + np.array(list(q.v), F)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        thin = (hi - lo) < F(1e-4)
        boxes.append((np.where(thin, lo - F(1e-4), lo).astype(F), np.where(thin, hi + F(1e-4), hi).astype(F)))
    nodes = (rtx.BvhNode * (d.n_nodes + 2))(*[d.nodes[i] for i in range(d.n_nodes)])
    pair, top, old = d.n_nodes, d.n_nodes + 1, d.roots[0]
    lo, hi = np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1])
    nodes[pair].bmin[:], nodes[pair].bmax[:] = [float(v) for v in lo], [float(v) for v in hi]
    nodes[pair].left, nodes[pair].right = (rtx.ref_prim(rtx.RTX_PRIM_QUAD, i) for i in range(2))
    lo, hi = np.minimum(lo, np.array(list(nodes[old].bmin), F)), np.maximum(hi, np.array(list(nodes[old].bmax), F))
    nodes[top].bmin[:], nodes[top].bmax[:] = [float(v) for v in lo], [float(v) for v in hi]
    nodes[top].left, nodes[top].right = old, pair
    w = rtx.SceneDesc()
    for f, _ in rtx.SceneDesc._fields_:
        setattr(w, f, getattr(d, f))
    quads = (rtx.Quad * 2)(*t.quads)
    roots = (ctypes.c_int32 * 1)(top)
    w.quads, w.n_quads = ctypes.cast(quads, ctypes.POINTER(rtx.Quad)), 2
    w.nodes, w.n_nodes = ctypes.cast(nodes, ctypes.POINTER(rtx.BvhNode)), d.n_nodes + 2
    w.roots, w.n_roots = ctypes.cast(roots, ctypes.POINTER(ctypes.c_int32)), 1
    p = ctypes.pointer(w)
    p._keep = (w, quads, nodes, roots, base)
    return Scene(name, p, base.cam_of, base.window, base.seed, ("census." + name,), base.adapt, keep=base)


def family_quads_tiered(c):
    quads = {"RTX_TIER_QUADS": "1"}
    tiered(c, with_quads("spheres_quads", spheres()), [(n, dict(e, **quads), f) for n, e, f in SMALL[:3]],
           modes=("timed", "count"), striped=(False,))
    tiered(c, with_quads("big_ties_quads", big_scene("big_ties", ((4, 4), 0.5, 4))), [("cache-12w", quads, 0)],
           modes=("timed", "count"), striped=(False,))


def family_big_quads(c):
    untiered(c, big_scene("mixed", ((4, 4), 0.4, 4)), BIG)


def noise_quad_scene():
    """ref64_cases' noise probe: a sphere and a quad with Perlin textures — a NOISE scene with a quad that fits the LDS copy."""
    import ref64_cases as rc
    import rtx

    desc, cam0 = rc.noise_scene(4.0, 0.5, (0.0, 0.0, 0.0))

    def cam_of(n):
        cam = rtx.Camera.from_buffer_copy(cam0)
        cam.samples_per_pixel = n
        return cam

    return Scene("noise_quad", desc, cam_of, (0, 0, rc.W, rc.H), 20, ("ref64_cases.noise_scene", 4.0, 0.5), ((4, 4), 0.002, 4))


def family_noise(c):
    small = [("lds", {}, 0), ("hbm", {}, NO_LDS)]
    untiered(c, host_scene("perlin_demo", 400, (150, 96, 24, 20), adapt=((4, 4, 4), 0.5, 4)), small, modes=("timed", "count"))
    untiered(c, noise_quad_scene(), small, modes=("timed", "count"))
    untiered(c, big_scene("mixed_noise", ((4, 4), 0.4, 4)), BIG[:1], modes=("timed", "count"))


FAMILIES = {f.__name__[len("family_"):]: f for f in (family_spheres_untiered, family_spheres_tiered, family_big_spheres,
                                                     family_quads_untiered, family_quads_tiered, family_big_quads,
                                                     family_noise)}


def child_main(family: str) -> int:
    """In the child: run the family, print its report as one line, exit EXIT_HIP after a HIP error."""
    import torch

    import rtx

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    os.environ["RTX_DEBUG_LAUNCH"] = "1"
    c = Census(family)
    try:
        FAMILIES[family](c)
        out = c.report()
    except Exception as e:
        c.rec.close()
        print(f"{family} stopped in its combination {c.combos}: {type(e).__name__}: {e}", file=sys.stderr)
        hip = (isinstance(e, rtx.RtxError) and e.code == rtx.RTX_ERR_HIP) or "HIP error" in str(e) or "hipError" in str(e)
        return EXIT_HIP if hip else 1
    c.rec.close()
    print(MARK + json.dumps(out))
    return 0


# ---- the GPU tests --------------------------------------------------------------------------------------------------
STOPPED = []  # why no further child is started: a child ended by a signal, its time limit or a HIP error
STARTED = []  # the families whose test ran
RESULTS = {}  # family -> the child's report
CHILD_TIMEOUT_S = 120


def run_family(family: str, module: str = "test_kernel_census", STARTED=STARTED, RESULTS=RESULTS) -> dict:
    """One child process for `family` of `module` (this one, or tests/test_block_census.py with its own STARTED and
    RESULTS; STOPPED is shared: after a fault no child of either module starts)."""
    STARTED.append(family)
    assert not STOPPED, f"not started: {STOPPED[0]}"
    code =(f"import sys; sys.path[:0] = ['raytracer-go_amd', 'tests']; import {module} as t; "
            f"sys.exit(t.child_main({family!r}))")
    env = dict(os.environ, RTX_WATCHDOG_S="10", RTX_DEBUG_LAUNCH="1")
    try:
        res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        STOPPED.append(f"the child of {family} ran into its time limit of {CHILD_TIMEOUT_S} s")
        raise AssertionError(STOPPED[0] + "\n" + str(e.stderr or "")[-4000:])
    if res.returncode < 0 or res.returncode == EXIT_HIP or "illegal memory access" in res.stderr:
        STOPPED.append(f"the child of {family} ended with status {res.returncode}")
    assert res.returncode == 0, f"status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    line = next(ln for ln in res.stdout.splitlines() if ln.startswith(MARK))
    out = RESULTS[family] = json.loads(line[len(MARK):])
    print(f"{family}: {out['combos']} combinations, {len(out['seen'])} kernels with evidence, "
          f"{len(out['launched'])} launched")
    for name, why in sorted(out["missing"].items()):
        print(f"  launched without evidence: {name}  ({why})")
    assert not out["failures"], "\n".join(out["failures"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_family(built, family):
    run_family(family)


@pytest.mark.gpu
def test_every_reachable_kernel_ran(built):
    """The union of the families' kernels seen with evidence is the committed list less UNREACHABLE, and no kernel of
    UNREACHABLE was launched by any of them.  RTX_CENSUS_OUT=<path>: the record (profiles/kernel_census.json)."""
    assert not STOPPED, STOPPED[0]
    lost = [f for f in STARTED if f not in RESULTS]
    assert not lost, f"families without a report: {lost}"
    absent = [f for f in FAMILIES if f not in STARTED]
    if absent:
        pytest.skip(f"families deselected: {absent}")
    want = set(listed()) - set(UNREACHABLE)
    seen, launched = {}, set()
    for family, out in RESULTS.items():
        launched |= set(out["launched"])
        for name, combo in out["seen"].items():
            seen.setdefault(name, {"family": family, "combination": combo})
    assert not launched & set(UNREACHABLE), sorted(launched & set(UNREACHABLE))
    assert not launched - set(listed()), sorted(launched - set(listed()))
    never = sorted(want - set(seen))
    assert not never, f"{len(never)} reachable kernels without evidence:\n" + "\n".join(
        n + ("  (launched)" if n in launched else "") for n in never)
    assert set(seen) == want
    path = os.environ.get("RTX_CENSUS_OUT")
    if path:
        with open(LIB, "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()
        with open(path, "w") as f:
            json.dump({"librtx_sha256": sha, "kernels": len(listed()), "unreachable": len(UNREACHABLE),
                       "seen": {k: seen[k] for k in sorted(seen)}}, f, indent=1)
            f.write("\n")
