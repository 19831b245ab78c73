"""The census of the block kernels: every __global__ function of rtx_trace.hip, rtx_direct.hip, rtx_guides.hip,
rtx_shade.hip and rtx_denoise.hip that librtx.so contains is on a committed list (tests/block_kernels.txt, 66 kernels),
and every one is launched against its reference with evidence that it did work.

  test_list_matches_library              CPU: the library's kernel symbols and the list are the same set; every name parses.
  test_block_scenes_are_what_they_say    CPU: the eight scenes of tests/block_scenes.py (QUADS x FIXED x NOISE) lie on the
                                         intended side of the LDS limit and their window holds misses, grid spheres,
                                         quads, noise-textured hits, and sampled / visible / occluded light samples.
  test_family[<family>]                  GPU: one child process each (RTX_WATCHDOG_S=10, RTX_DEBUG_LAUNCH=1, its own time
                                         limit), in the order of FAMILIES.  Every launch prints "rtx launch: <mangled
                                         name>"; the child attributes the names to the C-ABI call that launched them.
  test_every_block_kernel_ran            the kernels seen with evidence are the list less UNREACHABLE (empty), and no
                                         kernel of UNREACHABLE was launched.

The families, per combination (a kernel counts as seen only when every check of its combination passed; the template
arguments of the names a combination launches must be the scene's class):

  trace    8 scenes x {closest with UV, ANY} x {timed, RTX_TRACE_COUNTERS}.  Rays: the window's camera rays and the
           shadow rays direct_ref.sample gives for their reference first hits.  Every field of every record equals
           trace_ref.walk in float32; the counting calls' hits / node_visits / prim_tests are its sums.  Evidence:
           scene_placement agrees with FIXED; hits and misses both present; on QUADS scenes a quad and a sphere are named.
  shade    8 scenes through test_shade_gpu.loop_equals_oracle (wavefront.render, counting and timed, carried and
           compact): the image is the oracle's, the work counters too.  camera_rays is launched by every render.
           Evidence on NOISE scenes: the shaded first hits on noise-textured primitives take many distinct values.
  guides   8 scenes: test_guides_gpu.reference (camera rays -> trace -> shade, folded by denoise_ref) through same.
           Evidence: first hits on a quad (QUADS) and on the noise-textured Lambertian (NOISE) are among the folded ones.
  direct   8 scenes x {timed, RTX_DIRECT_COUNTERS}: the records equal direct_ref.sample (noise values from the oracle's
           NoiseTexture); n, sampled, visible, rng_draws are its sums; VISIBLE <=> the ANY trace of the record's ray.
           Evidence: sampled, visible and occluded records present; on NOISE scenes a sampled emitter is noise-textured.
  paths    8 scenes x {add_direct, add_mis}, 3 samples: the resolve equals wavefront.render(direct=True, mis=...).
           Evidence: it differs from the plain add(3) resolve, so a light sample did contribute.
  weights  emitter_weights x {timed, counting} on a quad scene and a sphere scene: mis_ref.weight, as
           test_mis_gpu.test_block_equals_reference.  Evidence: some weight lies strictly between 0 and 1.
  denoise  a 41 x 23 synthetic image, 2 and 3 levels: denoise_ref.  Evidence: atrous_level<false>, <true> and
           denoise_prepare are all launched.

guides and paths compare against blocks composed on the GPU, which trace, shade and direct hold to the numpy references:
they start only after those families passed (PREREQ).  If a child ends by a signal, its time limit or a HIP error, no
further child is started (test_kernel_census.STOPPED, shared with that module)."""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys

import pytest

import test_kernel_census as kc

ROOT = kc.ROOT
LIST = os.path.join(ROOT, "tests", "block_kernels.txt")
LIB = kc.LIB

# kernel -> its template arguments, in order
ARGS = {"trace_rays": ("COUNT", "QUADS", "FIXED", "ANY"), "direct_lights": ("COUNT", "QUADS", "FIXED", "NOISE"),
        "direct_paths": ("QUADS", "FIXED", "NOISE", "MIS"), "emitter_weights": ("COUNT",),
        "guide_images": ("QUADS", "FIXED", "NOISE"), "shade_hits": ("COUNT", "NOISE"), "camera_rays": (),
        "atrous_level": ("LAST",), "denoise_prepare": ()}
KERNEL = re.compile(r"^_ZN4rtxd(?:" + "|".join(f"{len(k)}{k}" for k in ARGS) + r")[IE]")
NAME = re.compile(r"^_ZN4rtxd(\d+)([a-z_]+?)(?:I((?:Lb[01]E)+)E)?(?:Ev)?[A-Z].*$")


def parse(name: str) -> dict:
    """kernel = the function's name, and its template arguments by name (0 / 1)."""
    m = NAME.match(name)
    assert m and len(m.group(2)) == int(m.group(1)) and m.group(2) in ARGS, f"not a block kernel: {name}"
    vals = [int(v) for v in re.findall(r"Lb([01])E", m.group(3) or "")]
    assert len(vals) == len(ARGS[m.group(2)]), f"{name}: {len(vals)} template arguments"
    return dict(zip(ARGS[m.group(2)], vals), kernel=m.group(2))


def listed() -> list:
    with open(LIST) as f:
        return [ln.split("\t")[0] for ln in f.read().splitlines() if ln and not ln.startswith("#")]


# kernel name -> the dispatch condition that excludes it for every scene, flag and environment knob.  Empty: each of
# the launchers names only the kernels it launches and every template argument follows a scene property or a flag.
UNREACHABLE = {}


# ---- the CPU tests --------------------------------------------------------------------------------------------------
def test_list_matches_library(built):
    """tests/block_kernels.txt and librtx.so name the same block kernels: 66, every instantiation of ARGS once."""
    want, have = listed(), kc.library_kernels(LIB, KERNEL)
    assert len(want) == len(set(want)), "a kernel is listed twice"
    assert not have - set(want), f"in librtx.so, not in block_kernels.txt: {sorted(have - set(want))}"
    assert not set(want) - have, f"in block_kernels.txt, not in librtx.so: {sorted(set(want) - have)}"
    forms = {tuple(sorted(parse(name).items())) for name in want}
    assert len(forms) == len(want) == sum(2 ** len(a) for a in ARGS.values()) == 66
    assert not set(UNREACHABLE) - set(want), sorted(set(UNREACHABLE) - set(want))


SEED = 0x5EED00D1CE
QUARTER_WAVE = 16


def reference_records(s):
    """(trace_ref.Scene of the caller's tree, pixel-centre camera rays, their reference hits, keys of event 1, the
    reference light samples) of a block scene, without a device."""
    import numpy as np

    import block_scenes as bsc
    import direct_ref
    import rtx
    import trace_ref

    entries = trace_ref.entries_of(s.desc)
    sc = trace_ref.Scene(entries, s.desc)
    rays = bsc.window_rays(s.cam)
    hits = trace_ref.walk(sc, rays, np.float32)
    x0, y0, w, h = bsc.WINDOW
    keys = np.zeros(len(rays), rtx.KEY_DTYPE)
    j, i = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    keys["pixel"], keys["event"] = (j * s.cam.image_width + i).reshape(-1), 1
    light = direct_ref.sample(s.desc, sc, hits.records(uv=True), keys, SEED)
    return sc, rays, hits, keys, light


def light_is_noise(s, light_index):
    """Per light-table index: the emitter's material carries the Perlin texture."""
    import numpy as np

    import direct_ref
    import rtx

    d = s.desc.contents
    tab = direct_ref.lights(s.desc)
    prim = tab["prim"][light_index]
    idx = prim & 0x0FFFFFFF
    mat = np.array([d.quads[int(i)].material if p >> 28 == rtx.RTX_PRIM_QUAD else d.spheres[int(i)].material
                    for p, i in zip(prim, idx)], np.int64)
    return np.isin(mat, s.noise_mats)


def shadow_conditions(s, light):
    """The shadow rays of the records `light` (rtx.DIRECT_DTYPE): sampled, visible and occluded each on a quarter of a
    wave; on a NOISE scene as many sampled records whose emitter carries the noise texture."""
    import rtx

    sampled = (light["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
    visible = (light["flags"] & rtx.RTX_DIRECT_VISIBLE) != 0
    n = {"sampled": int(sampled.sum()), "visible": int(visible.sum()), "occluded": int((sampled & ~visible).sum())}
    if s.noise:
        n["noise emitter"] = int(light_is_noise(s, light["light"][sampled]).sum())
    assert min(n.values()) >= QUARTER_WAVE, (s.name, n)
    return n


def test_block_scenes_are_what_they_say(built):
    """A condition on the inputs of the families, checked without a GPU: each of the eight scenes lies on the intended
    side of the LDS limit, and of the window's 312 pixel-centre camera rays on the caller's tree at least a quarter of a
    wave each misses, first hits a grid sphere, a quad (QUADS) and a noise-textured primitive (NOISE); of the light
    samples at those hits as many are sampled, visible, occluded and (NOISE) drawn on the noise-textured emitter."""
    import big_scenes
    import block_scenes as bsc

    assert len(bsc.CLASSES) == 8
    for quads, big, noise in bsc.CLASSES:
        s = bsc.block_scene(quads, big, noise)
        sc, rays, hits, keys, light = reference_records(s)
        assert len(rays) == 312 and len(rays) % 64 != 0
        n = len(sc.entries)
        assert (n > big_scenes.LIMIT) == big and (big or n < 256), (s.name, n)
        assert (s.desc.contents.n_quads > 0) == quads
        kinds = bsc.first_hit_kinds(s, hits.prim, hits.material)
        need = ["miss", "grid"] + (["quad"] if quads else []) + (["noise"] if noise else [])
        got = {k: int(kinds[k].sum()) for k in kinds}
        print(f"{s.name}: {n} entries, first hits {got}, light samples {shadow_conditions(s, light)}")
        assert all(got[k] >= QUARTER_WAVE for k in need), (s.name, got)
        assert quads or got["quad"] == 0
        assert noise or got["noise"] == 0


# ---- the children ---------------------------------------------------------------------------------------------------
MARK = kc.MARK
# the C-ABI calls whose launches are attributed, and the kernels each may launch
CALLS = {"trace_device": {"trace_rays"}, "trace": {"trace_rays"}, "shade_device": {"shade_hits"}, "shade": {"shade_hits"},
         "guides_device": {"guide_images"}, "guides": {"guide_images"}, "direct_device": {"direct_lights"},
         "direct": {"direct_lights"}, "emitter_weight_device": {"emitter_weights"}, "emitter_weight": {"emitter_weights"},
         "add_direct": {"direct_paths"}, "add_mis": {"direct_paths"}, "camera_rays_device": {"camera_rays"},
         "camera_rays": {"camera_rays"}, "denoise_device": {"atrous_level", "denoise_prepare"},
         "denoise": {"atrous_level", "denoise_prepare"}}


class Blocks:
    """The child's state: the launch recorder around every block entry, the scenes, the running combination."""

    def __init__(self, family, own):
        import numpy as np
        import torch

        import block_scenes as bsc
        import rtx

        self.np, self.torch, self.rtx, self.bsc = np, torch, rtx, bsc
        self.family, self.own = family, own
        self.rec = kc.Recorder()
        self.seen, self.launched, self.missing, self.failures, self.combos = {}, set(), {}, [], 0
        self.devs = {}
        for owner, names in ((rtx.DeviceScene, ("trace_device", "trace", "shade_device", "shade", "guides_device", "guides",
                                                "direct_device", "direct", "emitter_weight_device", "emitter_weight")),
                             (rtx.Accumulator, ("add_direct", "add_mis")),
                             (rtx, ("camera_rays_device", "camera_rays", "denoise_device", "denoise"))):
            for n in names:
                setattr(owner, n, self.wrap(n, getattr(owner, n)))

    def wrap(self, entry, fn):
        inner = self.rec.wrap(fn, lambda out: entry)  # Launch.st: the entry's name

        return inner

    def dev(self, s):
        """(device scene on the caller's tree with every box test, trace_ref.Scene of the same entries)."""
        import trace_ref

        if s.name not in self.devs:
            dev = self.rtx.DeviceScene(s.desc, reference_bvh=True, every_box=True)
            entries = trace_ref.entries_of(s.desc)
            assert dev.export() == entries.tobytes(), "the device walks other entries than trace_ref"
            self.devs[s.name] = (dev, trace_ref.Scene(entries, s.desc))
        return self.devs[s.name]

    def combo(self, label, expect, fn):
        """Run one combination; its launches count only when every check of fn passed and every kernel of the family
        it launched has the template arguments `expect`."""
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
            self.failures.append(f"{label}: {type(e).__name__}: {str(e)[:400]}")
            return
        good = []
        for call in self.rec.calls:
            for name in call.names:
                self.launched.add(name)
                k = parse(name)
                if k["kernel"] not in CALLS[call.st]:
                    self.failures.append(f"{label}: {call.st} launched {name}")
                    return
                if k["kernel"] not in self.own:
                    continue
                wrong = {a: v for a, v in expect.items() if a in k and k[a] != int(v)}
                if wrong:
                    self.failures.append(f"{label}: launched {name}, expected {expect}")
                    return
                good.append(name)
        if not good:
            self.failures.append(f"{label}: no kernel of {sorted(self.own)} was launched")
        for name in good:
            self.seen.setdefault(name, label)

    def report(self):
        self.rtx.device_check(0)
        return {"family": self.family, "combos": self.combos, "seen": self.seen, "launched": sorted(self.launched),
                "missing": {k: v for k, v in self.missing.items() if k not in self.seen}, "failures": self.failures}

    # -- the shared pieces ----------------------------------------------------------------------------------------
    def first_hits(self, s, count=1):
        """(rays, keys, hits with UV) of `count` samples of the window: camera_rays -> trace on the device, the hits
        equal to trace_ref.walk on the same rays."""
        import trace_ref

        np, rtx = self.np, self.rtx
        dev, sc = self.dev(s)
        rays, keys = rtx.camera_rays(s.camera(), SEED, s.region(), 0, count)
        rays, keys = rays.reshape(-1).copy(), keys.reshape(-1).copy()
        hits = dev.trace(rays, rtx.RTX_TRACE_UV)
        want = trace_ref.walk(sc, rays, np.float32).records(uv=True)
        assert hits.tobytes() == want.tobytes(), "the first hits differ from trace_ref.walk"
        return rays, keys, hits


def scene_expect(s):
    return {"QUADS": s.quads, "FIXED": not s.big, "NOISE": s.noise}


def family_trace(c: Blocks):
    import test_trace_gpu as tt
    import trace_ref

    np, rtx = c.np, c.rtx
    for cls in c.bsc.CLASSES:
        s = c.bsc.block_scene(*cls)
        dev, sc = c.dev(s)
        _, cam_rays, _, _, light = reference_records(s)
        shadow_conditions(s, light)
        sampled = (light["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
        rays = np.concatenate([cam_rays, light["ray"][sampled]])
        for any_hit, count in ((0, 0), (0, 1), (1, 0), (1, 1)):

            def run():
                w = trace_ref.walk(sc, rays, np.float32, uv=not any_hit, any_hit=bool(any_hit))
                want = w.records(uv=not any_hit)
                flags = (rtx.RTX_TRACE_ANY if any_hit else rtx.RTX_TRACE_UV) | (rtx.RTX_TRACE_COUNTERS if count else 0)
                got, st = tt.trace(c.torch, dev, rays, flags, stats=True)
                bad = tt.differing(got, want)
                assert bad.size == 0, (len(bad), bad[:8].tolist(), got[bad[:2]], want[bad[:2]])
                sums = (int(w.mask.sum()), int(w.node_visits.sum()), int(w.prim_tests.sum())) if count else (0, 0, 0)
                assert (st.rays, st.hits, st.node_visits, st.prim_tests) == (len(rays),) + sums, (st.as_dict(), sums)
                # evidence
                assert st.scene_placement == (rtx.RTX_SCENE_IN_HBM if s.big else rtx.RTX_SCENE_IN_LDS)
                hit = got["prim"] != rtx.RTX_HIT_NONE
                assert hit.any() and (~hit).any()
                if s.quads:
                    kinds = set((got["prim"][hit] >> 28).tolist())
                    assert {rtx.RTX_PRIM_QUAD, rtx.RTX_PRIM_SPHERE} <= kinds, kinds

            c.combo(f"{s.name} {'any' if any_hit else 'closest+uv'} {'counting' if count else 'timed'}",
                    dict(scene_expect(s), ANY=any_hit, COUNT=count), run)


def family_shade(c: Blocks):
    import test_shade_gpu as tsh

    np = c.np
    for cls in c.bsc.CLASSES:
        s = c.bsc.block_scene(*cls)
        dev, _ = c.dev(s)

        def run():
            tsh.loop_equals_oracle(c.torch, dev, s.desc, s.camera(), 23, s.region())
            rays, keys, hits = c.first_hits(s, c.bsc.SPP)
            got, st = tsh.shade_dev(c.torch, dev, rays, hits, keys, SEED, c.rtx.RTX_SHADE_COUNTERS, stats=True)
            assert got.tobytes() == dev.shade(rays, hits, keys, SEED).tobytes()  # the counting and the timed kernel
            assert st.hits == int((hits["prim"] != c.rtx.RTX_HIT_NONE).sum())
            if s.noise:  # evidence: the noise texture's values reach the shaded records
                k = c.bsc.first_hit_kinds(s, hits["prim"], hits["material"])
                lam, lit = k["noise_lambertian"], k["noise"] & ~k["noise_lambertian"]
                assert lam.sum() >= QUARTER_WAVE and len(np.unique(got["attenuation"][lam][:, 0])) >= QUARTER_WAVE
                assert not lit.any() or len(np.unique(got["emitted"][lit][:, 0])) > 1

        c.combo(s.name, {"NOISE": s.noise}, run)
    names = {parse(n)["kernel"]: n for n in c.launched}
    assert "camera_rays" in names


def family_guides(c: Blocks):
    import test_guides_gpu as tg

    for cls in c.bsc.CLASSES:
        s = c.bsc.block_scene(*cls)
        dev, _ = c.dev(s)

        def run():
            cam, region, n = s.camera(), s.region(), c.bsc.SPP
            want, kind = tg.reference(dev, s.desc, cam, SEED, region, 0, n)
            got, st = tg.guides_dev(c.torch, dev, cam, SEED, region, 0, n, stats=True)
            tg.same(got, want)
            assert st.rays == want.size * n
            tg.same(tg.guides_dev(c.torch, dev, cam, SEED, region, 0, n), want)
            _, _, hits = c.first_hits(s, n)  # evidence: what the folded first hits are
            k = c.bsc.first_hit_kinds(s, hits["prim"], hits["material"])
            assert k["miss"].any() and k["grid"].any()
            assert not s.quads or k["quad"].sum() >= QUARTER_WAVE
            assert not s.noise or k["noise_lambertian"].sum() >= QUARTER_WAVE

        c.combo(s.name, scene_expect(s), run)


def family_direct(c: Blocks):
    import direct_ref
    import test_direct_gpu as td

    np, rtx = c.np, c.rtx
    for cls in c.bsc.CLASSES:
        s = c.bsc.block_scene(*cls)
        dev, sc = c.dev(s)
        for count in (0, 1):

            def run():
                rays, keys, hits = c.first_hits(s, 1)
                want = direct_ref.sample(s.desc, sc, hits, keys, SEED)
                conditions = shadow_conditions(s, want)  # evidence, from the reference's own records
                got, st = td.direct_dev(c.torch, dev, hits, keys, SEED, rtx.RTX_DIRECT_COUNTERS if count else 0, stats=True)
                td.same_records(got, want)
                sums = (conditions["sampled"], conditions["visible"], int(want["rng_draws"].sum())) if count else (0, 0, 0)
                assert (st.n, st.sampled, st.visible, st.rng_draws) == (len(want),) + sums, (st.as_dict(), sums)
                k = np.nonzero(got["flags"] & rtx.RTX_DIRECT_SAMPLED)[0]
                any_hit = td.trace_dev(c.torch, dev, got["ray"][k].copy(), rtx.RTX_TRACE_ANY)
                assert np.array_equal((got["flags"][k] & rtx.RTX_DIRECT_VISIBLE) != 0, any_hit["prim"] == rtx.RTX_HIT_NONE)

            c.combo(f"{s.name} {'counting' if count else 'timed'}", dict(scene_expect(s), COUNT=count), run)


def family_paths(c: Blocks):
    import wavefront

    np = c.np
    for cls in c.bsc.CLASSES:
        s = c.bsc.block_scene(*cls)
        dev, _ = c.dev(s)
        for mis in (0, 1):

            def run():
                cam, region = s.camera(), s.region()
                want = wavefront.render(dev, cam, 29, region, direct=True, mis=bool(mis)).cpu().numpy()
                acc = dev.accumulator(cam, 29, region)
                try:
                    (acc.add_mis if mis else acc.add_direct)(c.bsc.SPP)
                    rgb = acc.resolve()[0]
                    bad = np.argwhere((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=2))
                    assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(rgb[y, x], want[y, x]) for y, x in bad[:3]])
                    acc.reset()
                    acc.add(c.bsc.SPP)
                    plain = acc.resolve()[0]
                    assert (plain.view(np.uint32) != rgb.view(np.uint32)).any(), "no light sample contributed"
                finally:
                    acc.close()

            c.combo(f"{s.name} {'add_mis' if mis else 'add_direct'}", dict(scene_expect(s), MIS=mis), run)


def family_weights(c: Blocks):
    import mis_ref
    import test_mis_gpu as tm

    rtx = c.rtx
    for cls in ((True, False, False), (False, False, False)):
        s = c.bsc.block_scene(*cls)
        dev, _ = c.dev(s)
        rays, keys, hits1 = c.first_hits(s, c.bsc.SPP)
        hits2 = dev.trace(dev.shade(rays, hits1, keys, SEED)["ray"].copy(), rtx.RTX_TRACE_UV)
        want = mis_ref.weight(s.desc, hits1, hits2)
        for count in (0, 1):

            def run():
                got, st = tm.weight_dev(c.torch, dev, hits1, hits2, rtx.RTX_EMITTER_COUNTERS if count else 0, stats=True)
                tm.same_records(got, want)
                weighted = (want["flags"] & rtx.RTX_EMITTER_WEIGHTED) != 0
                assert (st.n, st.weighted) == (len(want), int(weighted.sum()) if count else 0), st.as_dict()
                w = got["weight"][weighted]
                assert ((w > 0) & (w < 1)).any(), "no weight strictly between 0 and 1"  # evidence

            c.combo(f"{s.name} {'counting' if count else 'timed'}", {"COUNT": count}, run)


def family_denoise(c: Blocks):
    import denoise_ref as dr
    import test_denoise_gpu as tdn

    rgb, var, g = dr.synthetic(41023, 41, 23, None)
    for it in (2, 3):

        def run():
            tdn.same(tdn.denoise_dev(c.torch, rgb, var, g, tdn.params(it)), dr.denoise(rgb, var, g, iterations=it))
            kernels = [(parse(n)["kernel"], parse(n).get("LAST")) for call in c.rec.calls for n in call.names]
            assert kernels == [("denoise_prepare", None)] + [("atrous_level", 0)] * (it - 1) + [("atrous_level", 1)], kernels

        c.combo(f"41x23 {it} levels", {}, run)


FAMILIES = {"trace": (family_trace, {"trace_rays"}), "shade": (family_shade, {"shade_hits", "camera_rays"}),
            "guides": (family_guides, {"guide_images"}), "direct": (family_direct, {"direct_lights"}),
            "paths": (family_paths, {"direct_paths"}), "weights": (family_weights, {"emitter_weights"}),
            "denoise": (family_denoise, {"atrous_level", "denoise_prepare"})}
PREREQ = {"guides": ("trace", "shade"), "paths": ("trace", "shade", "direct"), "weights": ("trace", "shade")}


def child_main(family: str) -> int:
    """In the child: run the family, print its report as one line, exit EXIT_HIP after a HIP error."""
    import torch

    import rtx

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    os.environ["RTX_DEBUG_LAUNCH"] = "1"
    fn, own = FAMILIES[family]
    c = Blocks(family, own)
    try:
        fn(c)
        out = c.report()
    except Exception as e:
        c.rec.close()
        print(f"{family} stopped in its combination {c.combos}: {type(e).__name__}: {e}", file=sys.stderr)
        hip = (isinstance(e, rtx.RtxError) and e.code == rtx.RTX_ERR_HIP) or "HIP error" in str(e) or "hipError" in str(e)
        return kc.EXIT_HIP if hip else 1
    c.rec.close()
    print(MARK + json.dumps(out))
    return 0


# ---- the GPU tests --------------------------------------------------------------------------------------------------
STARTED = []  # the families whose test ran
RESULTS = {}  # family -> the child's report


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_family(built, family):
    for need in PREREQ.get(family, ()):
        if need in STARTED and not (need in RESULTS and not RESULTS[need]["failures"]):
            STARTED.append(family)  # (without a report: test_every_block_kernel_ran fails too)
            raise AssertionError(f"{family} compares against blocks that {need} holds to their references, and {need} did not pass")
    kc.run_family(family, "test_block_census", STARTED, RESULTS)


@pytest.mark.gpu
def test_every_block_kernel_ran(built):
    """The union of the families' kernels seen with evidence is the committed list less UNREACHABLE, and no kernel of
    UNREACHABLE was launched by any of them.  RTX_BLOCK_CENSUS_OUT=<path>: the record (profiles/block_census.json)."""
    assert not kc.STOPPED, kc.STOPPED[0]
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
    assert not never, f"{len(never)} block kernels without evidence:\n" + "\n".join(
        n + ("  (launched)" if n in launched else "") for n in never)
    assert set(seen) == want
    path = os.environ.get("RTX_BLOCK_CENSUS_OUT")
    if path:
        with open(LIB, "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()
        record = {}
        if os.path.exists(path):  # (keeps what scripts wrote beside the census: not_launched_before)
            with open(path) as f:
                record = json.load(f)
        record.update({"librtx_sha256": sha, "kernels": len(listed()), "unreachable": len(UNREACHABLE),
                       "families": {f: {"combinations": RESULTS[f]["combos"], "kernels": len(RESULTS[f]["seen"])} for f in RESULTS},
                       "seen": {k: seen[k] for k in sorted(seen)}})
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
