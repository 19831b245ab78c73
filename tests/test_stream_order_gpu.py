"""Every entry of include/rtx.h that takes a `void* hip_stream`, held to its ordering contract on NON-BLOCKING side
streams (tests/stream_order.py has the recipe).

Per entry (CASES, one key per entry: tests/test_stream_order.py holds the table to the header):
  (a) the bytes a call produces on a side stream, with its inputs arriving and its outputs poisoned behind a gate,
      equal the bytes of the same sequence on stream 0, and the PAD bytes keep their poison;
  (b) a call the header says returns after enqueueing returns while the gate is still running — a gate that has
      finished by then FAILS the case as vacuous;
  (c) a call with stats (or a noisy count, or rtx_encode_ppm_device) has synchronised its stream on return — the gate's
      event has completed — and its samples / rays / records are right.
An accumulator's passes have no input in the caller's memory, so the gate cannot hold their input back: each pass
case puts a region render on the stream first (the pass then waits for it through the device's render event, whatever
stream it runs on) and resolves on the stream straight after the pass.

Across streams (two side streams, no host synchronise between the enqueues): the scratch handed from render to render
between scenes and within one, independent accumulators interleaved, the blocking host-pointer readers after
side-stream passes, an adaptive pass on another stream than the last pass's, a pass straight after rtx_accum_reset and
rtx_accum_create, scratch growth, and destroy with work in flight.  The expected bytes are the serial stream-0 ones,
themselves pinned to the oracle and the references by the other GPU tests.

The gate's length is measured, not guessed: at least 20 times the warm host time of the slowest enqueue-only call and
at least 5 ms, at most 50 ms; the gates are made twice that minimum (stream_order.GATE_MARGIN).  Measured on an MI355X
(profiles/stream_order.json): slowest enqueue-only call 0.030 ms on the host (the preview; the tiered region render
0.029 ms, 0.06 ms in other runs), so the 5 ms floor applies: gate 10.04 ms, 138 in-place adds on 256 MiB."""
import json
import os

import numpy as np
import pytest

import rtx
import stream_order as so

pytestmark = pytest.mark.gpu

SEED = 0x57BEA4
REL_TOL = 0.5  # at which the reference closes some of the window's 15 tiles and not all (after 2 samples: 7, after 4: 13)
PAD = 7       # records after the last the call may write (the batch and guide tests' PAD)
PAD_IMG = 7 * 12  # bytes after an image (test_denoise_gpu's PAD)
WINDOW = (36, 20)  # 4.5 x 2.5 tiles of 8 x 8: ragged on both edges; 720 pixels: 11.25 waves
SPP = 3
UV, ANY = rtx.RTX_TRACE_UV, rtx.RTX_TRACE_ANY
MEASURED = {}


class Scene:
    """One of the two scenes with its window: random_spheres, whose camera sits in the near region (renders and passes
    take the tiered launch sequence chunk_start -> near -> far -> redo), and cornell_box (quads and emitters, the plain
    launch with its hipMemsetAsync of the counters)."""

    def __init__(self, name):
        self.name = name
        self.host = rtx.HostScene(name, seed=1)
        self.dev = rtx.DeviceScene(self.host.desc)
        if name == "random_spheres":
            self.cam_of = lambda n: self.host.camera(width=48, spp=n, depth=50)
            self.region = rtx.Region(5, 3, *WINDOW, 0, 1)
            self.batch_cam, self.batch_region = self.host.camera(width=64, spp=1, depth=50), rtx.Region(0, 0, 64, 36, 0, 1)
            self.key = ("random_spheres", 1, 48, 50)
        else:
            self.cam_of = lambda n: self.host.camera(width=64, spp=n, depth=8)
            self.region = rtx.Region(12, 20, *WINDOW, 0, 1)
            self.batch_cam, self.batch_region = self.host.camera(width=64, spp=1, depth=8), rtx.Region(0, 14, 64, 36, 0, 1)
            self.key = ("cornell_box", 1, 64, 8)
        self.cam = self.cam_of(SPP)
        self.tiered = name == "random_spheres"
        self.pixels = WINDOW[0] * WINDOW[1]
        assert rtx.region_rows(self.region) == WINDOW[1]
        assert rtx.walk_near_region(self.host.desc, self.cam)[1] == self.tiered


class World:
    """What the module shares: torch, the two side streams, the scenes, the batches, the gates."""

    def __init__(self, torch):
        self.torch = torch
        self.s1, self.s2 = so.side_stream(torch), so.side_stream(torch)
        assert self.s1.cuda_stream != self.s2.cuda_stream
        self.scenes, self._batches = {}, {}
        self.gate1 = self.gate2 = None

    def scene(self, name) -> Scene:
        if name not in self.scenes:
            self.scenes[name] = Scene(name)
        return self.scenes[name]

    def batch(self, name):
        """64 x 36 camera rays plus 200 incoherent rays of a scene, their keys, their closest hits (with u, v), and the
        closest hits of their bounces: produced on stream 0 by the blocking host entries, as the batch tests do."""
        if name not in self._batches:
            import trace_sets as ts
            sc = self.scene(name)
            rays, keys = rtx.camera_rays(sc.batch_cam, SEED, sc.batch_region, 0, 1)
            extra = (ts.incoherent_rays(200, 101, ts.scene("random_spheres").ref) if name == "random_spheres"
                     else ts.ray_set("cornell").rays[:200])
            ek = np.zeros(len(extra), rtx.KEY_DTYPE)
            ek["pixel"], ek["sample"], ek["event"] = 100000 + np.arange(len(extra)), np.arange(len(extra)) % 5, 1
            rays, keys = np.concatenate([rays.reshape(-1), extra]), np.concatenate([keys.reshape(-1), ek])
            assert len(rays) == 64 * 36 + 200 and len(rays) % 64 != 0
            hits = sc.dev.trace(rays, UV)
            bounce = sc.dev.shade(rays, hits, keys, SEED)
            hits2 = sc.dev.trace(bounce["ray"].copy(), UV)
            assert (hits["prim"] != rtx.RTX_HIT_NONE).sum() > 1000
            self._batches[name] = dict(rays=rays, keys=keys, hits=hits, hits2=hits2)
        return self._batches[name]


class Spec:
    """One case: the arguments of stream_order.run_on_side_stream, and what to hold the call's return value to."""

    def __init__(self, call, inputs=(), outputs=(), enqueue_only=True, fresh=None, before=None, after=None, check=None,
                 summary=None, keep=()):
        self.call, self.inputs, self.outputs, self.enqueue_only = call, list(inputs), list(outputs), enqueue_only
        self.fresh, self.before, self.after, self.check, self.keep = fresh, before, after, check, keep
        self.summary = summary or (lambda r: None)
        self.expected = self.summary0 = self.host_s = None

    def args(self):
        return dict(fresh=self.fresh, before=self.before, after=self.after)


def staged_input(w, a):
    """(buffer the call reads, staged real bytes): the bytes reach the buffer only behind the gate."""
    staged = so.device_bytes(w.torch, a)
    return w.torch.empty_like(staged), staged


def image_out(w, pixels, floats=3):
    return so.poisoned(w.torch, pixels * floats * 4, PAD_IMG)


# ---- the cases, one builder per entry ---------------------------------------------------------------------------
def render_region(w, scene, stats):
    sc = w.scene(scene)
    out = image_out(w, sc.pixels)

    def check(st):
        assert (st is not None) == stats
        if stats:
            assert st.samples == sc.pixels * SPP and st.sample_chunks == 1 and st.kernel_ms > 0
            assert bool(st.walk_layout & rtx.RTX_LAYOUT_TIERED) == sc.tiered

    return Spec(lambda s: sc.dev.render_region(sc.cam, SEED, sc.region, out.data_ptr(), s, timed=stats),
                outputs=[(out, sc.pixels * 12)], enqueue_only=not stats, check=check)


def encode_ppm(w):
    """37 x 5 with a NaN and a channel above 1 in it; the call always synchronises its stream."""
    wd, ht = 37, 5
    rgb = np.random.default_rng(375).random((ht, wd, 3), dtype=np.float32)
    rgb[2, 17, 1], rgb[4, 36, 2], rgb[0, 0, 0] = np.nan, 1.75, 0.0
    buf, staged = staged_input(w, rgb)
    cap = int(rtx.load().rtx_ppm_max_bytes(wd, ht))
    text = so.poisoned(w.torch, cap, 64)

    def check(n):
        assert len(f"P3\n{wd} {ht}\n255\n") + wd * ht * 6 <= n <= cap

    # (the whole capacity is compared: what the encoder leaves alone past the text is poison on either stream)
    return Spec(lambda s: rtx.encode_ppm_device(buf.data_ptr(), wd, ht, text.data_ptr(), cap, s), [(buf, staged)],
                [(text, cap)], enqueue_only=False, check=check, summary=lambda n: n)


def pass_case(w, scene, kind, stats):
    """rtx_accum_add / _adaptive / _direct / _mis: on the stream, a region render, a first pass of 2 samples, THE CALL
    (1 sample), then the resolve (and the count map) that shows what the pass left."""
    sc = w.scene(scene)
    acc = sc.dev.accumulator(sc.cam, SEED, sc.region)
    tmp = image_out(w, sc.pixels)
    rgb, var = image_out(w, sc.pixels), image_out(w, sc.pixels)
    counts = so.poisoned(w.torch, sc.pixels * 4, PAD * 4)

    def add(count, s, want_stats):
        if kind == "plain":
            return acc.add(count, s, stats=want_stats)
        if kind == "adaptive":
            return acc.add_adaptive(count, REL_TOL, 1, s, stats=want_stats)
        return (acc.add_direct if kind == "direct" else acc.add_mis)(count, s, stats=want_stats)

    def before(s):
        sc.dev.render_region(sc.cam, SEED + 1, sc.region, tmp.data_ptr(), s)
        add(2, s, False)

    def after(s):
        assert acc.samples == 3
        acc.resolve_device(rgb.data_ptr(), var.data_ptr(), REL_TOL, s)
        acc.sample_counts_device(counts.data_ptr(), s)

    def check(r):
        st, ad = r if kind == "adaptive" else (r, None)
        assert (st is not None) == stats
        if not stats:
            return
        if kind == "adaptive":
            assert 0 < ad.open_tiles <= ad.tiles == 15 and st.samples == ad.open_pixels
        else:
            assert st.samples == sc.pixels
        assert st.kernel_ms > 0
        if kind in ("plain", "adaptive"):
            assert bool(st.walk_layout & rtx.RTX_LAYOUT_TIERED) == sc.tiered

    def summary(r):
        ad = r[1] if kind == "adaptive" else None
        return (int(ad.open_tiles), int(ad.open_pixels)) if ad is not None else None

    return Spec(lambda s: add(1, s, stats), outputs=[(rgb, sc.pixels * 12), (var, sc.pixels * 12), (counts, sc.pixels * 4)],
                enqueue_only=not stats, fresh=acc.reset, before=before, after=after, check=check, summary=summary,
                keep=(acc, tmp))


def reader_case(w, which):
    """rtx_accum_resolve_device (with and without the noisy count), _sample_counts_device and _preview_device on an
    accumulator whose passes went onto the same stream behind the same gate."""
    sc = w.scene("random_spheres")
    acc = sc.dev.accumulator(sc.cam, SEED, sc.region)
    adaptive = which == "counts"  # (a count map that is not one constant)

    def before(s):
        for count in (2, 1):
            if adaptive:
                acc.add_adaptive(count, REL_TOL, 1, s, stats=False)
            else:
                acc.add(count, s)

    if which in ("resolve", "resolve-noisy"):
        rgb, var = image_out(w, sc.pixels), image_out(w, sc.pixels)
        noisy = which == "resolve-noisy"

        def check(n):
            assert (n is not None) == noisy and (n is None or 0 < n < sc.pixels)

        return Spec(lambda s: acc.resolve_device(rgb.data_ptr(), var.data_ptr(), REL_TOL, s, count_noisy=noisy),
                    outputs=[(rgb, sc.pixels * 12), (var, sc.pixels * 12)], enqueue_only=not noisy, fresh=acc.reset,
                    before=before, check=check, summary=lambda n: n, keep=(acc,))
    if which == "counts":
        counts = so.poisoned(w.torch, sc.pixels * 4, PAD * 4)
        return Spec(lambda s: acc.sample_counts_device(counts.data_ptr(), s), outputs=[(counts, sc.pixels * 4)],
                    fresh=acc.reset, before=before, keep=(acc,))
    out = image_out(w, sc.pixels)
    return Spec(lambda s: acc.preview_device(out.data_ptr(), 2, None, s), outputs=[(out, sc.pixels * 12)], fresh=acc.reset,
                before=before, keep=(acc,))


def trace(w, scene, flags, stats):
    sc, b = w.scene(scene), w.batch(scene)
    n = len(b["rays"])
    rays = staged_input(w, b["rays"])
    hits = so.poisoned(w.torch, n * 48, PAD * 48)

    def check(st):
        assert (st is not None) == stats and (st is None or (st.rays == n and st.kernel_ms > 0))

    return Spec(lambda s: sc.dev.trace_device(rays[0].data_ptr(), n, hits.data_ptr(), flags, s, stats), [rays],
                [(hits, n * 48)], enqueue_only=not stats, check=check)


def camera_rays(w):
    sc = w.scene("random_spheres")
    n = sc.pixels * SPP
    rays, keys = so.poisoned(w.torch, n * 32, PAD * 32), so.poisoned(w.torch, n * 16, PAD * 16)
    return Spec(lambda s: rtx.camera_rays_device(sc.cam, SEED, sc.region, 0, SPP, rays.data_ptr(), keys.data_ptr(), s),
                outputs=[(rays, n * 32), (keys, n * 16)])


def shade(w, stats):
    sc, b = w.scene("random_spheres"), w.batch("random_spheres")
    n = len(b["rays"])
    ins = [staged_input(w, b[k]) for k in ("rays", "hits", "keys")]
    out = so.poisoned(w.torch, n * 64, PAD * 64)

    def check(st):
        assert (st is not None) == stats and (st is None or (st.n == n and st.kernel_ms > 0))

    return Spec(lambda s: sc.dev.shade_device(SEED, *[i[0].data_ptr() for i in ins], n, out.data_ptr(), 0, s, stats), ins,
                [(out, n * 64)], enqueue_only=not stats, check=check)


def guides(w, scene, stats):
    sc = w.scene(scene)
    out = so.poisoned(w.torch, sc.pixels * 32, PAD * 32)

    def check(st):
        assert (st is not None) == stats and (st is None or (st.rays == sc.pixels * SPP and st.kernel_ms > 0))

    return Spec(lambda s: sc.dev.guides_device(sc.cam, SEED, sc.region, 0, SPP, out.data_ptr(), s, stats),
                outputs=[(out, sc.pixels * 32)], enqueue_only=not stats, check=check)


def denoise(w):
    """The filter on the window's resolved image, variance and guides (made on stream 0 by the blocking entries)."""
    sc = w.scene("random_spheres")
    acc = sc.dev.accumulator(sc.cam, SEED, sc.region)
    acc.add(SPP)
    w.torch.cuda.synchronize()
    rgb, var, _ = acc.resolve()
    acc.close()
    g = sc.dev.guides(sc.cam, SEED, sc.region, 0, SPP)
    ins = [staged_input(w, a) for a in (rgb, var, g)]
    wd, ht = WINDOW
    wb = rtx.denoise_workspace_bytes(wd, ht)
    out, work = image_out(w, sc.pixels), so.poisoned(w.torch, wb, 64)
    return Spec(lambda s: rtx.denoise_device(*[i[0].data_ptr() for i in ins], wd, ht, out.data_ptr(), work.data_ptr(), wb,
                                             None, s), ins, [(out, sc.pixels * 12), (work, wb)])


def direct(w, stats):
    sc, b = w.scene("cornell_box"), w.batch("cornell_box")
    n = len(b["hits"])
    ins = [staged_input(w, b[k]) for k in ("hits", "keys")]
    out = so.poisoned(w.torch, n * 64, PAD * 64)

    def check(st):
        assert (st is not None) == stats and (st is None or (st.n == n and st.kernel_ms > 0))

    return Spec(lambda s: sc.dev.direct_device(SEED, *[i[0].data_ptr() for i in ins], n, out.data_ptr(), 0, s, stats), ins,
                [(out, n * 64)], enqueue_only=not stats, check=check)


def emitter_weight(w, stats):
    sc, b = w.scene("cornell_box"), w.batch("cornell_box")
    n = len(b["hits"])
    ins = [staged_input(w, b[k]) for k in ("hits", "hits2")]
    out = so.poisoned(w.torch, n * 16, PAD * 16)

    def check(st):
        assert (st is not None) == stats and (st is None or (st.n == n and st.kernel_ms > 0))

    return Spec(lambda s: sc.dev.emitter_weight_device(*[i[0].data_ptr() for i in ins], n, out.data_ptr(), 0, s, stats), ins,
                [(out, n * 16)], enqueue_only=not stats, check=check)


def both(builder, *scenes):
    """{variant: builder} of a builder(w, scene, stats): every scene enqueue-only, the first also with stats."""
    v = {sc: (lambda w, sc=sc: builder(w, sc, False)) for sc in scenes}
    v[scenes[0] + "-stats"] = lambda w: builder(w, scenes[0], True)
    return v


def stats_too(builder):
    return {"enqueue": lambda w: builder(w, False), "stats": lambda w: builder(w, True)}


# entry of rtx.h -> (its wrapper in rtx.py, {variant: builder(world) -> Spec})
CASES = {
    "rtx_render_region_device": ("DeviceScene.render_region", {
        **both(render_region, "random_spheres", "cornell_box"), "cornell_box-stats": lambda w: render_region(w, "cornell_box", True)}),
    "rtx_encode_ppm_device": ("encode_ppm_device", {"sync": encode_ppm}),
    "rtx_accum_add": ("Accumulator.add", both(lambda w, sc, st: pass_case(w, sc, "plain", st), "random_spheres", "cornell_box")),
    "rtx_accum_add_adaptive": ("Accumulator.add_adaptive", both(lambda w, sc, st: pass_case(w, sc, "adaptive", st), "random_spheres")),
    "rtx_accum_add_direct": ("Accumulator.add_direct", both(lambda w, sc, st: pass_case(w, sc, "direct", st), "cornell_box")),
    "rtx_accum_add_mis": ("Accumulator.add_mis", both(lambda w, sc, st: pass_case(w, sc, "mis", st), "cornell_box")),
    "rtx_accum_resolve_device": ("Accumulator.resolve_device", {"enqueue": lambda w: reader_case(w, "resolve"),
                                                                "noisy": lambda w: reader_case(w, "resolve-noisy")}),
    "rtx_accum_sample_counts_device": ("Accumulator.sample_counts_device", {"adaptive": lambda w: reader_case(w, "counts")}),
    "rtx_accum_preview_device": ("Accumulator.preview_device", {"enqueue": lambda w: reader_case(w, "preview")}),
    "rtx_trace_device": ("DeviceScene.trace_device", {
        "random_spheres-closest": lambda w: trace(w, "random_spheres", UV, False),
        "random_spheres-any": lambda w: trace(w, "random_spheres", ANY, False),
        "cornell_box-closest": lambda w: trace(w, "cornell_box", UV, False),
        "cornell_box-any": lambda w: trace(w, "cornell_box", ANY, False),
        "random_spheres-stats": lambda w: trace(w, "random_spheres", UV, True)}),
    "rtx_camera_rays_device": ("camera_rays_device", {"window": camera_rays}),
    "rtx_shade_device": ("DeviceScene.shade_device", stats_too(shade)),
    "rtx_guides_device": ("DeviceScene.guides_device", both(guides, "random_spheres", "cornell_box")),
    "rtx_denoise_device": ("denoise_device", {"window": denoise}),
    "rtx_direct_device": ("DeviceScene.direct_device", stats_too(direct)),
    "rtx_emitter_weight_device": ("DeviceScene.emitter_weight_device", stats_too(emitter_weight)),
}
CASE_IDS = [f"{entry}-{variant}" for entry, (_, variants) in CASES.items() for variant in variants]


@pytest.fixture(scope="module")
def world(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    w = World(torch)
    yield w
    so.destroy_streams(torch)


@pytest.fixture(scope="module")
def plan(world):
    """Step 1 of the recipe for every case, once: the sequence on stream 0 twice (the first run uploads tables and
    layouts and grows the scratch; the second gives the expected bytes and the warm host time of the call), then the
    gates, sized from the slowest enqueue-only call."""
    w, torch = world, world.torch
    specs = {}
    for entry, (_, variants) in CASES.items():
        for variant, builder in variants.items():
            spec = builder(w)
            first = so.on_default_stream(torch, spec.call, spec.inputs, spec.outputs, **spec.args())
            run = so.on_default_stream(torch, spec.call, spec.inputs, spec.outputs, **spec.args())
            assert first.outputs == run.outputs, f"{entry}-{variant}: two runs on stream 0 differ"
            assert all((np.frombuffer(o, np.uint8) != so.POISON).any() for o in run.outputs)
            spec.expected, spec.summary0, spec.host_s = run.outputs, spec.summary(run.result), run.host_s
            specs[f"{entry}-{variant}"] = spec
    slow = max((s.host_s, k) for k, s in specs.items() if s.enqueue_only)
    with torch.cuda.stream(w.s1):  # the side streams' first launches (code objects, the allocator's pools)
        so.poisoned(torch, 64, 0).clone()
    with torch.cuda.stream(w.s2):
        so.poisoned(torch, 64, 0).clone()
    torch.cuda.synchronize()
    w.gate1 = so.Gate(torch).calibrate(min(so.GATE_MAX_MS, so.GATE_MARGIN * so.gate_target_ms(slow[0])))
    w.gate2 = w.gate1.like()
    MEASURED.update(slowest_enqueue_only_call=slow[1], slowest_enqueue_only_call_host_ms=slow[0] * 1e3,
                    gate_target_ms=so.gate_target_ms(slow[0]), gate_ms=w.gate1.measured_ms, gate_reps=w.gate1.reps,
                    gate_ms_per_rep=w.gate1.ms_per_rep,
                    host_ms={k: round(s.host_s * 1e3, 4) for k, s in specs.items()})
    print(f"stream order: slowest enqueue-only call {slow[1]} {slow[0] * 1e3:.3f} ms on the host; gate "
          f"{w.gate1.measured_ms:.2f} ms ({w.gate1.reps} adds)")
    return specs


def test_every_entry_has_a_case():
    assert len(CASES) == 16 and all(variants for _, variants in CASES.values())


@pytest.mark.parametrize("case", CASE_IDS)
def test_entry_on_a_side_stream(world, plan, case):
    spec = plan[case]
    run = so.run_on_side_stream(world.torch, world.s1, world.gate1, spec.call, spec.inputs, spec.outputs,
                                expected=spec.expected, enqueue_only=spec.enqueue_only, **spec.args())
    if spec.check:
        spec.check(run.result)
    assert spec.summary(run.result) == spec.summary0


def test_a_pass_equals_the_one_shot_render(plan):
    """What the pass cases' stream-0 bytes are: 2 + 1 samples resolve to the one-shot render at 3."""
    for scene in ("random_spheres", "cornell_box"):
        assert plan[f"rtx_accum_add-{scene}"].expected[0] == plan[f"rtx_render_region_device-{scene}"].expected[0]


def test_the_gate_is_long_enough(plan):
    """The measured gate against the measured host time (and the measurement written out when asked for)."""
    m = MEASURED
    assert m["gate_ms"] >= m["gate_target_ms"] >= so.GATE_MIN_MS
    assert m["gate_target_ms"] == so.GATE_MAX_MS or m["gate_ms"] >= so.GATE_HOST_FACTOR * m["slowest_enqueue_only_call_host_ms"]
    path = os.environ.get("RTX_STREAM_ORDER_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(m, f, indent=1)


# ---- across streams ---------------------------------------------------------------------------------------------
def serial_render(w, sc, spp, seed):
    """The bytes of a region render on stream 0, waited for."""
    out = image_out(w, sc.pixels)
    sc.dev.render_region(sc.cam_of(spp), seed, sc.region, out.data_ptr(), 0)
    w.torch.cuda.synchronize()
    return out.cpu().numpy()[: sc.pixels * 12].tobytes()


def enqueue_render(w, sc, spp, seed, stream):
    """A region render on `stream` into a buffer poisoned on that stream; nothing is waited for."""
    with w.torch.cuda.stream(stream):
        out = image_out(w, sc.pixels)
    sc.dev.render_region(sc.cam_of(spp), seed, sc.region, out.data_ptr(), stream.cuda_stream)
    return out


def enqueue_resolve(w, acc, sc, stream):
    with w.torch.cuda.stream(stream):
        out = image_out(w, sc.pixels)
    acc.resolve_device(out.data_ptr(), 0, 0.0, stream.cuda_stream)
    return out


def image_bytes(sc, t):
    got = t.cpu().numpy()
    assert (got[sc.pixels * 12:] == so.POISON).all()
    return got[: sc.pixels * 12].tobytes()


def start_together(w, times=1):
    """Both side streams behind one gate: S1 runs it, S2 waits for its event (the caller's own ordering: S2 on S1,
    never the other way round), so work enqueued on the two streams becomes runnable at the same moment and nothing but
    the library's own events orders it.  Returns the gate's event."""
    torch = w.torch
    default = torch.cuda.current_stream()
    w.s1.wait_stream(default)
    w.s2.wait_stream(default)
    for _ in range(times):
        ev = w.gate1.enqueue(w.s1)
    w.s2.wait_event(ev)
    return ev


def finish(w, ev, enqueue_only=True):
    pending = not ev.query()
    w.s1.synchronize()
    w.s2.synchronize()
    if enqueue_only:
        assert pending, "vacuous: the gate had finished before the last enqueue returned"


@pytest.mark.parametrize("second", ["cornell_box", "random_spheres"], ids=["between-scenes", "within-one-scene"])
def test_scratch_handed_from_stream_to_stream(world, plan, second):
    """A, B, A', B' on S1, S2, S1, S2: the device's one sample scratch (and, within one scene, its counters and unit
    queue) goes from render to render through Scratch::last alone."""
    w = world
    a, b = w.scene("random_spheres"), w.scene(second)
    jobs = [(a, SEED + 10, w.s1), (b, SEED + 11, w.s2), (a, SEED + 12, w.s1), (b, SEED + 13, w.s2)]
    want = [serial_render(w, sc, SPP, seed) for sc, seed, _ in jobs]
    assert len(set(want)) == 4
    ev = start_together(w)
    outs = [enqueue_render(w, sc, SPP, seed, st) for sc, seed, st in jobs]
    finish(w, ev)
    for i, ((sc, _, _), out) in enumerate(zip(jobs, outs)):
        assert image_bytes(sc, out) == want[i], f"render {i} differs from the serial render"


def test_independent_accumulators_interleave(world, plan):
    """Two accumulators of one scene on S1 and S2, passes 3, 2, 1 and 1, 2, 3 interleaved, each resolved on its own
    stream: both are the one-shot render at 6 samples."""
    w = world
    sc = w.scene("random_spheres")
    want = serial_render(w, sc, 6, SEED)
    a1, a2 = (sc.dev.accumulator(sc.cam_of(6), SEED, sc.region) for _ in range(2))
    w.torch.cuda.synchronize()
    ev = start_together(w, times=2)
    for c1, c2 in ((3, 1), (2, 2), (1, 3)):
        a1.add(c1, w.s1.cuda_stream)
        a2.add(c2, w.s2.cuda_stream)
    o1, o2 = enqueue_resolve(w, a1, sc, w.s1), enqueue_resolve(w, a2, sc, w.s2)
    finish(w, ev)
    assert image_bytes(sc, o1) == want and image_bytes(sc, o2) == want
    a1.close()
    a2.close()


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_blocking_readers_after_side_stream_passes(world, plan, adaptive):
    """The host-pointer twins run "after every render enqueued on the device so far": no synchronise by the caller
    between the passes on S1, still behind their gate, and rtx_accum_resolve, _sample_counts, _ppm and _preview."""
    w = world
    sc = w.scene("random_spheres")
    acc = sc.dev.accumulator(sc.cam, SEED, sc.region)

    def passes(stream):
        for count in (2, 1):
            if adaptive:
                acc.add_adaptive(count, REL_TOL, 1, stream, stats=False)
            else:
                acc.add(count, stream)

    def read():
        rgb, var, noisy = acc.resolve(REL_TOL)
        return rgb.tobytes(), var.tobytes(), noisy, acc.sample_counts().tobytes(), acc.ppm(), acc.preview(2).tobytes()

    passes(0)
    w.torch.cuda.synchronize()
    want = read()
    for reader in range(4):  # each reader first after the passes once
        acc.reset()
        w.s1.wait_stream(w.torch.cuda.current_stream())
        w.gate1.enqueue(w.s1)
        passes(w.s1.cuda_stream)
        if reader == 0:
            rgb, var, noisy = acc.resolve(REL_TOL)
            got = (rgb.tobytes(), var.tobytes(), noisy)
            assert got == want[:3]
        elif reader == 1:
            assert acc.sample_counts().tobytes() == want[3]
        elif reader == 2:
            assert acc.ppm() == want[4]
        else:
            assert acc.preview(2).tobytes() == want[5]
        assert read() == want
    if adaptive:
        assert len(set(np.frombuffer(want[3], np.uint32).tolist())) > 1  # some tiles closed
    acc.close()


def test_adaptive_pass_on_another_stream(world, plan):
    """4 adaptive samples on S1, S2.wait_stream(S1) by the caller (the header's rule), 4 more on S2, the count map and
    the resolve on S2: the selection, the counts and the image are tests/adaptive_ref.py's."""
    import accum_ref
    import adaptive_ref

    w = world
    sc = w.scene("random_spheres")
    cam = sc.cam_of(8)
    col = accum_ref.sample_colours(sc.key, sc.host.desc, cam, SEED, sc.region, 8)
    acc = sc.dev.accumulator(cam, SEED, sc.region)
    ref = adaptive_ref.simulate(col, acc.tile_shape, (4, 4), REL_TOL, 1)
    assert 0 < ref.passes[1][0] < 15, "the reference closes some tiles and not all"
    w.torch.cuda.synchronize()
    w.s1.wait_stream(w.torch.cuda.current_stream())
    ev = w.gate1.enqueue(w.s1)
    acc.add_adaptive(4, REL_TOL, 1, w.s1.cuda_stream, stats=False)
    w.s2.wait_stream(w.s1)
    acc.add_adaptive(4, REL_TOL, 1, w.s2.cuda_stream, stats=False)
    with w.torch.cuda.stream(w.s2):
        counts = so.poisoned(w.torch, sc.pixels * 4, PAD * 4)
        rgb, var = image_out(w, sc.pixels), image_out(w, sc.pixels)
    acc.sample_counts_device(counts.data_ptr(), w.s2.cuda_stream)
    acc.resolve_device(rgb.data_ptr(), var.data_ptr(), REL_TOL, w.s2.cuda_stream)
    finish(w, ev)
    want_rgb, want_var, _ = ref.resolved(REL_TOL)
    got = counts.cpu().numpy()
    assert (got[sc.pixels * 4:] == so.POISON).all()
    assert got[: sc.pixels * 4].tobytes() == ref.counts.tobytes()
    assert image_bytes(sc, rgb) == want_rgb.tobytes() and image_bytes(sc, var) == want_var.tobytes()
    acc.close()


def test_a_pass_straight_after_reset_and_create(world, plan):
    """rtx_accum_reset ("Blocking") and rtx_accum_create ("allocates and zeroes") zero S and Q with host memsets on the
    null stream, which a non-blocking stream does not wait for: the pass that follows at once on S1, with no
    synchronise, must find them zeroed."""
    w = world
    sc = w.scene("random_spheres")
    want = serial_render(w, sc, SPP, SEED)
    acc = sc.dev.accumulator(sc.cam, SEED, sc.region)
    acc.add(2, w.s1.cuda_stream)
    acc.add(1, w.s1.cuda_stream)
    acc.reset()
    acc.add(SPP, w.s1.cuda_stream)
    out = enqueue_resolve(w, acc, sc, w.s1)
    fresh = sc.dev.accumulator(sc.cam, SEED, sc.region)
    fresh.add(SPP, w.s2.cuda_stream)
    out2 = enqueue_resolve(w, fresh, sc, w.s2)
    w.s1.synchronize()
    w.s2.synchronize()
    assert image_bytes(sc, out) == want, "after reset"
    assert image_bytes(sc, out2) == want, "after create"
    # The null stream busy when the accumulator is made (a pipeline's own work on the default stream): a zeroing that
    # only queues behind that work would wipe the pass's sums later.  Resolved at once, and again after the device
    # has drained.
    default = w.torch.cuda.current_stream()
    busy = w.gate2.enqueue(default)
    late = sc.dev.accumulator(sc.cam, SEED, sc.region)
    late.add(SPP, w.s2.cuda_stream)
    out3 = enqueue_resolve(w, late, sc, w.s2)
    w.s2.synchronize()
    w.torch.cuda.synchronize()
    assert busy.query()
    out4 = enqueue_resolve(w, late, sc, w.s2)
    w.s2.synchronize()
    assert image_bytes(sc, out3) == want, "after create with the null stream busy"
    assert image_bytes(sc, out4) == want, "after create with the null stream busy, once the device has drained"
    for a in (acc, fresh, late):
        a.close()


def test_scratch_growth_across_streams(world, plan):
    """The scratch released, a 1-sample render on S1 behind a gate, then a 3-sample render on S2 that needs a larger
    scratch: the library waits on the host for the first before it reallocates (allowed to block: no check (b))."""
    w = world
    a, b = w.scene("cornell_box"), w.scene("random_spheres")
    want = serial_render(w, a, 1, SEED + 20), serial_render(w, b, SPP, SEED + 21)
    rtx.release_device_memory(0)
    assert rtx.device_scratch_bytes(0) == 0
    w.s1.wait_stream(w.torch.cuda.current_stream())
    w.gate1.enqueue(w.s1)
    o1 = enqueue_render(w, a, 1, SEED + 20, w.s1)
    small = rtx.device_scratch_bytes(0)
    o2 = enqueue_render(w, b, SPP, SEED + 21, w.s2)
    assert rtx.device_scratch_bytes(0) == SPP * small > 0
    w.s1.synchronize()
    w.s2.synchronize()
    assert image_bytes(a, o1) == want[0] and image_bytes(b, o2) == want[1]


def test_destroy_with_work_in_flight(world, plan):
    """rtx_accum_destroy and rtx_scene_destroy ("Blocking") called with a render and a pass still behind their gate:
    the clones taken on the stream hold the serial results, and the device reports no error."""
    w, torch = world, world.torch
    sc = w.scene("random_spheres")
    want = serial_render(w, sc, SPP, SEED + 30), serial_render(w, sc, SPP, SEED)
    dev = rtx.DeviceScene(sc.host.desc)
    acc = dev.accumulator(sc.cam, SEED, sc.region)
    warm = image_out(w, sc.pixels)
    dev.render_region(sc.cam, SEED + 30, sc.region, warm.data_ptr(), 0)  # the copy's layouts: blocking uploads
    torch.cuda.synchronize()
    assert image_bytes(sc, warm) == want[0]
    w.s1.wait_stream(torch.cuda.current_stream())
    ev = w.gate1.enqueue(w.s1)
    with torch.cuda.stream(w.s1):
        out, res = image_out(w, sc.pixels), image_out(w, sc.pixels)
    dev.render_region(sc.cam, SEED + 30, sc.region, out.data_ptr(), w.s1.cuda_stream)
    acc.add(SPP, w.s1.cuda_stream)
    acc.resolve_device(res.data_ptr(), 0, 0.0, w.s1.cuda_stream)
    with torch.cuda.stream(w.s1):
        clones = out.clone(), res.clone()
    assert not ev.query(), "vacuous: the gate had finished before the destroys"
    acc.close()
    dev.close()
    assert ev.query(), "the destroys are blocking"
    w.s1.synchronize()
    assert image_bytes(sc, clones[0]) == want[0] and image_bytes(sc, clones[1]) == want[1]
    assert rtx.load().rtx_device_check(0) == rtx.RTX_OK


def test_the_device_reports_no_error_at_the_end(world):
    assert rtx.load().rtx_device_check(0) == rtx.RTX_OK
