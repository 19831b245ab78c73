"""Direct light sampling on the GPU (rtx_direct*, wavefront.render(direct=True)).

The block is held to tests/direct_ref.py bit for bit, field by field, on real hits of three scenes (camera rays ->
trace(UV), events 1 and 2) and on hand-made edge records; its VISIBLE flag also to rtx_trace_device(RTX_TRACE_ANY) on
the record's own shadow ray.  The estimator built on it (wavefront.render(direct=True)) is held to closed forms with
tolerances derived from the geometry, and to the plain render where a scene has no emitter."""
import math
import os

import numpy as np
import pytest

import direct_ref
import direct_scenes as ds
import rtx
import wavefront

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 5  # records after the n the call may write: they must keep their poison
SEED = 0x5EED00D1CE
COUNTS = (0, 1, 63, 64, 65)


@pytest.fixture(scope="module")
def torch(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def trace_dev(torch, dev, rays, flags=rtx.RTX_TRACE_UV):
    n = len(rays)
    d_rays = to_device(torch, rays)
    d_hits = torch.zeros((max(n, 1) * 48,), dtype=torch.uint8, device="cuda")
    dev.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags, stream_of(torch))
    torch.cuda.synchronize()
    return d_hits.cpu().numpy()[: n * 48].view(rtx.HIT_DTYPE)


def direct_dev(torch, dev, hits, keys, seed, flags=0, stats=False):
    """rtx_direct_device on torch tensors: the output poisoned with 0xFF, PAD records longer than n."""
    n = len(hits)
    d = [to_device(torch, a) for a in (hits, keys)]
    out = torch.full(((n + PAD) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    st = dev.direct_device(seed, *[t.data_ptr() if n else 0 for t in d], n, out.data_ptr(), flags, stream_of(torch), stats)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * 64:] == 0xFF).all(), "records past n were written"
    return got[: n * 64].view(rtx.DIRECT_DTYPE), st


def window_camera(host_name, width, window):
    host = rtx.HostScene(host_name, 1)
    cam = host.camera(width=width, spp=1, depth=8)
    return host, host.desc, cam, rtx.Region(*window, 0, 1)


def material_where(desc, want):
    """The first material for which want(material, its texture's type) holds."""
    d = desc.contents
    for i in range(d.n_materials):
        m = d.materials[i]
        tex = d.textures[m.texture].type if m.type in (rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT) else None
        if want(m.type, tex):
            return i
    raise AssertionError("no such material")


def edge_records(desc, floor_point, plane_point):
    """Hand-made hits on a SolidColor Lambertian: a miss, a hit on a material that is not Lambertian (a Metal where the
    scene has one, else the DiffuseLight), a hit in the quad light's own plane (cl = 0 when that light is drawn), a hit
    facing away from every light (cs <= 0), a NaN point, a material index outside the table; each repeated with 24
    keys so that every light of the table is drawn."""
    lam = material_where(desc, lambda t, tex: t == rtx.RTX_MAT_LAMBERTIAN and tex == rtx.RTX_TEX_SOLID)
    try:
        metal_material = material_where(desc, lambda t, tex: t == rtx.RTX_MAT_METAL)
    except AssertionError:
        metal_material = material_where(desc, lambda t, tex: t == rtx.RTX_MAT_DIFFUSE_LIGHT)
    kinds = []
    h = np.zeros(6, rtx.HIT_DTYPE)
    h["prim"] = (rtx.RTX_PRIM_QUAD << 28)
    h["t"], h["front_face"], h["normal"], h["material"] = 1.0, 1, (0, 1, 0), lam
    h["point"] = floor_point
    h["prim"][0], h["t"][0] = rtx.RTX_HIT_NONE, np.inf
    kinds.append("miss")
    h["material"][1] = metal_material
    kinds.append("metal")
    h["point"][2], h["normal"][2] = plane_point, (-1, 0, 0)
    kinds.append("plane")
    h["normal"][3] = (0, -1, 0)
    kinds.append("away")
    h["point"][4] = (np.nan, 0, 0)
    kinds.append("nan")
    h["material"][5] = desc.contents.n_materials
    kinds.append("nomat")
    reps = 24
    hits = np.repeat(h, reps)
    keys = np.zeros(len(hits), rtx.KEY_DTYPE)
    keys["pixel"], keys["sample"], keys["event"] = np.arange(len(hits)) * 7 + 3, np.arange(len(hits)) % 5, 1
    return hits, keys, [k for k in kinds for _ in range(reps)]


_records = {}


def records(torch, name):
    """(description, device scene, hits, keys, albedo, reference records, edge kinds) of one scene: the real hits of
    a window's camera rays (event 1) and of their bounces (event 2), then the edge records.  Computed once, shared,
    never modified."""
    if name in _records:
        return _records[name]
    if name == "cornell_box":
        host, desc, cam, region = window_camera("cornell_box", 64, (12, 20, 37, 25))
        edges = ((278.0, 0.0, 278.0), (50.0, 554.0, 279.0))
    elif name == "simple_light_demo":
        host, desc, cam, region = window_camera("simple_light_demo", 64, (10, 6, 41, 23))
        edges = ((3.0, 0.0, 1.0), (9.0, 7.0, 0.0))
    else:
        host = None
        desc, cam = ds.five()
        region = rtx.Region(8, 6, 37, 25, 0, 1)
        edges = ((0.3, 0.0, 2.0), (3.0, 3.0, 0.25))
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    P = rtx.region_rows(region) * region.width
    d_rays = torch.empty((P, 8), dtype=torch.float32, device="cuda")
    d_keys = torch.empty((P, 4), dtype=torch.int32, device="cuda")
    rtx.camera_rays_device(cam, SEED, region, 0, 1, d_rays.data_ptr(), d_keys.data_ptr(), stream_of(torch))
    torch.cuda.synchronize()
    rays1 = d_rays.cpu().numpy().reshape(-1).view(rtx.RAY_DTYPE).copy()
    keys1 = d_keys.cpu().numpy().reshape(-1).view(rtx.KEY_DTYPE).copy()
    hits1 = trace_dev(torch, dev, rays1)
    b1 = dev.shade(rays1, hits1, keys1, SEED)
    rays2 = b1["ray"].copy()
    keys2 = keys1.copy()
    keys2["event"] = 2
    hits2 = trace_dev(torch, dev, rays2)
    b2 = dev.shade(rays2, hits2, keys2, SEED)
    eh, ek, kinds = edge_records(desc, *edges)
    hits = np.concatenate([hits1, hits2, eh])
    keys = np.concatenate([keys1, keys2, ek])
    albedo = np.concatenate([b1["attenuation"], b2["attenuation"], np.zeros((len(eh), 3), F32)])
    want = direct_ref.sample(desc, dev.export(), hits, keys, SEED, albedo=albedo)
    _records[name] = (desc, dev, hits, keys, want, [None] * (2 * P) + kinds, host)
    return _records[name]


def same_records(got, want):
    assert got.dtype == want.dtype == rtx.DIRECT_DTYPE and got.shape == want.shape
    if got.tobytes() == want.tobytes():
        return
    g, w = got.view(np.uint32).reshape(-1, 16), want.view(np.uint32).reshape(-1, 16)
    bad = np.argwhere(g != w)
    raise AssertionError(f"{len(np.unique(bad[:, 0]))} of {len(got)} records differ; first (record, word): {bad[:6].tolist()}; "
                         f"got {got[bad[0, 0]]} want {want[bad[0, 0]]}")


SCENES = ("cornell_box", "simple_light_demo", "five")


@pytest.mark.parametrize("name", SCENES)
def test_block_equals_reference(torch, name):
    """Every bit of every field, about 2000 records; the counters are the sums over the records."""
    desc, dev, hits, keys, want, kinds, _ = records(torch, name)
    got, st = direct_dev(torch, dev, hits, keys, SEED, rtx.RTX_DIRECT_COUNTERS, stats=True)
    sampled = (want["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
    visible = (want["flags"] & rtx.RTX_DIRECT_VISIBLE) != 0
    print(f"{name}: {len(want)} records, {int((want['rng_draws'] != 0).sum())} Lambertian, {int(sampled.sum())} sampled, "
          f"{int(visible.sum())} visible, most draws {int(want['rng_draws'].max())}, lights {np.bincount(want['light'][sampled])}")
    same_records(got, want)
    assert (st.n, st.sampled, st.visible, st.rng_draws) == (len(want), int(sampled.sum()), int(visible.sum()),
                                                            int(want["rng_draws"].sum()))
    assert st.kernel_ms > 0
    timed, none = direct_dev(torch, dev, hits, keys, SEED)
    assert none is None
    same_records(timed, want)
    # the cases the scenes are there for
    assert sampled.sum() > 100 and visible.sum() > 50 and (sampled & ~visible).sum() >= 5
    if name != "cornell_box":
        assert want["rng_draws"].max() > 4, "no record took a second rejection attempt"


@pytest.mark.parametrize("name", SCENES)
def test_edge_records(torch, name):
    desc, dev, hits, keys, want, kinds, _ = records(torch, name)
    kinds = np.array([k or "" for k in kinds])
    tab = rtx.lights(desc)
    for k in ("miss", "metal", "nomat"):
        assert not want[kinds == k].view(np.uint32).any(), k  # all zero
    for k in ("away", "nan"):
        w = want[kinds == k]
        assert (w["flags"] == 0).all() and (w["rng_draws"] >= 3).all(), k
        assert not w["radiance"].any() and not np.ascontiguousarray(w["ray"]).view(np.uint32).any() and not w["geom"].view(np.uint32).any(), k
    w = want[kinds == "plane"]
    on_quad = (tab["prim"][w["light"]] >> 28) == rtx.RTX_PRIM_QUAD
    if name != "simple_light_demo":
        assert on_quad.any() and (w["flags"][on_quad] == 0).all()  # cl = 0 exactly
    if len(tab) > 1:
        assert len(np.unique(want[kinds == "away"]["light"])) == len(tab)


@pytest.mark.parametrize("name", SCENES)
def test_visible_is_the_any_hit_trace(torch, name):
    """VISIBLE <=> rtx_trace_device(the record's ray, RTX_TRACE_ANY) finds nothing, on the GPU's own records."""
    desc, dev, hits, keys, want, _, _ = records(torch, name)
    got, _ = direct_dev(torch, dev, hits, keys, SEED)
    s = np.nonzero(got["flags"] & rtx.RTX_DIRECT_SAMPLED)[0]
    rays = got["ray"][s].copy()
    assert (rays["tmin"] == F32(0.001)).all() and (rays["tmax"] == F32(0.999)).all()
    assert np.array_equal(np.ascontiguousarray(rays["origin"]).view(np.uint32), np.ascontiguousarray(hits["point"][s]).view(np.uint32))
    any_hit = trace_dev(torch, dev, rays, rtx.RTX_TRACE_ANY)
    assert np.array_equal((got["flags"][s] & rtx.RTX_DIRECT_VISIBLE) != 0, any_hit["prim"] == rtx.RTX_HIT_NONE)
    unsampled = got[(got["flags"] & rtx.RTX_DIRECT_SAMPLED) == 0]
    assert (unsampled["flags"] == 0).all() and not np.ascontiguousarray(unsampled["ray"]).view(np.uint32).any()


@pytest.mark.parametrize("n", COUNTS)
def test_counts_and_partial_waves(torch, n):
    """n = 0, 1, 63, 64, 65: a prefix of the records gives the prefix of the reference, through both entries."""
    desc, dev, hits, keys, want, _, _ = records(torch, "five")
    lo = 40
    got, st = direct_dev(torch, dev, hits[lo: lo + n], keys[lo: lo + n], SEED, rtx.RTX_DIRECT_COUNTERS, stats=True)
    same_records(got, want[lo: lo + n])
    assert st.n == n and st.rng_draws == int(want["rng_draws"][lo: lo + n].sum())
    host_got, host_st = dev.direct(hits[lo: lo + n], keys[lo: lo + n], SEED, stats=True, flags=rtx.RTX_DIRECT_COUNTERS)
    same_records(host_got, want[lo: lo + n])
    assert (host_st.n, host_st.sampled, host_st.visible) == (st.n, st.sampled, st.visible)


@pytest.mark.parametrize("knob,value", [("RTX_DIRECT_LAUNCH_RECORDS", "64"), ("RTX_DIRECT_RANGE", "64"),
                                        ("RTX_DIRECT_RANGE", "1024"), ("RTX_DIRECT_PRIM_BATCH", "1")])
def test_launch_cut_and_knobs_change_nothing(torch, knob, value):
    desc, dev, hits, keys, want, _, _ = records(torch, "five")
    os.environ[knob] = value
    try:
        got, st = direct_dev(torch, dev, hits[:333], keys[:333], SEED, rtx.RTX_DIRECT_COUNTERS, stats=True)
    finally:
        os.environ.pop(knob, None)
    same_records(got, want[:333])
    assert st.rng_draws == int(want["rng_draws"][:333].sum())


def test_scene_table_and_renders_left_alone(torch):
    """rtx_scene_lights equals rtx_lights; a render before and after a counting direct call gives the same image and
    stats, and the block uses none of the sample scratch."""
    desc, dev, hits, keys, want, _, _ = records(torch, "five")
    assert dev.lights().tobytes() == rtx.lights(desc).tobytes()
    _, cam = ds.five()
    cam.samples_per_pixel = 2
    before, st0 = dev.render_host(cam, 5, stats=True, counters=True)
    scratch = rtx.device_scratch_bytes(0)
    direct_dev(torch, dev, hits, keys, SEED, rtx.RTX_DIRECT_COUNTERS, stats=True)
    assert rtx.device_scratch_bytes(0) == scratch
    after, st1 = dev.render_host(cam, 5, stats=True, counters=True)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert (st0.segments, st0.hits, st0.rng_draws, st0.node_visits) == (st1.segments, st1.hits, st1.rng_draws, st1.node_visits)


def test_noise_textured_emitter_and_albedo(torch):
    """Le and a from Perlin noise, against the oracle's NoiseTexture value (no colour handed in): a quad light and a
    floor that both carry simple_light_demo's noise texture, hand-made hits on a grid of floor points."""
    host = rtx.HostScene("simple_light_demo", 1)
    hd = host.desc.contents
    noise = next(hd.textures[i] for i in range(hd.n_textures) if hd.textures[i].type == rtx.RTX_TEX_NOISE)
    tex = rtx.Texture()
    tex.type, tex.scale, tex.texel_offset = noise.type, noise.scale, noise.texel_offset
    desc = ds.world([], [ds.quad((-3, 0, -3), (0, 0, 6), (6, 0, 0), 0), ds.quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), 1)],
                    [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 0)], [tex])
    desc.contents.texels, desc.contents.n_texels = hd.texels, hd.n_texels
    n = 300
    hits = np.zeros(n, rtx.HIT_DTYPE)
    hits["prim"], hits["t"], hits["front_face"], hits["normal"] = rtx.RTX_PRIM_QUAD << 28, 1.0, 1, (0, 1, 0)
    g = np.arange(n)
    hits["point"] = np.stack([-2.5 + 0.37 * (g % 14), np.zeros(n), -2.4 + 0.23 * (g // 14)], axis=1).astype(F32)
    keys = np.zeros(n, rtx.KEY_DTYPE)
    keys["pixel"], keys["sample"], keys["event"] = g * 13 + 1, g % 7, 1 + g % 3
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        want = direct_ref.sample(desc, dev.export(), hits, keys, SEED)
        got, _ = direct_dev(torch, dev, hits, keys, SEED)
        sampled = (want["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
        assert sampled.sum() > 200 and len(np.unique(want["radiance"][sampled][:, 0])) > 100  # the texture varies
        same_records(got, want)
    finally:
        dev.close()


def memory_scene():
    """One emitting quad, one emitting sphere, a Lambertian floor and a 32 x 32 grid of small Lambertian spheres under
    a binary tree of its own: 3 + 1023 nodes + 1024 spheres = 2050 entries, the fewest of a square grid with
    (entries + 1) * 16 B past the 32 KB of 'a' halves the LDS copy holds (2048 entries).  The grid floats between the
    floor and the lights, so a good part of the floor's shadow rays is blocked."""
    texs = [ds.solid(0.8, 0.7, 0.6), ds.solid(6, 5, 4), ds.solid(3, 4, 5), ds.solid(0.2, 0.5, 0.3)]
    mats = [ds.material(ds.LAMB, 0), ds.material(ds.LIGHT, 1), ds.material(ds.LIGHT, 2), ds.material(ds.LAMB, 3)]
    quads = [ds.quad((-4, 0, -4), (0, 0, 8), (8, 0, 0), 0),   # floor, normal +y
             ds.quad((-1, 3, -1), (2, 0, 0), (0, 0, 2), 1)]   # light, normal -y
    g, radius = 32, F32(0.05)
    xz = (np.arange(g, dtype=F32) - F32((g - 1) / 2)) * F32(0.2)
    centres = np.stack([np.repeat(xz, g), np.full(g * g, 0.9, F32), np.tile(xz, g)], axis=1).astype(F32)
    spheres = [ds.sphere((2, 1.6, 0), 0.5, 2)] + [ds.sphere([float(v) for v in c], float(radius), 3) for c in centres]
    nodes = []

    def build(idx, axis):  # a median split, x and z in turn; the grid's sphere k is sphere 1 + k of the table
        if len(idx) == 1:
            return rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 1 + int(idx[0]))
        me = len(nodes)
        nodes.append(rtx.BvhNode())
        idx = idx[np.argsort(centres[idx, axis], kind="stable")]
        left, right = build(idx[: len(idx) // 2], 2 - axis), build(idx[len(idx) // 2:], 2 - axis)
        n = nodes[me]
        n.bmin[:] = [float(v) for v in centres[idx].min(axis=0) - radius]
        n.bmax[:] = [float(v) for v in centres[idx].max(axis=0) + radius]
        n.left, n.right = left, right
        return me

    root = build(np.arange(g * g), 0)
    roots = [rtx.ref_prim(rtx.RTX_PRIM_QUAD, 0), rtx.ref_prim(rtx.RTX_PRIM_QUAD, 1), rtx.ref_prim(rtx.RTX_PRIM_SPHERE, 0), root]
    desc = ds.world(spheres, quads, mats, texs, roots=roots)
    desc._keep["nodes"] = (rtx.BvhNode * len(nodes))(*nodes)
    desc.contents.n_nodes, desc.contents.nodes = len(nodes), desc._keep["nodes"]
    return desc, ds.five()[1]


def test_a_scene_read_from_memory(torch):
    """direct_lights and direct_paths on a layout read from HBM (the FIXED = false instantiations), a 24 x 13 window:
    312 records, a partial last wave.  The block equals direct_ref bit for bit, VISIBLE equals the any-hit trace, and
    add_direct of 3 samples resolves bit-equal to the composed blocks."""
    desc, cam = memory_scene()
    region = rtx.Region(20, 12, 24, 13, 0, 1)
    dev = rtx.DeviceScene(desc, reference_bvh=True, every_box=True)
    try:
        P = rtx.region_rows(region) * region.width
        assert P == 312
        d_rays = torch.empty((P, 8), dtype=torch.float32, device="cuda")
        d_keys = torch.empty((P, 4), dtype=torch.int32, device="cuda")
        rtx.camera_rays_device(cam, SEED, region, 0, 1, d_rays.data_ptr(), d_keys.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        rays = d_rays.cpu().numpy().reshape(-1).view(rtx.RAY_DTYPE).copy()
        keys = d_keys.cpu().numpy().reshape(-1).view(rtx.KEY_DTYPE).copy()
        hits, st = dev.trace(rays, rtx.RTX_TRACE_UV, stats=True)
        assert st.scene_placement == rtx.RTX_SCENE_IN_HBM
        # the block
        want = direct_ref.sample(desc, dev.export(), hits, keys, SEED)
        got, dst = direct_dev(torch, dev, hits, keys, SEED, rtx.RTX_DIRECT_COUNTERS, stats=True)
        sampled = (want["flags"] & rtx.RTX_DIRECT_SAMPLED) != 0
        visible = (want["flags"] & rtx.RTX_DIRECT_VISIBLE) != 0
        print(f"memory scene: {len(want)} records, {int(sampled.sum())} sampled, {int(visible.sum())} visible, "
              f"{int((sampled & ~visible).sum())} occluded")
        same_records(got, want)
        assert (dst.n, dst.sampled, dst.visible, dst.rng_draws) == (P, int(sampled.sum()), int(visible.sum()),
                                                                    int(want["rng_draws"].sum()))
        assert visible.sum() > 0 and (sampled & ~visible).sum() > 0  # both outcomes of a shadow walk
        s = np.nonzero(got["flags"] & rtx.RTX_DIRECT_SAMPLED)[0]
        any_hit = trace_dev(torch, dev, got["ray"][s].copy(), rtx.RTX_TRACE_ANY)
        assert np.array_equal((got["flags"][s] & rtx.RTX_DIRECT_VISIBLE) != 0, any_hit["prim"] == rtx.RTX_HIT_NONE)
        # the fused pass
        cam.max_depth, cam.samples_per_pixel = 8, 3
        composed = wavefront.render(dev, cam, 29, region, direct=True).cpu().numpy()
        acc = dev.accumulator(cam, 29, region)
        try:
            acc.add_direct(3)
            rgb = acc.resolve()[0]
        finally:
            acc.close()
        bad = np.argwhere((rgb.view(np.uint32) != composed.view(np.uint32)).any(axis=2))
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(rgb[y, x], composed[y, x]) for y, x in bad[:3]])
    finally:
        dev.close()


# ---- the estimator ----------------------------------------------------------------------------------------------
def test_no_emitters_is_the_plain_render(torch):
    """random_spheres 24 x 13, the caller's tree, depth 8: with no emitter nothing is added and nothing suppressed."""
    host = rtx.HostScene("random_spheres", 1)
    cam = host.camera(width=24, spp=8, depth=8)
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True)
    try:
        assert len(dev.lights()) == 0
        plain = wavefront.render(dev, cam, 11, region).cpu().numpy()
        for compact in (False, True):
            lit = wavefront.render(dev, cam, 11, region, compact=compact, direct=True).cpu().numpy()
            assert np.array_equal(plain.view(np.uint32), lit.view(np.uint32))
        out = np.zeros((cam.image_height, cam.image_width, 3), F32)
        reg = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
        d_out = torch.zeros(out.shape, dtype=torch.float32, device="cuda")
        dev.render_region(cam, 11, reg, d_out.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), plain.view(np.uint32))
    finally:
        dev.close()


def test_depth_one_takes_no_light_sample(torch):
    """max_depth 1: s + 1 < max_depth never holds, so the estimator is the plain render; compact = carried."""
    desc, cam = ds.five()
    region = rtx.Region(3, 2, 37, 21, 0, 1)
    dev = records(torch, "five")[1]
    for depth in (1, 2, 8):
        cam.max_depth, cam.samples_per_pixel = depth, 3
        lit = [wavefront.render(dev, cam, 17, region, compact=c, direct=True).cpu().numpy() for c in (False, True)]
        assert np.array_equal(lit[0].view(np.uint32), lit[1].view(np.uint32)), depth
        plain = wavefront.render(dev, cam, 17, region).cpu().numpy()
        assert np.array_equal(plain.view(np.uint32), lit[0].view(np.uint32)) == (depth == 1), depth


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_unbiased_against_closed_forms(torch, kind):
    """The estimator on the analytic scenes, 16 x 16, depth 2: a sample is T * radiance of one light sample, so it
    lies in [0, a Le g_max] with g_max from the geometry (direct_scenes.g_max) and sigma_p <= a Le g_max / 2 per pixel.
      every pixel:  |mean of N samples - a Le F| <= 6 sigma_p / sqrt(N)
      image mean:   within 6 sqrt(mean of sigma_p^2) / sqrt(P N)
    N is the least power of two >= 256 for which the image bound is at most 3 % of the expected mean.  The float32
    rounding of a sample (2^-24 relative) is far below both.  A missing factor L (case b) would halve the image."""
    desc, cam, lights = ds.floor_scene(kind)
    want, f = ds.expected_image(cam, lights)
    scale = np.array(ds.ALBEDO) * np.array(ds.EMIT)
    sigma = ds.g_max(cam, lights) / 2  # in units of a Le
    P = f.size
    N = 256
    while 6 * math.sqrt(float((sigma ** 2).mean()) / (P * N)) > 0.03 * float(f.mean()):
        N *= 2
    assert N <= 4096, N
    cam.samples_per_pixel = N
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(desc)
    try:
        assert len(dev.lights()) == len(lights)
        img = wavefront.render(dev, cam, 424242, region, direct=True).cpu().numpy().astype(np.float64)
    finally:
        dev.close()
    tol_img = 6 * math.sqrt(float((sigma ** 2).mean()) / (P * N))
    ratio = img.mean(axis=(0, 1)) / want.mean(axis=(0, 1))
    worst = np.abs(img - want).max(axis=2) / scale.max() / (6 * sigma / math.sqrt(N))
    print(f"{kind}: N {N}, image mean / closed form {ratio}, bound {tol_img / f.mean():.4f}; worst pixel at "
          f"{worst.max():.3f} of its bound")
    assert np.all(np.abs(img.mean(axis=(0, 1)) - want.mean(axis=(0, 1))) <= tol_img * scale), (ratio, tol_img / f.mean())
    assert np.all(np.abs(img - want) <= (6 * sigma / math.sqrt(N))[..., None] * scale[None, None, :])

# ---- the fused pass (rtx_accum_add_direct) ----------------------------------------------------------------------
def test_fused_no_emitters_is_the_plain_pass(torch):
    """random_spheres 24 x 13, the caller's tree, depth 8: add_direct(3) + add_direct(5) resolves, rgb and var,
    bit-equal to add(8)."""
    host = rtx.HostScene("random_spheres", 1)
    cam = host.camera(width=24, spp=8, depth=8)
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(host.desc, reference_bvh=True)
    try:
        a, b = dev.accumulator(cam, 11, region), dev.accumulator(cam, 11, region)
        a.add_direct(3)
        st = a.add_direct(5, stats=True)
        b.add(8)
        assert a.samples == b.samples == 8
        assert st.samples == 5 * 24 * 13 and st.kernel_ms > 0 and st.walk_layout == rtx.RTX_LAYOUT_REFERENCE
        (rgb_a, var_a, _), (rgb_b, var_b, _) = a.resolve(), b.resolve()
        assert np.array_equal(rgb_a.view(np.uint32), rgb_b.view(np.uint32))
        assert np.array_equal(var_a.view(np.uint32), var_b.view(np.uint32))
        a.close()
        b.close()
    finally:
        dev.close()


FUSED_CASES = {  # region (x0, y0, width, height, rank, world), max_depth, passes
    "ragged_37x21_3+5": ((3, 2, 37, 21, 0, 1), 8, (3, 5)),
    "rank_1_of_3_depth_2": ((0, 0, 64, 30, 1, 3), 2, (8,)),
    "depth_1": ((3, 2, 37, 21, 0, 1), 1, (8,)),
    "depth_2": ((3, 2, 37, 21, 0, 1), 2, (8,)),
    "rank_1_of_3_depth_8": ((0, 0, 64, 30, 1, 3), 8, (8,)),
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
@pytest.mark.parametrize("name", SCENES)
def test_fused_equals_composed(torch, name, case):
    """add_direct resolves bit-equal to wavefront.render(direct=True): ragged tiles, a rank of three, passes 3 + 5
    against 8 samples at once, max_depth 1 (no light sample: also the plain pass), 2 and 8."""
    window, depth, passes = FUSED_CASES[case]
    desc, dev = records(torch, name)[:2]
    if name == "five":
        cam = ds.five()[1]
    else:
        cam = rtx.HostScene(name, 1).camera(width=64, spp=8, depth=depth)
    cam.max_depth, cam.samples_per_pixel = depth, sum(passes)
    region = rtx.Region(*window)
    want = wavefront.render(dev, cam, 29, region, direct=True).cpu().numpy()
    acc = dev.accumulator(cam, 29, region)
    try:
        for n in passes:
            acc.add_direct(n)
        rgb, _, _ = acc.resolve()
        bad = np.argwhere((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=2))
        print(f"{name} {case}: {len(bad)} of {rgb.shape[0] * rgb.shape[1]} pixels differ; means {rgb.mean():.6g} "
              f"{want.mean():.6g}; zero pixels {int((rgb == 0).all(axis=2).sum())} {int((want == 0).all(axis=2).sum())}")
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(rgb[y, x], want[y, x]) for y, x in bad[:3]])
        if depth == 1:
            acc.reset()
            acc.add(sum(passes))
            assert np.array_equal(acc.resolve()[0].view(np.uint32), rgb.view(np.uint32))
    finally:
        acc.close()


def test_fused_unbiased_against_closed_forms(torch):
    """The fused pass itself on analytic scene b (two quad lights), with test_unbiased_against_closed_forms' bounds."""
    desc, cam, lights = ds.floor_scene("b")
    want, f = ds.expected_image(cam, lights)
    scale = np.array(ds.ALBEDO) * np.array(ds.EMIT)
    sigma = ds.g_max(cam, lights) / 2
    P, N = f.size, 256
    tol_img = 6 * math.sqrt(float((sigma ** 2).mean()) / (P * N))
    assert tol_img <= 0.03 * float(f.mean())
    region = rtx.Region(0, 0, cam.image_width, cam.image_height, 0, 1)
    dev = rtx.DeviceScene(desc)
    try:
        acc = dev.accumulator(cam, 424242, region)
        acc.add_direct(N)
        img = acc.resolve()[0].astype(np.float64)
        acc.close()
    finally:
        dev.close()
    print(f"fused b: image mean / closed form {img.mean(axis=(0, 1)) / want.mean(axis=(0, 1))}")
    assert np.all(np.abs(img.mean(axis=(0, 1)) - want.mean(axis=(0, 1))) <= tol_img * scale)
    assert np.all(np.abs(img - want) <= (6 * sigma / math.sqrt(N))[..., None] * scale[None, None, :])


def test_accumulator_modes(torch):
    """Plain after direct, direct after plain, direct after adaptive and adaptive after direct fail until reset;
    flags must be 0; preview, ppm and sample_counts of a direct accumulator run."""
    desc, dev = records(torch, "five")[:2]
    cam = ds.five()[1]
    cam.max_depth = 4
    region = rtx.Region(0, 0, 40, 20, 0, 1)
    acc = dev.accumulator(cam, 3, region)

    def refused(call):
        with pytest.raises(rtx.RtxError) as e:
            call()
        assert e.value.code == rtx.RTX_ERR_INVALID_ARG

    try:
        refused(lambda: acc.add_direct(0))
        refused(lambda: acc.add_direct(1, flags=1))
        acc.add_direct(2)
        refused(lambda: acc.add(1))
        refused(lambda: acc.add_adaptive(1, 0.1))
        assert acc.samples == 2
        rgb = acc.resolve()[0]
        assert np.isfinite(rgb).all() and rgb.max() > 0
        assert acc.ppm().startswith(b"P3\n40 20\n255\n") and acc.preview(2).shape == (20, 40, 3)
        assert (acc.sample_counts() == 2).all()
        acc.reset()
        acc.add(2)
        refused(lambda: acc.add_direct(1))
        acc.reset()
        acc.add_adaptive(2, 0.1)
        refused(lambda: acc.add_direct(1))
        acc.reset()
        acc.add_direct(1)
        acc.add_direct(1)
        assert acc.samples == 2 and np.array_equal(acc.resolve()[0].view(np.uint32), rgb.view(np.uint32))
    finally:
        acc.close()


def test_device_check_is_clean(torch):
    for rec in _records.values():
        rec[1].close()
    _records.clear()
    rtx.device_check(0)
