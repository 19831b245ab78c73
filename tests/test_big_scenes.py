"""The preconditions of tests/test_big_scenes_gpu.py, on the CPU: what makes its GPU cases mean something.

  - Layout is big.  Every scene of tests/big_scenes.py exports more than LIMIT entries, and so does the walk the
    library plans for it (the collapsed walk leaves node entries out: rtx_collapse.h), so pack_layout takes the big,
    hot-first layout; split_tier's near tree stays under the limit while its guarded tree passes it.
  - Trees are sound.  The walk of each hand-made tree (trace_ref.walk) returns what a scan of every primitive returns
    (trace_ref.scan) for the window's camera rays: a GPU mismatch cannot be blamed on a broken tree.
  - Windows are sensitive.  On the window each GPU test renders, every kind of primitive is the first hit of at least
    2 % of the pixels, the oracle fetches texels, and on big_ties the oracle without the rank rule differs from the
    oracle with it on more than 50 pixels.
  - The adaptive case closes some tiles of mixed's window after 4 samples and leaves some open.
  - ref64 keeps enough on the two cases ref64_cases.CASES holds of these scenes.
"""
import numpy as np
import pytest

import accum_ref
import adaptive_ref
import big_scenes as bs
import oracle_binding as ob
import ref64_cases as rc
import rtx
import trace_ref

F32 = np.float32
SEED = 5  # the render seed of the GPU tests
ADAPT_TOL = 0.4  # rel_tol of the GPU file's adaptive pass
MIXED = ("mixed", "mixed_noise", "mixed_world")
VIEWS = [(n, ax) for n in MIXED for ax in (False, True)] + [("big_ties", False), ("split_tier", False)]
KINDS = {"mixed": ("sphere", "quad", "emitter", "image", "nested"),
         "mixed_noise": ("sphere", "quad", "emitter", "image", "nested", "noise"),
         "mixed_world": ("sphere", "quad", "emitter", "image")}


def planned_entries(desc, cam):
    """Entries of the layout the library uploads for the walk of desc's (or its rebuilt) tree: the tree's entries less
    the node entries the collapsed walk leaves out."""
    return len(trace_ref.entries_of(rtx.walk_tree_desc(desc, cam))) - int(rtx.walk_skip(desc, cam).sum())


def least_kept(desc):
    """A lower bound of a collapsed walk's entries: the primitives, and the nodes with a primitive for a child, which
    keep their box test whatever the plan (rtx_collapse.h)."""
    d = desc.contents
    return d.n_spheres + d.n_quads + sum(1 for i in range(d.n_nodes) if d.nodes[i].left < 0 or d.nodes[i].right < 0)


@pytest.mark.parametrize("name,axis_aligned", VIEWS)
def test_layout_is_big(built, name, axis_aligned):
    b = bs.scene(name)
    cam = bs.camera(name, axis_aligned)
    n = len(trace_ref.entries_of(b.desc))
    planned = planned_entries(b.desc, cam)
    print(f"{name}: {n} entries, {planned} in the planned walk")
    assert n > bs.LIMIT and planned > bs.LIMIT
    if name in ("mixed", "mixed_noise"):  # more than the cache holds: a render reads from the cache and from HBM
        assert planned > bs.CACHE_MAX
    if name == "mixed_world":  # no nodes, as few primitives as pass the limit (in round numbers)
        assert b.desc.contents.n_nodes == 0 and n == bs.N_SPHERES + bs.N_QUADS < bs.LIMIT + 16
    if name in ("big_ties", "split_tier"):  # sphere scenes: the library walks its own trees, in two tiers for this camera
        box, active = rtx.walk_near_region(b.desc, cam)
        assert active and rtx.walk_tree_desc(b.desc, cam) is not b.desc
        near = rtx.walk_near_desc(b.desc, cam)
        n_near = len(trace_ref.entries_of(near))
        if name == "big_ties":  # both tiers past the limit whatever the near walk leaves out
            assert least_kept(near) > bs.LIMIT
        else:  # the near tree in the small layout, the guarded tree in the big one: placed unalike
            assert n_near <= bs.LIMIT < planned, (n_near, planned)


@pytest.mark.parametrize("name,axis_aligned", VIEWS)
def test_trees_are_sound(built, name, axis_aligned):
    b = bs.scene(name)
    cam = bs.camera(name, axis_aligned)
    rays = bs.window_rays(cam, bs.window(name))
    sc = trace_ref.Scene(trace_ref.entries_of(b.desc), b.desc)
    want = trace_ref.scan(sc, rays, F32)
    got = trace_ref.walk(sc, rays, F32)
    assert want.mask.sum() > len(rays) // 2
    assert np.array_equal(got.entry, want.entry) and np.array_equal(got.t, want.t)
    if name in ("big_ties", "split_tier"):  # the trees the library walks instead: the same hits where nothing ties
        for tree in (rtx.walk_tree_desc(b.desc, cam), rtx.walk_near_desc(b.desc, cam)):
            st = trace_ref.Scene(trace_ref.entries_of(tree), tree)
            h = trace_ref.walk(st, rays, F32)
            ok = ~want.tie
            assert np.array_equal(h.prim[ok], want.prim[ok]) and np.array_equal(h.t, want.t)
    assert want.tie.any() == (name == "big_ties")


@pytest.mark.parametrize("name,axis_aligned", [v for v in VIEWS if v[0] in MIXED])
def test_windows_show_every_kind(built, name, axis_aligned):
    b = bs.scene(name)
    cam = bs.camera(name, axis_aligned)
    x0, y0, w, h = win = bs.window(name)
    assert w <= 40 and h <= 24 and w % 8 and h % 8
    sc = trace_ref.Scene(trace_ref.entries_of(b.desc), b.desc)
    kinds = bs.first_hit_kinds(b, trace_ref.scan(sc, bs.window_rays(cam, win), F32))
    share = {k: float(kinds[k].mean()) for k in KINDS[name]}
    print(name, axis_aligned, {k: round(100 * v, 1) for k, v in share.items()})
    for k, v in share.items():
        assert v >= 0.02, (k, v)
    _, cnt = ob.render(b.desc, cam, SEED, rtx.Region(*win, 0, 1), ob.ORDER_ITERATIVE)
    assert cnt["texel_fetches"] > 0 and cnt["texel_border"] > 0  # the image and its border texel


def test_mixed_holds_what_it_says(built):
    d = bs.scene("mixed").desc.contents
    mats = [d.materials[i] for i in range(d.n_materials)]
    assert {m.type for m in mats} == {rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_METAL, rtx.RTX_MAT_DIELECTRIC,
                                      rtx.RTX_MAT_DIFFUSE_LIGHT}
    textured = [m for m in mats if m.type in (rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT)]
    assert {d.textures[m.texture].type for m in textured} == {rtx.RTX_TEX_SOLID, rtx.RTX_TEX_CHECKERED, rtx.RTX_TEX_IMAGE}
    assert d.n_lists == 3 and d.n_quads == bs.N_QUADS and sum(np.isnan(d.quads[i].normal[0]) for i in range(d.n_quads)) == 5
    radii = np.array([d.spheres[i].radius for i in range(d.n_spheres)])
    assert radii.min() < 2e-3 and radii.max() == 999.0
    n = bs.scene("mixed_noise").desc.contents
    noisy = [m for m in (n.materials[i] for i in range(n.n_materials)) if n.textures[m.texture].type == rtx.RTX_TEX_NOISE]
    assert sorted(m.type for m in noisy) == [rtx.RTX_MAT_LAMBERTIAN, rtx.RTX_MAT_DIFFUSE_LIGHT]
    for i in range(d.n_spheres):  # the same primitives
        assert list(d.spheres[i].center) == list(n.spheres[i].center) and d.spheres[i].radius == n.spheres[i].radius


def test_split_tier_paths_leave_the_near_region(built):
    """More than 5 % of the window's first hits lie outside the near region (the far ground): at 4 samples per pixel
    more paths are deferred to the far pass than the 64 records the starved queue of the GPU test holds."""
    b = bs.scene("split_tier")
    cam = bs.camera("split_tier")
    box, active = rtx.walk_near_region(b.desc, cam)
    assert active
    rays = bs.window_rays(cam, bs.window("split_tier"))
    h = trace_ref.scan(trace_ref.Scene(trace_ref.entries_of(b.desc), b.desc), rays, F32)
    outside = h.mask & ((h.point < np.array(box[:3], F32)) | (h.point > np.array(box[3:], F32))).any(axis=1)
    assert outside.sum() > 0.05 * len(rays) and 4 * outside.sum() > 2 * 64, outside.sum()
    assert (h.mask & (h.prim != 0)).sum() > 0.1 * len(rays)  # and the small spheres show


def test_big_ties_matter(built):
    """test_ties_matter_on_the_near_tree's check on big_ties' window: the tiered walk without the tie rule differs
    from the reference walk on more than 50 pixels; with it (oracle_sphere_rank) it is bit-identical."""
    b = bs.scene("big_ties")
    cam = bs.camera("big_ties")
    box, active = rtx.walk_near_region(b.desc, cam)
    assert active
    near, far = rtx.walk_near_desc(b.desc, cam), rtx.walk_tree_desc(b.desc, cam)
    reg = rtx.Region(*bs.window("big_ties"), 0, 1)
    want, _ = ob.render(b.desc, cam, SEED, reg, ob.ORDER_ITERATIVE)
    bare, _ = ob.render(near, cam, SEED, reg, ob.ORDER_ITERATIVE, tier=(box, far, None))
    ranked, _ = ob.render(near, cam, SEED, reg, ob.ORDER_ITERATIVE, tier=(box, far, None), rank=ob.sphere_ranks(b.desc))
    assert np.array_equal(ranked, want)
    assert (bare != want).any(axis=2).sum() > 50


@pytest.mark.parametrize("case", list(bs.REF64))
def test_ref64_keeps_enough(built, case):
    assert case in rc.NAMES
    r = rc.built(case)
    print(r.report())
    assert (r.cam.image_width, r.cam.image_height, r.spp) == (36, 20, 1) and r.cam.max_depth <= 6
    assert r.cap == rc.CAP_SCENE and r.ref.left_out <= rc.CAP_SCENE and r.ref.tol <= 1e-5


def test_adaptive_case_closes_some_tiles(built):
    """From the reference alone (adaptive_ref on the oracle's per-sample colours): at ADAPT_TOL the second pass of 4
    samples finds 7 of the window's 15 tiles open."""
    b = bs.scene("mixed")
    reg = rtx.Region(*bs.window("mixed"), 0, 1)
    col = accum_ref.sample_colours(("big_scenes.mixed", bs.SEED, bs.CAM_SEED), b.desc, bs.camera("mixed", spp=8), SEED,
                                   reg, 8)
    r = adaptive_ref.simulate(col, (8, 8), (4, 4), ADAPT_TOL, 4)
    assert [p[0] for p in r.passes] == [15, 7] and sorted(np.unique(r.counts)) == [4, 8]
