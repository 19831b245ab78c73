"""NewBVHFromWorld for a World of spheres and quads in plain Python / numpy — TEST INFRASTRUCTURE (the reference of
rtx_scene_create_world).

Written from the Go source of TwFlem/raytracer-go (bvh.go:28-50, 63-82, 138-218, hittables.go:85-100, 149-165, cited
line by line below) and from the contract in include/rtx.h.  It shares no code with csrc/, host/ or oracle/.  From
bvh_ref it takes what works on box arrays per list position and knows no primitive kind: go_min, go_max, axes, calls,
compare and sort_func, and sphere_boxes for the spheres among the items.  What is new here is the quad's box, and a
recursion over a list of items instead of a table of spheres.

  build(items, spheres, quads, seed, draw0, tables)  ->  a pointer to an rtx.SceneDesc with `nodes` and one root over
  the CALLER's sphere and quad tables, neither copied nor reordered: every leaf is the item's own ref, an index into
  the caller's table, whatever the item's place in the list.  The threaded entries rtx_scene_export must return for the
  same inputs are trace_ref.entries_of(desc).

items: the World's list in World.Add order, each rtx.ref_prim(RTX_PRIM_SPHERE or RTX_PRIM_QUAD, index).  The sort
is stable and the k-th NewBVH call, in pre-order, takes Intn(3) from word draw0 + k of host stream 1 of `seed`, as
bvh_ref states.  HittableCompare{X,Y,Z} (bvh.go:187-218) reads GetBounds(): for a quad that is the PADDED box
(hittables.go:161, 196-198), so the padded minimum is its sort key.  A NaN bound is refused (out of contract).
"""
from __future__ import annotations

import ctypes

import numpy as np

import bvh_ref
import rtx
from bvh_ref import go_max, go_min

F32 = np.float32
EPS = F32(0.0001)  # eps := float32(0.0001), bvh.go:64


def quad_boxes(q: np.ndarray, u: np.ndarray, v: np.ndarray):
    """NewQuad's boxes (hittables.go:161): NewAabb(Q, Add(Add(Q, u), v)).GetPaddedAabb().  q, u, v [n, 3] float32 ->
    (bmin, bmax) [n, 3] float32.  Add rounds each sum to float32 (vec3.go); NewAabb takes MinF32 / MaxF32 per axis
    (bvh.go:28-34); GetPaddedAabb (bvh.go:63-82) widens an axis by eps on both sides when max - min < eps, a
    comparison that is false for a NaN difference."""
    q, u, v = (np.asarray(x, F32).reshape(-1, 3) for x in (q, u, v))
    with np.errstate(all="ignore"):
        p2 = ((q + u).astype(F32) + v).astype(F32)
        a, b = q.tolist(), p2.tolist()
        lo = np.array([[go_min(x, y) for x, y in zip(r, s)] for r, s in zip(a, b)], F32).reshape(-1, 3)
        hi = np.array([[go_max(x, y) for x, y in zip(r, s)] for r, s in zip(a, b)], F32).reshape(-1, 3)
        thin = (hi - lo).astype(F32) < EPS  # float32 subtraction; NaN < eps is false
        lo = np.where(thin, (lo - EPS).astype(F32), lo).astype(F32)
        hi = np.where(thin, (hi + EPS).astype(F32), hi).astype(F32)
    return lo, hi


def split_ref(ref: int):
    """(type, index) of a primitive ref (rtx.h: p = ~ref, type = p >> 28, index = p & 0x0FFFFFFF)."""
    if ref >= 0:
        raise ValueError(f"item {ref}: a node ref is no item of a World")
    p = (~ref) & 0xFFFFFFFF
    return p >> 28, p & 0x0FFFFFFF


def item_boxes(items, spheres, quads):
    """The box of every list position: (bmin, bmax) [n, 3] float32."""
    n = len(items)
    kinds = [split_ref(int(r)) for r in items]
    bmin, bmax = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    s_pos = [i for i, (t, _) in enumerate(kinds) if t == rtx.RTX_PRIM_SPHERE]
    q_pos = [i for i, (t, _) in enumerate(kinds) if t == rtx.RTX_PRIM_QUAD]
    if len(s_pos) + len(q_pos) != n:
        raise ValueError("an item that is neither a sphere nor a quad")
    if s_pos:
        raw = np.ctypeslib.as_array(ctypes.cast(spheres, ctypes.POINTER(ctypes.c_float)), shape=(len(spheres), 8))
        idx = [kinds[i][1] for i in s_pos]
        if max(idx) >= len(spheres):
            raise ValueError("a sphere index outside the table")
        bmin[s_pos], bmax[s_pos] = bvh_ref.sphere_boxes(raw[idx, 0:3], raw[idx, 3])
    if q_pos:
        raw = np.ctypeslib.as_array(ctypes.cast(quads, ctypes.POINTER(ctypes.c_float)), shape=(len(quads), 20))
        idx = [kinds[i][1] for i in q_pos]
        if max(idx) >= len(quads):
            raise ValueError("a quad index outside the table")
        bmin[q_pos], bmax[q_pos] = quad_boxes(raw[idx, 0:3], raw[idx, 4:7], raw[idx, 8:11])  # q, u, v of rtx_quad
    return bmin, bmax


def build(items, spheres, quads, seed: int, draw0: int, tables=None):
    """NewBVHFromWorld (bvh.go:138-140) of the World whose list is `items` (Add order).  spheres, quads: ctypes arrays
    (rtx.Sphere, rtx.Quad) or None.  tables: a scene description whose material, texture and texel tables the result
    points to as well."""
    items = [int(r) for r in items]
    n = len(items)
    if n < 1:
        raise ValueError("an empty World: NewBVH indexes h[0] (bvh.go:163)")
    bmin, bmax = item_boxes(items, spheres, quads)
    if np.isnan(bmin).any() or np.isnan(bmax).any():
        raise ValueError("a NaN box: the comparator is no order (out of contract)")
    axis_of = bvh_ref.axes(seed, draw0, bvh_ref.calls(n))
    lo, hi = bmin.tolist(), bmax.tolist()
    nodes = []  # [bmin, left, bmax, right] in pre-order
    drawn = [0]

    def leaf(i):  # list position -> (the item's own ref, its box)
        return items[i], lo[i], hi[i]

    def new_bvh(h):  # bvh.go:142-185 -> (ref, box min, box max)
        axis = axis_of[drawn[0]]  # :147, before the size switch
        drawn[0] += 1
        me = len(nodes)
        nodes.append(None)
        if len(h) == 1:  # :162-165
            left = right = leaf(h[0])
        elif len(h) == 2:  # :166-174
            if bvh_ref.compare(bmin, axis, h[0], h[1]) > 0:
                left, right = leaf(h[1]), leaf(h[0])
            else:
                left, right = leaf(h[0]), leaf(h[1])
        else:  # :175-179
            h = bvh_ref.sort_func(bmin, axis, h)
            mid = len(h) // 2
            left = new_bvh(h[:mid])
            right = new_bvh(h[mid:])
        box = ([go_min(a, b) for a, b in zip(left[1], right[1])],  # :182, NewAabbFromBoxes :44-50
               [go_max(a, b) for a, b in zip(left[2], right[2])])
        nodes[me] = (box[0], left[0], box[1], right[0])
        return me, box[0], box[1]

    with np.errstate(all="ignore"):
        new_bvh(np.arange(n))  # :144-145: a copy of the World's list
    assert drawn[0] == len(axis_of) == len(nodes)
    arr = (rtx.BvhNode * len(nodes))()
    flat = np.ctypeslib.as_array(ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint32)), shape=(len(nodes), 8))
    flat[:, 0:3].view(F32)[...] = np.array([nd[0] for nd in nodes], F32)
    flat[:, 4:7].view(F32)[...] = np.array([nd[2] for nd in nodes], F32)
    flat[:, 3].view(np.int32)[...] = [nd[1] for nd in nodes]
    flat[:, 7].view(np.int32)[...] = [nd[3] for nd in nodes]
    d = rtx.SceneDesc()
    roots = (ctypes.c_int32 * 1)(0)
    d.nodes, d.n_nodes, d.roots, d.n_roots = arr, len(nodes), roots, 1
    if spheres is not None and len(spheres):
        d.spheres, d.n_spheres = ctypes.cast(spheres, ctypes.POINTER(rtx.Sphere)), len(spheres)
    if quads is not None and len(quads):
        d.quads, d.n_quads = ctypes.cast(quads, ctypes.POINTER(rtx.Quad)), len(quads)
    if tables is not None:
        t = tables.contents if hasattr(tables, "contents") else tables
        d.materials, d.n_materials, d.textures, d.n_textures = t.materials, t.n_materials, t.textures, t.n_textures
        d.texels, d.n_texels = t.texels, t.n_texels
    p = ctypes.pointer(d)
    p._keep = (arr, roots, spheres, quads, tables)
    return p
