"""NewBVHFromWorld for a list of spheres in plain Python / numpy — TEST INFRASTRUCTURE (the reference of
rtx_scene_create_spheres).

Written from the Go source of TwFlem/raytracer-go (bvh.go:28-50, 138-218, hittables.go:85-100, cited line by line
below) and from the contract in include/rtx.h and DESIGN.md §2, §3 and §11.  It shares no code with csrc/, host/ or
oracle/: the recursion is the Go recursion itself, one Python call per NewBVH call; the Philox blocks are
ref64.philox4x32_10's; math.Min / math.Max are written out here.

  build(spheres, n, seed, draw0)  ->  a pointer to an rtx.SceneDesc with `nodes` and one root over the CALLER's sphere
  table, which is neither copied nor reordered: every primitive ref is an index in World.Add order.  The threaded
  entries rtx_scene_export must return for the same inputs are trace_ref.entries_of(desc).

The contract's two stated choices: the sort is stable (x/exp/slices.SortFunc promises no order among
elements that compare equal, so the stable order is one of its allowed results), and the k-th NewBVH call, in pre-order,
takes its rand.Intn(3) from word draw0 + k of host stream 1 of `seed`: Philox4x32-10 with the counter
(n >> 2 low word, n >> 2 high word, 0, 0x80000000 | 1), the key (seed low word, seed high word), word n & 3 of the
block, reduced by multiply-shift: Intn(3) = (word * 3) >> 32.

The sort itself is numpy's stable argsort of the negated minima; its result is then checked against the comparator as
Go states it (diff = b.min - a.min in float32: > 0, < 0, else equal): no neighbour out of order, equal neighbours in
their earlier order.  For a comparator that is a strict weak order that is the one stable result.  A NaN minimum makes
the comparator no order at all (out of contract): build() refuses it.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

import ref64
import rtx

F32, U64 = np.float32, np.uint64
HOST_STREAM = 1


def go_min(x: float, y: float) -> float:
    """math.Min as MinF32 calls it (math.go:38-40): the operands are float32 values, so is the result."""
    if (math.isinf(x) and x < 0) or (math.isinf(y) and y < 0):
        return -math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and x == y:
        return x if math.copysign(1.0, x) < 0 else y  # Min(-0, +0) = Min(+0, -0) = -0
    return x if x < y else y


def go_max(x: float, y: float) -> float:
    """math.Max (math.go:42-44)."""
    if (math.isinf(x) and x > 0) or (math.isinf(y) and y > 0):
        return math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and x == y:
        return y if math.copysign(1.0, x) < 0 else x  # Max(-0, +0) = Max(+0, -0) = +0
    return x if x > y else y


def sphere_boxes(center: np.ndarray, radius: np.ndarray):
    """NewSphere's boxes (hittables.go:85-92): NewAabb(center + rvec * -1, center + rvec), NewAabb (bvh.go:28-34)
    taking MinF32 / MaxF32 per axis.  center [n, 3], radius [n] float32 -> (bmin, bmax) [n, 3] float32."""
    old = np.seterr(all="ignore")
    try:
        r = radius.astype(F32)[:, None]
        p1 = (center.astype(F32) + r * F32(-1)).tolist()
        p2 = (center.astype(F32) + r).tolist()
    finally:
        np.seterr(**old)
    bmin = np.array([[go_min(a, b) for a, b in zip(u, v)] for u, v in zip(p1, p2)], F32).reshape(-1, 3)
    bmax = np.array([[go_max(a, b) for a, b in zip(u, v)] for u, v in zip(p1, p2)], F32).reshape(-1, 3)
    return bmin, bmax


def calls(m: int, memo=None) -> int:
    """The NewBVH calls a list of m makes (bvh.go:161-180): itself, and for m >= 3 its two halves'."""
    if m <= 2:
        return 1
    memo = {} if memo is None else memo
    if m not in memo:
        memo[m] = 1 + calls(m // 2, memo) + calls(m - m // 2, memo)
    return memo[m]


def axes(seed: int, draw0: int, count: int) -> list:
    """Intn(3) of words draw0 .. draw0 + count - 1 of the host stream."""
    n = np.arange(count, dtype=U64) + U64(draw0)
    blk = n >> U64(2)
    lo, hi = blk & U64(0xFFFFFFFF), blk >> U64(32)
    zero = np.zeros(count, U64)
    w = ref64.philox4x32_10(lo, hi, zero, zero + U64(0x80000000 | HOST_STREAM), U64(seed & 0xFFFFFFFF), U64(seed >> 32))
    word = np.choose((n & U64(3)).astype(np.int64), [np.asarray(x, U64) for x in w])
    return ((word * U64(3)) >> U64(32)).astype(np.int64).tolist()


def compare(bmin: np.ndarray, axis: int, h1, h2):
    """HittableCompare{X,Y,Z} (bvh.go:187-218) of the spheres h1, h2 (indices or index arrays): 1, -1 or 0."""
    diff = bmin[h2, axis] - bmin[h1, axis]  # float32; +-inf and inf - inf = NaN (equal) are meant
    return np.where(diff > 0, 1, np.where(diff < 0, -1, 0))


def sort_func(bmin: np.ndarray, axis: int, h: np.ndarray) -> np.ndarray:
    """slices.SortFunc(h, compare) (bvh.go:176), the stable result."""
    order = np.argsort(-bmin[h, axis], kind="stable")
    out = h[order]
    c = compare(bmin, axis, out[:-1], out[1:])
    if (c > 0).any() or (order[:-1][c == 0] > order[1:][c == 0]).any():
        raise AssertionError("the sort's result is not the comparator's stable order")
    return out


def build(spheres, n: int, seed: int, draw0: int, tables=None):
    """NewBVHFromWorld (bvh.go:138-140) of spheres[0 .. n) in World.Add order.  tables: a scene description whose
    material, texture and texel tables the result points to as well (a scene needs them; the tree does not)."""
    if n < 1:
        raise ValueError("an empty World: NewBVH indexes h[0] (bvh.go:163)")
    raw = np.ctypeslib.as_array(ctypes.cast(spheres, ctypes.POINTER(ctypes.c_float)), shape=(n, 8))
    bmin, bmax = sphere_boxes(raw[:, 0:3], raw[:, 3])
    if np.isnan(bmin).any() or np.isnan(bmax).any():
        raise ValueError("a NaN box: the comparator is no order (out of contract)")
    axis_of = axes(seed, draw0, calls(n))
    lo, hi = bmin.tolist(), bmax.tolist()
    nodes = []  # [bmin, left, bmax, right] in pre-order
    drawn = [0]

    def leaf(i):
        return rtx.ref_prim(rtx.RTX_PRIM_SPHERE, int(i)), lo[i], hi[i]

    def new_bvh(h):  # bvh.go:142-185 -> (ref, box min, box max)
        axis = axis_of[drawn[0]]  # :147, before the size switch
        drawn[0] += 1
        me = len(nodes)
        nodes.append(None)
        if len(h) == 1:  # :162-165
            left = right = leaf(h[0])
        elif len(h) == 2:  # :166-174
            if compare(bmin, axis, h[0], h[1]) > 0:
                left, right = leaf(h[1]), leaf(h[0])
            else:
                left, right = leaf(h[0]), leaf(h[1])
        else:  # :175-179
            h = sort_func(bmin, axis, h)
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
    d.spheres, d.n_spheres = ctypes.cast(spheres, ctypes.POINTER(rtx.Sphere)), n
    if tables is not None:
        t = tables.contents if hasattr(tables, "contents") else tables
        d.materials, d.n_materials, d.textures, d.n_textures = t.materials, t.n_materials, t.textures, t.n_textures
        d.texels, d.n_texels = t.texels, t.n_texels
    p = ctypes.pointer(d)
    p._keep = (arr, roots, spheres, tables)
    return p
