"""Multiple importance sampling of the direct light in numpy float32 — TEST INFRASTRUCTURE (the reference of
rtx_prim_lights and rtx_emitter_weight*, and of the light sample's weight).

Written from the contract in include/rtx.h ("multiple importance sampling of the direct light").  It
shares no code with csrc/: the emitter table is direct_ref.lights' own walk over the scene description, and every
operation is its own float32 ufunc, left-associative, widened to float64 exactly where the contract widens (Len's
square root)."""
from __future__ import annotations

import numpy as np

import direct_ref
import ref64
import rtx

F32, F64, I64 = np.float32, np.float64, np.int64
PI32 = direct_ref.PI32


def prim_lights(desc):
    """(rtx.PRIM_LIGHT_DTYPE array: the caller's spheres, then its quads; the number of spheres) from the emitter
    table: area and table index of the primitives in it, 0 and RTX_LIGHT_NONE for every other."""
    d = desc.contents if hasattr(desc, "contents") else desc
    ns, nq = int(d.n_spheres), int(d.n_quads)
    out = np.zeros(ns + nq, rtx.PRIM_LIGHT_DTYPE)
    out["light"] = rtx.RTX_LIGHT_NONE
    for j, (prim, area) in enumerate(direct_ref.lights(desc)):
        kind, idx = int(prim) >> 28, int(prim) & 0x0FFFFFFF
        k = idx if kind == rtx.RTX_PRIM_SPHERE else ns + idx
        out[k] = (area, j)
    return out, ns


def wl(g):
    """The light sample's weight of its own geom: 1 / (1 + g * g), float32, each operation rounded."""
    g = np.asarray(g, F32)
    return F32(1) / (F32(1) + g * g)


def weight(desc, from_hits, hits) -> np.ndarray:
    """rtx_emitter_weight for pairs of rtx.HIT_DTYPE records (the hit a bounce left, the hit it found) of the scene
    `desc`.  Returns rtx.EMITTER_WEIGHT_DTYPE records."""
    sc = ref64.Scene(desc)
    tab, ns = prim_lights(desc)
    nq = len(tab) - ns
    L = int((tab["light"] != rtx.RTX_LIGHT_NONE).sum())
    fr, h = np.asarray(from_hits).reshape(-1), np.asarray(hits).reshape(-1)
    n, nm = len(h), len(sc.m_type)
    out = np.zeros(n, rtx.EMITTER_WEIGHT_DTYPE)
    out["weight"], out["light"] = F32(1), rtx.RTX_LIGHT_NONE
    if n == 0:
        return out
    old = np.seterr(all="ignore")
    try:
        fm, hm = fr["material"].astype(I64), h["material"].astype(I64)
        f_ok = (fr["prim"] != rtx.RTX_HIT_NONE) & (fm < nm)
        h_ok = (h["prim"] != rtx.RTX_HIT_NONE) & (hm < nm)
        pair = (f_ok & h_ok & (sc.m_type[np.where(f_ok, fm, 0)] == rtx.RTX_MAT_LAMBERTIAN) &
                (sc.m_type[np.where(h_ok, hm, 0)] == rtx.RTX_MAT_DIFFUSE_LIGHT))
        kind, idx = h["prim"] >> 28, (h["prim"] & 0x0FFFFFFF).astype(I64)
        sph, quad = (kind == rtx.RTX_PRIM_SPHERE) & (idx < ns), (kind == rtx.RTX_PRIM_QUAD) & (idx < nq)
        known = pair & (sph | quad) & (len(tab) > 0)
        slot = np.where(known, np.where(sph, idx, ns + idx), 0)
        safe = tab if len(tab) else np.zeros(1, rtx.PRIM_LIGHT_DTYPE)
        area = np.where(known, safe["area"][slot], F32(0)).astype(F32)
        light = np.where(known, safe["light"][slot], rtx.RTX_LIGHT_NONE).astype(np.uint32)

        w = h["point"].astype(F32) - fr["point"].astype(F32)
        d2 = direct_ref._dot(w, w)
        dist = np.sqrt(d2.astype(F64)).astype(F32)  # vec3.go:119-121
        cs = direct_ref._dot(fr["normal"].astype(F32), w) / dist
        cl = np.abs(direct_ref._dot(h["normal"].astype(F32), w)) / dist
        g = (((cs * cl) * area) * F32(L)) / (PI32 * d2)
        weighted = pair & (area > 0) & (d2 > 0) & ~np.isnan(g)
        wb = F32(1) - F32(1) / (F32(1) + g * g)
        out["weight"] = np.where(weighted, wb, F32(1))
        out["geom"] = np.where(weighted, g, F32(0))
        out["light"] = light
        out["flags"] = np.where(weighted, rtx.RTX_EMITTER_WEIGHTED, 0)
        return out
    finally:
        np.seterr(**old)
