"""Direct light sampling in numpy float32 — TEST INFRASTRUCTURE (the reference of rtx_lights* and rtx_direct*).

Written from the contract in include/rtx.h ("direct light sampling") and the cited lines of the Go
source.  It shares no code with csrc/: the emitter table is its own walk over the scene description, the Philox
blocks are ref64.philox4x32_10's, the visibility is trace_ref.walk(any_hit=True) over the scene's threaded entries.
Every operation is its own float32 ufunc, left-associative as Go evaluates it, widened to float64 exactly where the
contract widens (Len's square root, the sphere UV's Acos / Atan2 through liboracle.so's restatement of Go's).

Textures: SolidColor and Checkered are evaluated here, Perlin noise by liboracle.so's oracle_noise_texture (the oracle's
restatement of NoiseTexture.GetTexture, as the sphere UV goes through its Acos / Atan2).  A caller may pass a
Lambertian's colour in (`albedo`: the attenuation rtx_shade gives for the same hit, which the shade tests hold to the
oracle), which then stands for an image or Perlin albedo; an emitter with an image texture is refused.
"""
from __future__ import annotations

import numpy as np

import ref64
import rtx
import trace_ref

F32, F64, U64, I64 = np.float32, np.float64, np.uint64, np.int64
PI32 = F32(np.pi)  # math.go:48 PiF32
LIGHT_EVENT = 0x40000000  # the light events of the Philox counter


def _dot(a, b):  # vec3.go:137-139, left-associative
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(l, r):  # vec3.go:129-135
    return np.stack([l[..., 1] * r[..., 2] - l[..., 2] * r[..., 1], l[..., 2] * r[..., 0] - l[..., 0] * r[..., 2],
                     l[..., 0] * r[..., 1] - l[..., 1] * r[..., 0]], axis=-1)


def _len(a):  # vec3.go:119-121
    return np.sqrt(_dot(a, a).astype(F64)).astype(F32)


def referenced(desc):
    """The sphere and the quad indices the world references (roots, nodes, lists), as two sorted lists."""
    d = desc.contents if hasattr(desc, "contents") else desc
    spheres, quads, seen = set(), set(), set()
    stack = [int(d.roots[i]) for i in range(d.n_roots)]
    while stack:
        ref = stack.pop()
        if ref in seen:
            continue
        seen.add(ref)
        if ref >= 0:
            stack += [int(d.nodes[ref].left), int(d.nodes[ref].right)]
            continue
        p = ~ref & 0xFFFFFFFF
        kind, idx = p >> 28, p & 0x0FFFFFFF
        if kind == rtx.RTX_PRIM_LIST:
            lst = d.lists[idx]
            stack += [int(d.list_refs[lst.first + k]) for k in range(lst.count)]
        elif kind == rtx.RTX_PRIM_QUAD:
            quads.add(idx)
        else:
            spheres.add(idx)
    return sorted(spheres), sorted(quads)


def lights(desc) -> np.ndarray:
    """The emitter table (rtx.LIGHT_DTYPE): referenced DiffuseLight spheres in sphere-table order, then quads in
    quad-table order; radius <= 0 and areas that are not finite and > 0 left out."""
    sc = desc if isinstance(desc, ref64.Scene) else ref64.Scene(desc)
    spheres, quads = referenced(desc)
    out = []
    old = np.seterr(all="ignore")
    try:
        for i in spheres:
            r = F32(sc.s_radius[i])
            if sc.m_type[sc.s_mat[i]] != rtx.RTX_MAT_DIFFUSE_LIGHT or not r > 0:
                continue
            out.append(((rtx.RTX_PRIM_SPHERE << 28) | i, (F32(4) * PI32) * (r * r)))
        for i in quads:
            if sc.m_type[sc.q_mat[i]] != rtx.RTX_MAT_DIFFUSE_LIGHT:
                continue
            out.append(((rtx.RTX_PRIM_QUAD << 28) | i, _len(_cross(sc.q_u[i], sc.q_v[i]))))
    finally:
        np.seterr(**old)
    out = [(p, a) for p, a in out if np.isfinite(a) and a > 0]
    return np.array(out, dtype=rtx.LIGHT_DTYPE)


def _texture(sc, tid, p):
    """SolidColor / Checkered GetTexture (materials.go:127-137, 155-157) of texture `tid` at the points p [m, 3]."""
    kind = int(sc.t_type[tid])
    if kind == rtx.RTX_TEX_SOLID:
        return np.broadcast_to(sc.t_even[tid].astype(F32), p.shape).copy()
    if kind == rtx.RTX_TEX_CHECKERED:
        inv = F32(1) / F32(sc.t_scale[tid])
        cell = [np.floor((inv * p[:, c]).astype(F64)).astype(I64) for c in range(3)]
        par = (cell[0] + cell[1] + cell[2]) % 2
        return np.where((par == 0)[:, None], sc.t_even[tid].astype(F32)[None], sc.t_odd[tid].astype(F32)[None])
    if kind == rtx.RTX_TEX_NOISE:  # NoiseTexture.GetTexture as liboracle.so restates it (materials.go:280-288)
        import ctypes

        import oracle_binding as ob
        f = ob.load().oracle_noise_texture
        off = int(sc.t_off[tid])
        tab = np.ascontiguousarray(sc.texels[off: off + 1536], np.uint32)
        words = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        g = np.array([f(words, float(sc.t_scale[tid]), (ctypes.c_float * 3)(*[float(c) for c in q])) for q in p], F32)
        return np.repeat(g[:, None], 3, axis=1)
    raise ValueError(f"texture kind {kind}: pass the colour in (direct_ref's docstring)")


def _unit01(w):  # rand.Float32 of a Philox word: float32(w >> 8) * 2^-24
    return (w >> U64(8)).astype(F32) * F32(2.0 ** -24)


def sample(desc, entries, hits, keys, seed: int, albedo=None) -> np.ndarray:
    """rtx_direct for records (hits: rtx.HIT_DTYPE, keys: rtx.KEY_DTYPE) of the scene `desc` whose threaded entries
    are `entries` (rtx_scene_export's bytes, or trace_ref.entries_of(desc)).  albedo [n, 3]: the Lambertian's colour
    where its texture is not evaluated here.  Returns rtx.DIRECT_DTYPE records."""
    sc = ref64.Scene(desc)
    tab = lights(desc)
    L = len(tab)
    hits, keys = np.asarray(hits).reshape(-1), np.asarray(keys).reshape(-1)
    n = len(hits)
    out = np.zeros(n, rtx.DIRECT_DTYPE)
    old = np.seterr(all="ignore")
    try:
        mat = hits["material"].astype(I64)
        ok = (hits["prim"] != rtx.RTX_HIT_NONE) & (mat < len(sc.m_type))
        lam = ok & (sc.m_type[np.where(ok, mat, 0)] == rtx.RTX_MAT_LAMBERTIAN) & (L > 0)
        k = np.nonzero(lam)[0]
        if not k.size:
            return out
        p, nrm = hits["point"][k].astype(F32), hits["normal"][k].astype(F32)
        pix, smp = keys["pixel"][k].astype(U64), keys["sample"][k].astype(U64)
        ev = (keys["event"][k].astype(U64) | U64(LIGHT_EVENT))
        k0, k1 = U64(seed & 0xFFFFFFFF), U64((seed >> 32) & 0xFFFFFFFF)
        b0 = ref64.philox4x32_10(pix, smp, ev, U64(0), k0, k1)
        fL = F32(L)
        j = np.minimum((_unit01(b0[0]) * fL).astype(np.uint32), np.uint32(L - 1)).astype(I64)
        kind, idx = tab["prim"][j] >> 28, (tab["prim"][j] & 0x0FFFFFFF).astype(I64)
        area = tab["area"][j].astype(F32)
        m = len(k)
        q, nl = np.zeros((m, 3), F32), np.zeros((m, 3), F32)
        lu, lv = np.zeros(m, F32), np.zeros(m, F32)
        draws = np.ones(m, I64)
        emat = np.zeros(m, I64)

        s = np.nonzero(kind == rtx.RTX_PRIM_QUAD)[0]
        if s.size:
            x1, x2 = _unit01(b0[1][s]), _unit01(b0[2][s])
            qi = idx[s]
            q[s] = (sc.q_q[qi] + sc.q_u[qi] * x1[:, None]) + sc.q_v[qi] * x2[:, None]
            nl[s], lu[s], lv[s] = sc.q_n[qi], x1, x2
            draws[s] += 2
            emat[s] = sc.q_mat[qi]
        s = np.nonzero(kind == rtx.RTX_PRIM_SPHERE)[0]
        if s.size:
            d = np.zeros((len(s), 3), F32)
            pend, a = np.arange(len(s)), 1
            while pend.size:  # vec3.go:182-190, attempt a on block (.., a)
                g = s[pend]
                bb = ref64.philox4x32_10(pix[g], smp[g], ev[g], U64(a), k0, k1)
                v = np.stack([F32(-1) + _unit01(bb[c]) * F32(2) for c in range(3)], axis=-1)  # math.go:30-32
                draws[g] += 3
                acc = _dot(v, v) < F32(1)
                va = v[acc]
                d[pend[acc]] = va * (F32(1) / _len(va))[:, None]  # vec3.go:103-107
                pend, a = pend[~acc], a + 1
            si = idx[s]
            q[s] = sc.s_center[si] + d * sc.s_radius[si][:, None]
            nl[s] = d
            acos, atan2 = trace_ref._go_math()
            theta = np.array([acos(-float(y)) for y in d[:, 1]], F64).astype(F32)  # hittables.go:122
            phi = (np.array([atan2(-float(z), float(x)) for z, x in zip(d[:, 2], d[:, 0])], F64) + np.pi).astype(F32)
            lu[s] = (phi + trace_ref._UV_SHIFT) / trace_ref._UV_TWO_PI  # :125
            lv[s] = theta / PI32  # :126
            emat[s] = sc.s_mat[si]

        w = q - p
        d2 = _dot(w, w)
        dist = np.sqrt(d2.astype(F64)).astype(F32)
        cs = _dot(nrm, w) / dist
        cl = np.abs(_dot(nl, w)) / dist
        sampled = (d2 > 0) & (cs > 0) & (cl > 0)
        geom = (((cs * cl) * area) * fL) / (PI32 * d2)

        a_col = np.zeros((m, 3), F32)
        le = np.zeros((m, 3), F32)
        for t in np.unique(sc.m_tex[mat[k]]):
            r = np.nonzero(sc.m_tex[mat[k]] == t)[0]
            if albedo is not None and int(sc.t_type[t]) not in (rtx.RTX_TEX_SOLID, rtx.RTX_TEX_CHECKERED):
                a_col[r] = np.asarray(albedo, F32).reshape(-1, 3)[k[r]]
            else:
                a_col[r] = _texture(sc, t, p[r])
        for t in np.unique(sc.m_tex[emat]):
            r = np.nonzero(sc.m_tex[emat] == t)[0]
            le[r] = _texture(sc, t, q[r])
        rad = (a_col * le) * geom[:, None]

        rays = np.zeros(m, rtx.RAY_DTYPE)
        rays["origin"], rays["tmin"], rays["dir"], rays["tmax"] = p, F32(0.001), w, F32(0.999)
        scene = entries if isinstance(entries, trace_ref.Scene) else trace_ref.Scene(entries, desc)
        blocked = np.zeros(m, bool)
        sm = np.nonzero(sampled)[0]
        if sm.size:
            blocked[sm] = trace_ref.walk(scene, rays[sm], F32, uv=False, any_hit=True).mask
        visible = sampled & ~blocked

        rec = np.zeros(m, rtx.DIRECT_DTYPE)
        rec["light"], rec["rng_draws"] = j, draws
        rec["flags"] = np.where(sampled, rtx.RTX_DIRECT_SAMPLED, 0) | np.where(visible, rtx.RTX_DIRECT_VISIBLE, 0)
        rec["radiance"][sampled] = rad[sampled]
        rec["geom"][sampled] = geom[sampled]
        for f in ("origin", "tmin", "dir", "tmax"):
            rec["ray"][f][sampled] = rays[f][sampled]
        out[k] = rec
        return out
    finally:
        np.seterr(**old)
