"""Hittable.Hit for a batch of rays in numpy — TEST INFRASTRUCTURE (the reference of rtx_trace*).

The project's own reading of the Go source of TwFlem/raytracer-go (cited file:line below), written
from it and from the layouts of include/rtx.h and csrc/rtx_layout.h.  It takes a scene as the threaded
entries rtx_scene_export returns (the reference walk's pre-order: a node, then its first child's
subtree, then its second's, every node naming the entry after its subtree; a nested World's items one
after another) plus the scene description (the quad records), and rays as rtx.RAY_DTYPE.

  scan   World.Hit over every primitive in the reference walk's order (hittables.go:55-72), each with
         the ray's own Interval{tmin, tmax}: the first minimum wins, exact ties are reported.  No box
         is tested, so this is what any correct tree returns.  (tests/ref64.py's `closest` with the
         ray's own interval.)
  walk   the threaded walk itself: Aabb.Hit as InBoundary states it (bvh.go:52-61, 84-102) with
         (tmin, running bound), Sphere.Hit / Quad.Hit against the running bound, vectorised over rays
         and stepping while any ray is active.  Returns the hits and, per ray, node_visits and
         prim_tests in the units of rtx_trace_stats.

Both run in np.float32 (every operation its own float32 ufunc, left-associative as Go evaluates it,
widened to float64 exactly where Go widens: math.Sqrt, math.Abs, Acos, Atan2) and in np.float64.
Interval.In is strict at both ends (bvh.go:18-20).  Sphere UV (hittables.go:122-126) goes through
Go's own Acos / Atan2 as liboracle.so restates them (oracle_go_acos, oracle_go_atan2), and its typed
float32 constants fold operation by operation, as the Go compiler folds typed constants:
5*PiF32/12 = (5 * PiF32) / 12 in float32.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle_binding as ob
import ref64
import rtx

F32, F64, I64 = np.float32, np.float64, np.int64

_PI32 = F32(np.pi)  # math.go:48
_UV_SHIFT = F32(5) * _PI32 / F32(12)  # hittables.go:125, folded in float32 step by step
_UV_TWO_PI = F32(2) * _PI32

_go = None


def _go_math():
    global _go
    if _go is None:
        L = ob.load()
        for f, n in ((L.oracle_go_acos, 1), (L.oracle_go_atan2, 2)):
            f.argtypes = [ctypes.c_double] * n
            f.restype = ctypes.c_double
        _go = (L.oracle_go_acos, L.oracle_go_atan2)
    return _go


def entries_of(desc) -> np.ndarray:
    """The threaded entries of a scene description, [n, 8] uint32, as rtx_scene_export returns them
    (rtx_layout.h: node a = (bmin, escape), b = (bmax, -1); sphere a = (centre, radius), b = (radius *
    radius in float32, sphere, 0, material); quad a = (normal, D), b = (quad, 0, 0, -2)): every root in
    turn, left before right, a one-element split's child once, a nested World's items in Add order."""
    d = desc.contents if hasattr(desc, "contents") else desc
    rows = []

    def row(a, b):
        r = np.zeros(8, np.uint32)
        for k, v in enumerate(list(a) + list(b)):
            if isinstance(v, (float, np.floating)):
                r[k: k + 1].view(F32)[0] = v
            else:
                r[k: k + 1].view(np.int32)[0] = v
        return r

    def emit(ref):
        if ref >= 0:
            n = d.nodes[ref]
            me = len(rows)
            rows.append(None)
            emit(n.left)
            if n.right != n.left:
                emit(n.right)
            rows[me] = row([F32(v) for v in n.bmin] + [len(rows)], [F32(v) for v in n.bmax] + [-1])
            return
        p = ~ref & 0xFFFFFFFF
        kind, idx = p >> 28, p & 0x0FFFFFFF
        if kind == rtx.RTX_PRIM_LIST:
            lst = d.lists[idx]
            for k in range(lst.count):
                emit(d.list_refs[lst.first + k])
        elif kind == rtx.RTX_PRIM_QUAD:
            q = d.quads[idx]
            rows.append(row([F32(v) for v in q.normal] + [F32(q.d)], [idx, 0, 0, -2]))
        else:
            s = d.spheres[idx]
            r = F32(s.radius)
            rows.append(row([F32(v) for v in s.center] + [r], [F32(r * r), idx, 0, int(s.material)]))

    for i in range(d.n_roots):
        emit(d.roots[i])
    return np.array(rows, np.uint32).reshape(-1, 8)


class Scene:
    """The entries ([n, 8] uint32, or rtx_scene_export's bytes) and the quad records of `desc`."""

    def __init__(self, entries, desc):
        e = np.frombuffer(entries, np.uint32) if isinstance(entries, (bytes, bytearray)) else np.asarray(entries, np.uint32)
        e = e.reshape(-1, 8)
        self.entries = e
        fl = e.view(F32)
        self.tag = e[:, 7].view(np.int32).astype(I64)
        self.is_node, self.is_quad, self.is_sphere = self.tag == -1, self.tag == -2, self.tag >= 0
        self.a3, self.aw, self.b3 = fl[:, 0:3], fl[:, 3], fl[:, 4:7]
        self.escape = e[:, 3].astype(I64)
        self.sphere = e[:, 5].astype(I64)
        self.quad = e[:, 4].astype(I64)
        q = ref64.Scene(desc)
        self.q_q, self.q_u, self.q_v, self.q_w, self.q_mat = q.q_q, q.q_u, q.q_v, q.q_w, q.q_mat
        self.prims = np.nonzero(~self.is_node)[0]  # in the reference walk's order


class Hits:
    """One record per ray in dtype T; `entry` is the winning entry (-1: a miss), `tie` scan's exact ties."""

    def __init__(self, n, T):
        self.T = T
        self.entry = np.full(n, -1, I64)
        self.t = np.full(n, np.inf, T)
        self.prim = np.full(n, rtx.RTX_HIT_NONE, np.uint32)
        self.material = np.zeros(n, np.uint32)
        self.front = np.zeros(n, np.uint32)
        self.point, self.normal = np.zeros((n, 3), T), np.zeros((n, 3), T)
        self.u, self.v = np.zeros(n, T), np.zeros(n, T)
        self.tie = np.zeros(n, bool)
        self.node_visits = np.zeros(n, I64)
        self.prim_tests = np.zeros(n, I64)

    @property
    def mask(self):
        return self.entry >= 0

    def records(self, uv: bool = True) -> np.ndarray:
        """The rtx_hit records (rtx.HIT_DTYPE) a float32 run stands for; u, v zero without RTX_TRACE_UV."""
        assert self.T is F32
        out = np.zeros(len(self.t), rtx.HIT_DTYPE)
        out["t"], out["prim"], out["material"], out["front_face"] = self.t, self.prim, self.material, self.front
        out["point"], out["normal"] = self.point, self.normal
        if uv:
            out["u"], out["v"] = self.u, self.v
        return out


def _dot(a, b):  # vec3.go:137-139, left-associative
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(l, r):  # vec3.go:129-135
    return np.stack([l[..., 1] * r[..., 2] - l[..., 2] * r[..., 1], l[..., 2] * r[..., 0] - l[..., 0] * r[..., 2],
                     l[..., 0] * r[..., 1] - l[..., 1] * r[..., 0]], axis=-1)


def _sphere(T, o, d, c, rad, tmin, bound):
    """Sphere.Hit, hittables.go:96-116: (t, accepted) for broadcastable o, d [.., 3], c [.., 3], rad, tmin, bound."""
    ax, ay, az = o[..., 0] - c[..., 0], o[..., 1] - c[..., 1], o[..., 2] - c[..., 2]  # :97
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    a = dx * dx + dy * dy + dz * dz  # :98
    hb = dx * ax + dy * ay + dz * az  # :99
    cc = (ax * ax + ay * ay + az * az) - rad * rad  # :100
    disc = hb * hb - a * cc  # :102
    sq = np.sqrt(disc.astype(F64)).astype(T)  # :108
    r1, r2 = (-hb - sq) / a, (-hb + sq) / a  # :110, :112
    in1, in2 = (tmin < r1) & (r1 < bound), (tmin < r2) & (r2 < bound)  # Interval.In, bvh.go:18-20
    return np.where(in1, r1, r2), (in1 | in2) & ~(disc < 0)  # :104


def _quad(T, o, d, nrm, dd, qq, qu, qv, qw, tmin, bound):
    """Quad.Hit, hittables.go:167-194: (t, accepted, alpha, beta)."""
    den = _dot(d, nrm)  # :168
    par = np.abs(den.astype(F64)) < 1e-8  # :170
    t = (dd - _dot(nrm, o)) / den  # :174
    ok = (tmin < t) & (t < bound) & ~par  # :176
    ph = (d * t[..., None] + o) - qq  # :180-181 (At: ray.go:25-30)
    al = _dot(qw, _cross(ph, qv))  # :182
    be = _dot(qw, _cross(qu, ph))  # :183
    outside = (al < 0) | (T(1) < al) | (be < 0) | (T(1) < be)  # InPlane :192-194 (a NaN is inside)
    return t, ok & ~outside, al, be


def _box(T, o, d, mn, mx, tmin, bound):
    """Aabb.Hit, bvh.go:52-61, with InBoundary (:84-102) per axis; the interval only shrinks and a NaN slab
    distance changes nothing, so the three results and-ed are the early exits' result."""
    lo, hi = np.array(tmin, T, copy=True), np.array(bound, T, copy=True)
    ok = np.ones(lo.shape, bool)
    for k in range(3):
        inv = T(1) / d[:, k]
        t0, t1 = (mn[:, k] - o[:, k]) * inv, (mx[:, k] - o[:, k]) * inv
        neg = inv < 0
        t0, t1 = np.where(neg, t1, t0), np.where(neg, t0, t1)
        lo = np.where(t0 > lo, t0, lo)
        hi = np.where(t1 < hi, t1, hi)
        ok &= lo < hi
    return ok


def _rays(rays, T):
    r = np.asarray(rays).reshape(-1)
    assert r.dtype == rtx.RAY_DTYPE
    return r["origin"].astype(T), r["dir"].astype(T), r["tmin"].astype(T), r["tmax"].astype(T)


def _finish(sc: Scene, T, o, d, h: Hits, uv: bool):
    """NewHitInfo (hittables.go:22-37) of every hit in h (entry, t set)."""
    k = np.nonzero(h.entry >= 0)[0]
    if not k.size:
        return
    j, t = h.entry[k], h.t[k]
    point = d[k] * t[:, None] + o[k]  # ray.go:25-30
    normal = np.zeros((len(k), 3), T)
    u, v = np.zeros(len(k), T), np.zeros(len(k), T)
    isq = sc.is_quad[j]
    s = np.nonzero(~isq)[0]
    if s.size:  # hittables.go:118-126
        js = j[s]
        nv = (point[s] - sc.a3[js].astype(T)) * sc.aw[js].astype(T)[:, None]  # :119
        l = np.sqrt(_dot(nv, nv).astype(F64)).astype(T)  # vec3.go:103-107
        nv = nv * (T(1) / l)[:, None]
        normal[s] = nv
        h.prim[k[s]] = (rtx.RTX_PRIM_SPHERE << 28) | sc.sphere[js]
        h.material[k[s]] = sc.tag[js]
        if uv:
            acos, atan2 = _go_math()
            ny, nz, nx = nv[:, 1].astype(F64), nv[:, 2].astype(F64), nv[:, 0].astype(F64)
            theta = np.array([acos(-float(y)) for y in ny], F64).astype(T)  # :122
            phi = (np.array([atan2(-float(z), float(x)) for z, x in zip(nz, nx)], F64) + np.pi).astype(T)  # :123
            u[s] = (phi + T(_UV_SHIFT)) / T(_UV_TWO_PI)  # :125
            v[s] = theta / T(_PI32)  # :126
    q = np.nonzero(isq)[0]
    if q.size:  # hittables.go:180-190
        jq = j[q]
        qi = sc.quad[jq]
        normal[q] = sc.a3[jq].astype(T)
        h.prim[k[q]] = (rtx.RTX_PRIM_QUAD << 28) | qi
        h.material[k[q]] = sc.q_mat[qi]
        if uv:
            ph = point[q] - sc.q_q[qi].astype(T)
            w = sc.q_w[qi].astype(T)
            u[q] = _dot(w, _cross(ph, sc.q_v[qi].astype(T)))
            v[q] = _dot(w, _cross(sc.q_u[qi].astype(T), ph))
    front = _dot(d[k], normal) < 0  # hittables.go:23
    normal = np.where(front[:, None], normal, normal * T(-1))  # :24-26
    h.point[k], h.normal[k], h.front[k], h.u[k], h.v[k] = point, normal, front, u, v


def scan(sc: Scene, rays, dtype, uv: bool = True) -> Hits:
    """World.Hit over every primitive entry in the reference walk's order; `tie`: an exact tie for the minimum."""
    T = np.dtype(dtype).type
    old = np.seterr(all="ignore")
    try:
        o, d, tmin, tmax = _rays(rays, T)
        n, P = len(o), len(sc.prims)
        h = Hits(n, T)
        if P == 0 or n == 0:
            return h
        tall = np.full((n, P), np.inf, T)
        oo, dd_, lo, hi = o[:, None, :], d[:, None, :], tmin[:, None], tmax[:, None]
        cols = np.nonzero(sc.is_sphere[sc.prims])[0]
        if cols.size:
            j = sc.prims[cols]
            t, ok = _sphere(T, oo, dd_, sc.a3[j].astype(T)[None], sc.aw[j].astype(T)[None], lo, hi)
            tall[:, cols] = np.where(ok, t, T(np.inf))
        cols = np.nonzero(sc.is_quad[sc.prims])[0]
        if cols.size:
            j = sc.prims[cols]
            qi = sc.quad[j]
            t, ok, _, _ = _quad(T, oo, dd_, sc.a3[j].astype(T)[None], sc.aw[j].astype(T)[None], sc.q_q[qi].astype(T)[None],
                                sc.q_u[qi].astype(T)[None], sc.q_v[qi].astype(T)[None], sc.q_w[qi].astype(T)[None], lo, hi)
            tall[:, cols] = np.where(ok, t, T(np.inf))
        best = np.argmin(tall, axis=1)  # the first minimum: World.Hit's strict `<` against the running bound
        tb = tall[np.arange(n), best]
        # (an accepted root is < tmax <= +inf, so +inf marks "no primitive accepted")
        hit = tb < T(np.inf)
        h.tie = hit & ((tall == tb[:, None]).sum(axis=1) > 1)
        h.entry = np.where(hit, sc.prims[best], -1)
        h.t = np.where(hit, tb, T(np.inf))
        _finish(sc, T, o, d, h, uv)
        return h
    finally:
        np.seterr(**old)


def walk(sc: Scene, rays, dtype, uv: bool = True, any_hit: bool = False) -> Hits:
    """The reference's walk over the threaded entries (bvh.go:220-249, hittables.go:55-72), every ray at once.
    any_hit: a ray stops at the first primitive it accepts (RTX_TRACE_ANY)."""
    T = np.dtype(dtype).type
    old = np.seterr(all="ignore")
    try:
        o, d, tmin, tmax = _rays(rays, T)
        n, E = len(o), len(sc.entries)
        h = Hits(n, T)
        pos = np.zeros(n, I64)
        bound = tmax.copy()
        stopped = np.zeros(n, bool)
        while True:
            act = np.nonzero((pos < E) & ~stopped)[0]
            if not act.size:
                break
            j = pos[act]
            k = np.nonzero(sc.is_node[j])[0]
            if k.size:  # Aabb.Hit with (tmin, the running bound): descend, or skip the subtree
                r, jk = act[k], j[k]
                ok = _box(T, o[r], d[r], sc.a3[jk].astype(T), sc.b3[jk].astype(T), tmin[r], bound[r])
                h.node_visits[r] += 1
                pos[r] = np.where(ok, jk + 1, sc.escape[jk])
            k = np.nonzero(sc.is_sphere[j])[0]
            if k.size:
                r, jk = act[k], j[k]
                t, ok = _sphere(T, o[r], d[r], sc.a3[jk].astype(T), sc.aw[jk].astype(T), tmin[r], bound[r])
                h.prim_tests[r] += 1
                pos[r] = jk + 1
                bound[r[ok]], h.t[r[ok]], h.entry[r[ok]] = t[ok], t[ok], jk[ok]
                if any_hit:
                    stopped[r[ok]] = True
            k = np.nonzero(sc.is_quad[j])[0]
            if k.size:
                r, jk = act[k], j[k]
                qi = sc.quad[jk]
                t, ok, _, _ = _quad(T, o[r], d[r], sc.a3[jk].astype(T), sc.aw[jk].astype(T), sc.q_q[qi].astype(T),
                                    sc.q_u[qi].astype(T), sc.q_v[qi].astype(T), sc.q_w[qi].astype(T), tmin[r], bound[r])
                h.prim_tests[r] += 1
                pos[r] = jk + 1
                bound[r[ok]], h.t[r[ok]], h.entry[r[ok]] = t[ok], t[ok], jk[ok]
                if any_hit:
                    stopped[r[ok]] = True
        _finish(sc, T, o, d, h, uv)
        return h
    finally:
        np.seterr(**old)


def kept(h32: Hits, h64: Hits) -> np.ndarray:
    """The rays a float32 implementation over ANY tree is held to: scan in float32 and in float64 agree on the
    primitive and the front face and neither meets an exact tie."""
    return (h32.prim == h64.prim) & (h32.front == h64.front) & ~h32.tie & ~h64.tie
