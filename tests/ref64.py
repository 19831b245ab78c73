"""An independent path tracer in numpy — TEST INFRASTRUCTURE (the second opinion).

Written from the Go source of TwFlem/raytracer-go (cited file:line below), the RNG contract of
DESIGN.md §3 and the table layouts of include/rtx.h.  It shares no code with oracle/oracle.c,
csrc/rtx_device.h or host/: it imports `rtx` for the ctypes structs alone and loads no native
library for anything it computes.

  - No BVH: the closest hit is a scan over every primitive with the primitive's own Hit,
    Interval.In strict (bvh.go:18-20) and tmin = 0.001 (ray.go:38).  The scan is World.Hit's
    (hittables.go:55-72): the first primitive in index order wins an exact tie.  A tree visits
    in another order, so a sample that meets a tie is reported (`tie`) and left out by callers.
  - Vectorised over samples and parametrised by dtype.  With np.float32 every operation is its
    own float32 ufunc, left-associative as Go evaluates it, widened to float64 exactly where
    the Go code widens (math.Sqrt, Acos, Atan2, Pow, Floor, Sin, Abs, Min); with np.float64 the
    same code runs in double.  numpy's arccos, arctan2, sin and power stand for Go's.
  - Its own Philox4x32-10 in uint64 arithmetic; one block per (pixel y*W+x, sample, event,
    attempt), u = float(w >> 8) * 2^-24.
  - Colours are combined in the reference's recursive order (ray.go:48-50).

Per sample it returns the colour, a decision signature (one integer row: disk attempts, then per
segment the primitive, root, front face, scatter branch, unit-sphere attempts, checker parity,
texel index and Perlin lattice cells) and its own counters in the units of rtx_stats: segments =
world.Hit calls, hits, rng_draws = Float32() calls as Go makes them (4 per camera ray + 2 per
further disk attempt, 3 per unit-sphere attempt, 1 for a Dielectric that can refract),
texel_fetches = ImageTexture lookups.

A sample is KEPT when the float32 and the float64 run decide alike (`Case`); a float32
implementation is held to the float64 colours on those samples only.
"""
from __future__ import annotations

import ctypes

import numpy as np

import rtx

F32, F64, U64, I64 = np.float32, np.float64, np.uint64, np.int64

# ---- Philox4x32-10 (Salmon et al., SC'11) ---------------------------------------------------
_M0, _M1 = U64(0xD2511F53), U64(0xCD9E8D57)
_W0, _W1 = U64(0x9E3779B9), U64(0xBB67AE85)
_LO = U64(0xFFFFFFFF)
_S32 = U64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four output words (uint64 arrays holding 32-bit values) of counter (c0..c3), key (k0, k1)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=U64) for a in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


# ---- tables -----------------------------------------------------------------------------------
def _words(ptr, n, words):
    if n == 0:
        return np.zeros((0, words), np.uint32)
    a = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint32)), shape=(n * words,))
    return np.array(a, dtype=np.uint32).reshape(n, words)


class Scene:
    """The primitive, material and texture tables of an rtx.SceneDesc (nodes, roots, lists ignored)."""

    def __init__(self, desc):
        d = desc.contents if hasattr(desc, "contents") else desc
        assert isinstance(d, rtx.SceneDesc)
        s = _words(d.spheres, d.n_spheres, 8)  # rtx_sphere: center[3], radius, material
        self.s_center, self.s_radius, self.s_mat = s[:, 0:3].view(F32), s[:, 3].view(F32), s[:, 4].astype(I64)
        q = _words(d.quads, d.n_quads, 20)  # rtx_quad: q, material, u, d, v, -, w, -, normal, -
        self.q_q, self.q_mat, self.q_u, self.q_d = q[:, 0:3].view(F32), q[:, 3].astype(I64), q[:, 4:7].view(F32), \
            q[:, 7].view(F32)
        self.q_v, self.q_w, self.q_n = q[:, 8:11].view(F32), q[:, 12:15].view(F32), q[:, 16:19].view(F32)
        m = _words(d.materials, d.n_materials, 8)  # rtx_material: type, texture, fuzz, ior, albedo[3]
        self.m_type, self.m_tex = m[:, 0].astype(I64), m[:, 1].astype(I64)
        self.m_fuzz, self.m_ior, self.m_albedo = m[:, 2].view(F32), m[:, 3].view(F32), m[:, 4:7].view(F32)
        t = _words(d.textures, d.n_textures, 12)  # rtx_texture: type, scale, w, h, even[3], offset, odd[3]
        self.t_type, self.t_scale = t[:, 0].astype(I64), t[:, 1].view(F32)
        self.t_w, self.t_h, self.t_off = t[:, 2].astype(I64), t[:, 3].astype(I64), t[:, 7].astype(I64)
        self.t_even, self.t_odd = t[:, 4:7].view(F32), t[:, 8:11].view(F32)
        self.texels = _words(d.texels, int(d.n_texels), 1).reshape(-1)
        self.n_spheres, self.n_quads = int(d.n_spheres), int(d.n_quads)


class Result:
    def __init__(self, n, dtype):
        self.colour = np.zeros((n, 3), dtype)
        self.tie = np.zeros(n, bool)
        self.segments = np.zeros(n, I64)
        self.hits = np.zeros(n, I64)
        self.rng_draws = np.zeros(n, I64)
        self.texel_fetches = np.zeros(n, I64)
        self.abs_used = np.zeros(n, bool)  # refract took math.Abs of a negative number (vec3.go:219)
        self.sig = None
        self.dump = []

    def counters(self, mask=None) -> dict:
        m = slice(None) if mask is None else mask
        return {"samples": int(self.segments[m].size), "segments": int(self.segments[m].sum()),
                "hits": int(self.hits[m].sum()), "rng_draws": int(self.rng_draws[m].sum()),
                "texel_fetches": int(self.texel_fetches[m].sum())}


SIG_COLS = 10  # per segment: prim, root, front, branch, attempts, parity, texel, cell, near-zero, spare
BR_EMIT, BR_LAMBERT, BR_METAL, BR_ABSORBED, BR_REFLECT_TIR, BR_REFLECT_SCHLICK, BR_REFRACT = 0, 1, 2, 3, 4, 5, 6

_PI32 = F32(np.pi)  # math.go:48 PiF32
_UV_SHIFT = F32(5.0 * np.pi / 12.0)  # hittables.go:125: the constant 5*PiF32/12 as a float32
_UV_TWO_PI = F32(2.0 * float(_PI32))  # hittables.go:125: 2*PiF32
_TMIN = F32(0.001)  # ray.go:38
_NEAR_ZERO = F32(1e-8)  # vec3.go:168
_COL_SCALE = F32(1.0 / 65535.0)  # materials.go:188


def trace(desc, cam, seed: int, samples, dtype, dump: bool = False) -> Result:
    """GetRay + GetColor (camera.go:265-287, ray.go:32-54) of every (x, y, k) in `samples`."""
    T = np.dtype(dtype).type
    sc = desc if isinstance(desc, Scene) else Scene(desc)
    S = np.asarray(samples, I64).reshape(-1, 3)
    N = len(S)
    res = Result(N, T)
    old = np.seterr(all="ignore")
    try:
        _trace(sc, cam, int(seed), S, T, res, dump)
    finally:
        np.seterr(**old)
    return res


def _trace(sc, cam, seed, S, T, res, dump):
    N = len(S)
    wide = lambda a: np.asarray(a).astype(F64)  # noqa: E731  float64(x)
    nar = lambda a: np.asarray(a).astype(T)  # noqa: E731  float32(...)

    def dot(a, b):  # vec3.go:137-139, left-associative
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]

    def unit(a):  # vec3.go:103-107: Scale(1 / float32(math.Sqrt(float64(LenSq))))
        l = nar(np.sqrt(wide(dot(a, a))))
        return a * (T(1) / l)[:, None]

    def cross(l, r):  # vec3.go:129-135
        return np.stack([l[..., 1] * r[..., 2] - l[..., 2] * r[..., 1], l[..., 2] * r[..., 0] - l[..., 0] * r[..., 2],
                         l[..., 0] * r[..., 1] - l[..., 1] * r[..., 0]], axis=-1)

    pix = (S[:, 1] * int(cam.image_width) + S[:, 0]).astype(U64)
    smp = S[:, 2].astype(U64)
    k0, k1 = U64(seed & 0xFFFFFFFF), U64((seed >> 32) & 0xFFFFFFFF)

    def block(g, event, attempt):  # one block per (pixel, sample, event, attempt)
        return philox4x32_10(pix[g], smp[g], U64(event), U64(attempt), k0, k1)

    def u01(w):  # u = float32(w >> 8) * 2^-24
        return (w >> U64(8)).astype(T) * T(2.0 ** -24)

    def pm1(w):  # RandF32N(-1, 1) = min + Float32() * (max - min)        math.go:30-32
        return T(-1) + u01(w) * T(2)

    vec = lambda a: np.array(list(a), F32).astype(T)  # noqa: E731
    p00, du, dv, cen = vec(cam.pixel00), vec(cam.pixel_du), vec(cam.pixel_dv), vec(cam.center)
    ddu, ddv, bg = vec(cam.defocus_disk_u), vec(cam.defocus_disk_v), vec(cam.background)

    # ---- GetRay, camera.go:265-287 -------------------------------------------------------
    allg = np.arange(N)
    b = block(allg, 0, 0)
    fi, fj = S[:, 0].astype(T), S[:, 1].astype(T)
    pc = (p00[None, :] + du[None, :] * fi[:, None]) + dv[None, :] * fj[:, None]  # :266-274
    dx, dy = T(-0.5) + u01(b[0]), T(-0.5) + u01(b[1])  # sampleUnitSquare :289-299
    pc = pc + (du[None, :] * dx[:, None] + dv[None, :] * dy[:, None])  # :275
    x, y = pm1(b[2]), pm1(b[3])  # NewVec3RandInUnitDisk, vec3.go:203-210: ALWAYS drawn (:277)
    disk_att = np.ones(N, I64)
    pend = allg[~(x * x + y * y < T(1))]
    a = 1
    while pend.size:
        bb = block(pend, 0, a)
        x[pend], y[pend] = pm1(bb[0]), pm1(bb[1])
        disk_att[pend] += 1
        pend = pend[~(x[pend] * x[pend] + y[pend] * y[pend] < T(1))]
        a += 1
    res.rng_draws += 4 + 2 * (disk_att - 1)
    O = np.broadcast_to(cen, (N, 3)).copy()
    if F32(cam.defocus_angle) > 0:  # :279-281
        O = cen[None, :] + (ddu[None, :] * x[:, None] + ddv[None, :] * y[:, None])
    D = pc - O  # :283-284

    # ---- tables in T ----------------------------------------------------------------------
    Ps, Pq = sc.n_spheres, sc.n_quads
    C, R = sc.s_center.astype(T), sc.s_radius.astype(T)
    QQ, QU, QV, QW, QN, QD = (a.astype(T) for a in (sc.q_q, sc.q_u, sc.q_v, sc.q_w, sc.q_n, sc.q_d))
    tmin, inf = T(_TMIN), T(np.inf)

    def closest(o, d):
        """World.Hit over every primitive (hittables.go:55-72) -> prim, t, root, alpha, beta, tie."""
        n = len(o)
        ts, extra = [], {}
        ox, oy, oz, dx_, dy_, dz_ = (a[:, None] for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]))
        if Ps:  # Sphere.Hit, hittables.go:96-116
            ax, ay, az = ox - C[None, :, 0], oy - C[None, :, 1], oz - C[None, :, 2]  # :97
            aa = (dx_ * dx_ + dy_ * dy_ + dz_ * dz_)  # :98
            hb = dx_ * ax + dy_ * ay + dz_ * az  # :99
            cc = (ax * ax + ay * ay + az * az) - (R * R)[None, :]  # :100
            disc = hb * hb - aa * cc  # :102
            sq = nar(np.sqrt(wide(disc)))  # :108
            r1, r2 = (-hb - sq) / aa, (-hb + sq) / aa  # :110, :112
            in1, in2 = (tmin < r1) & (r1 < inf), (tmin < r2) & (r2 < inf)  # Interval.In, bvh.go:18-20
            t = np.where(in1, r1, np.where(in2, r2, inf))
            t = np.where(disc < 0, inf, t)  # :104
            ts.append(t)
            extra["root"] = np.where(in1, 0, 1)
        if Pq:  # Quad.Hit, hittables.go:167-190
            nx, ny, nz = QN[None, :, 0], QN[None, :, 1], QN[None, :, 2]
            den = dx_ * nx + dy_ * ny + dz_ * nz  # :168
            par = np.abs(wide(den)) < 1e-8  # :170
            t = (QD[None, :] - (nx * ox + ny * oy + nz * oz)) / den  # :174
            ok = (tmin < t) & (t < inf) & ~par  # :176
            ph = np.stack([dx_ * t + ox - QQ[None, :, 0], dy_ * t + oy - QQ[None, :, 1],
                           dz_ * t + oz - QQ[None, :, 2]], axis=-1)  # :180-181 (At: ray.go:25-30)
            al = dot(np.broadcast_to(QW[None], ph.shape), cross(ph, np.broadcast_to(QV[None], ph.shape)))  # :182
            be = dot(np.broadcast_to(QW[None], ph.shape), cross(np.broadcast_to(QU[None], ph.shape), ph))  # :183
            outside = (al < 0) | (T(1) < al) | (be < 0) | (T(1) < be)  # InPlane :192-194 (a NaN is inside)
            ts.append(np.where(ok & ~outside, t, inf))
            extra["al"], extra["be"] = al, be
        if not ts:
            z = np.zeros(n, T)
            return np.full(n, -1, I64), z + inf, np.zeros(n, I64), z, z, np.zeros(n, bool)
        tall = np.concatenate(ts, axis=1)
        j = np.argmin(tall, axis=1)  # the first minimum: World.Hit's strict `<` running bound
        rows = np.arange(n)
        tb = tall[rows, j]
        hit = tb < inf
        tie = hit & ((tall == tb[:, None]).sum(axis=1) > 1)
        prim = np.where(hit, j, -1)
        root = extra["root"][rows, np.minimum(j, Ps - 1)] if Ps else np.zeros(n, I64)
        root = np.where(j < Ps, root, 0)
        if Pq:
            jq = np.clip(j - Ps, 0, Pq - 1)
            al, be = extra["al"][rows, jq], extra["be"][rows, jq]
        else:
            al = be = np.zeros(n, T)
        return prim, tb, root, al, be, tie

    def texture(tid, u, v, p, g):
        """Texture.GetTexture -> colour [m, 3], signature columns [m, 3] (parity, texel, cell)."""
        m = len(tid)
        out = np.zeros((m, 3), T)
        sg = np.full((m, 3), -1, I64)
        for t in np.unique(tid):
            k = np.nonzero(tid == t)[0]
            kind = int(sc.t_type[t])
            if kind == rtx.RTX_TEX_SOLID:  # materials.go:155-157
                out[k] = sc.t_even[t].astype(T)
            elif kind == rtx.RTX_TEX_CHECKERED:  # materials.go:127-137
                inv = T(1) / T(sc.t_scale[t])
                cell = [np.floor(wide(inv * p[k, c])).astype(I64) for c in range(3)]
                par = (cell[0] + cell[1] + cell[2]) % 2  # Go's % keeps the sign: -1 != 0 is odd too
                out[k] = np.where((par == 0)[:, None], sc.t_even[t].astype(T)[None], sc.t_odd[t].astype(T)[None])
                sg[k, 0] = par
            elif kind == rtx.RTX_TEX_IMAGE:  # materials.go:175-193
                w_, h_, off = int(sc.t_w[t]), int(sc.t_h[t]), int(sc.t_off[t])
                if h_ <= 0:  # :177-179
                    out[k] = np.array([0, 1, 1], T)
                    continue
                clamp = lambda a: np.where(a < 0, T(0), np.where(a > T(1), T(1), a))  # noqa: E731  math.go:20-28
                uu = clamp(u[k])  # :181
                vv = T(1) - clamp(v[k])  # :182
                fi_, fj_ = uu * T(w_), vv * T(h_)  # :184-185
                ok = (fi_ == fi_) & (fj_ == fj_)  # int(NaN) lies outside every image
                ii = np.where(ok, np.trunc(wide(fi_)), -1).astype(I64)  # :186 int() truncates
                jj = np.where(ok, np.trunc(wide(fj_)), -1).astype(I64)
                inside = ok & (ii >= 0) & (ii < w_) & (jj >= 0) & (jj < h_)
                idx = np.where(inside, jj * w_ + ii, w_ * h_)  # rtx.h: the border texel after the raster
                w0, w1 = sc.texels[off + 2 * idx].astype(I64), sc.texels[off + 2 * idx + 1].astype(I64)
                rgb = np.stack([w0 & 0xFFFF, w0 >> 16, w1 & 0xFFFF], axis=-1)  # rtx.h: r | g << 16, b | a << 16
                out[k] = rgb.astype(T) * T(_COL_SCALE)  # :188-191
                sg[k, 1] = idx
                res.texel_fetches[g[k]] += 1
            elif kind == rtx.RTX_TEX_NOISE:  # materials.go:285-288
                off = int(sc.t_off[t])
                tab = sc.texels[off: off + 1536]
                grad = tab[:768].view(F32).reshape(256, 3).astype(T)
                perm = [tab[768 + 256 * c: 1024 + 256 * c].astype(I64) for c in range(3)]
                cells = np.zeros(len(k), U64)

                def noise(q):  # Perlin.Noise, materials.go:223-249
                    fl = [nar(np.floor(wide(q[:, c]))) for c in range(3)]  # :224-226
                    tx, ty, tz = q[:, 0] - fl[0], q[:, 1] - fl[1], q[:, 2] - fl[2]  # :228-230
                    r0 = [fl[c].astype(I64) & 255 for c in range(3)]  # :232-237
                    r1 = [(r0[c] + 1) & 255 for c in range(3)]
                    nonlocal cells
                    key = (r0[0] << 16) | (r0[1] << 8) | r0[2]
                    cells = cells * U64(1000003) + key.astype(U64)
                    one = T(1)

                    def corner(ix, iy, iz, wx, wy, wz):  # :239-246
                        gv = grad[perm[0][ix] ^ perm[1][iy] ^ perm[2][iz]]
                        return gv[:, 0] * wx + gv[:, 1] * wy + gv[:, 2] * wz

                    c000 = corner(r0[0], r0[1], r0[2], tx, ty, tz)
                    c001 = corner(r0[0], r0[1], r1[2], tx, ty, tz - one)
                    c010 = corner(r0[0], r1[1], r0[2], tx, ty - one, tz)
                    c011 = corner(r0[0], r1[1], r1[2], tx, ty - one, tz - one)
                    c100 = corner(r1[0], r0[1], r0[2], tx - one, ty, tz)
                    c101 = corner(r1[0], r0[1], r1[2], tx - one, ty, tz - one)
                    c110 = corner(r1[0], r1[1], r0[2], tx - one, ty - one, tz)
                    c111 = corner(r1[0], r1[1], r1[2], tx - one, ty - one, tz - one)
                    sm = lambda s: s * s * (T(3) - T(2) * s)  # noqa: E731  smoothstep :218-220
                    lerp = lambda s, a_, b_: a_ * (one - s) + b_ * s  # noqa: E731  math.go:58-60
                    sx, sy, sz = sm(tx), sm(ty), sm(tz)
                    e = lerp(sy, lerp(sx, c000, c100), lerp(sx, c010, c110))  # math.go:78-92
                    f = lerp(sy, lerp(sx, c001, c101), lerp(sx, c011, c111))
                    return lerp(sz, e, f)

                pt = p[k] * T(sc.t_scale[t])  # :286
                q, total, weight = pt.copy(), np.zeros(len(k), T), T(1)
                for _ in range(7):  # Turb(point, 7), materials.go:251-262
                    total = total + weight * noise(q)
                    weight = weight * T(0.5)
                    q = q * T(2)
                turb = nar(np.abs(wide(total)))
                val = T(0.5) * (T(1) + nar(np.sin(wide(pt[:, 2] + T(10) * turb))))  # :287
                out[k] = val[:, None]
                sg[k, 2] = cells.view(I64)
            else:
                raise ValueError(f"texture kind {kind}")
        return out, sg

    def unit_sphere(g, event):
        """NewVec3UnitRandOnUnitSphere32 (vec3.go:182-190): attempt a = words 0-2 of block (event, a)."""
        out = np.zeros((len(g), 3), T)
        att = np.zeros(len(g), I64)
        pend = np.arange(len(g))
        a_ = 0
        while pend.size:
            bb = block(g[pend], event, a_)
            v = np.stack([pm1(bb[0]), pm1(bb[1]), pm1(bb[2])], axis=-1)
            att[pend] += 1
            ok = dot(v, v) < T(1)
            out[pend[ok]] = unit(v[ok])
            pend = pend[~ok]
            a_ += 1
        res.rng_draws[g] += 3 * att
        return out, att

    # ---- GetColor, ray.go:32-54 ------------------------------------------------------------
    alive = np.ones(N, bool)
    E_list, A_list, sig_list = [], [], []
    for s in range(int(cam.max_depth)):  # :33: a ray with no depth left is black
        g = np.nonzero(alive)[0]
        if g.size == 0:
            break
        o, d = O[g], D[g]
        res.segments[g] += 1
        prim, t, root, al, be, tie = closest(o, d)
        res.tie[g] |= tie
        E, A = np.zeros((N, 3), T), np.zeros((N, 3), T)
        sig = np.full((N, SIG_COLS), -1, I64)
        sig[:, 0] = -2
        sig[g, 0] = prim
        hit = prim >= 0
        E[g[~hit]] = bg  # :53
        alive[g[~hit]] = False
        h = np.nonzero(hit)[0]
        gh = g[h]
        res.hits[gh] += 1
        oh, dh, th, ph = o[h], d[h], t[h], prim[h]
        point = dh * th[:, None] + oh  # ray.go:25-30
        m = len(h)
        normal, uu, vv, mat = np.zeros((m, 3), T), np.zeros(m, T), np.zeros(m, T), np.zeros(m, I64)
        isq = ph >= Ps
        if (~isq).any():  # hittables.go:118-126
            k = np.nonzero(~isq)[0]
            i = ph[k]
            nrm = unit((point[k] - C[i]) * R[i][:, None])  # :119-120
            theta = nar(np.arccos(-wide(nrm[:, 1])))  # :122
            phi = nar(np.arctan2(-wide(nrm[:, 2]), wide(nrm[:, 0])) + np.pi)  # :123
            uu[k] = (phi + T(_UV_SHIFT)) / T(_UV_TWO_PI)  # :125
            vv[k] = theta / T(_PI32)  # :126
            normal[k], mat[k] = nrm, sc.s_mat[i]
        if isq.any():  # hittables.go:189
            k = np.nonzero(isq)[0]
            i = ph[k] - Ps
            normal[k], uu[k], vv[k], mat[k] = QN[i], al[h][k], be[h][k], sc.q_mat[i]
        front = dot(dh, normal) < 0  # NewHitInfo, hittables.go:22-26
        normal = np.where(front[:, None], normal, normal * T(-1))
        sig[gh, 1], sig[gh, 2] = root[h], front
        mtype = sc.m_type[mat]
        newD = np.zeros((m, 3), T)
        cont = np.zeros(m, bool)

        k = np.nonzero(mtype == rtx.RTX_MAT_DIFFUSE_LIGHT)[0]  # materials.go:301-313: emits, never scatters
        if k.size:
            c, sg = texture(sc.m_tex[mat[k]], uu[k], vv[k], point[k], gh[k])
            E[gh[k]] = c
            sig[gh[k], 3] = BR_EMIT
            sig[gh[k], 5:8] = sg

        k = np.nonzero(mtype == rtx.RTX_MAT_LAMBERTIAN)[0]  # materials.go:33-42
        if k.size:
            rs, att = unit_sphere(gh[k], s + 1)
            dr = normal[k] + rs  # :34
            nz = (np.abs(dr) < T(_NEAR_ZERO)).all(axis=1)  # vec3.go:170-172
            dr = np.where(nz[:, None], normal[k], dr)  # :35-37
            c, sg = texture(sc.m_tex[mat[k]], uu[k], vv[k], point[k], gh[k])  # :40
            A[gh[k]] = c
            newD[k], cont[k] = dr, True
            sig[gh[k], 3], sig[gh[k], 4], sig[gh[k], 8] = BR_LAMBERT, att, nz
            sig[gh[k], 5:8] = sg

        k = np.nonzero(mtype == rtx.RTX_MAT_METAL)[0]  # materials.go:60-75
        if k.size:
            ud = unit(dh[k])  # :61
            n_ = normal[k]
            refl = ud - n_ * (T(2) * dot(ud, n_))[:, None]  # vec3.go:212-214
            rs, att = unit_sphere(gh[k], s + 1)  # :64
            fz = rs * sc.m_fuzz[mat[k]].astype(T)[:, None]  # :65
            scd = refl + fz  # :67
            ok = dot(scd, n_) > 0  # :68
            A[gh[k[ok]]] = sc.m_albedo[mat[k[ok]]].astype(T)
            newD[k], cont[k] = scd, ok
            sig[gh[k], 3], sig[gh[k], 4] = np.where(ok, BR_METAL, BR_ABSORBED), att

        k = np.nonzero(mtype == rtx.RTX_MAT_DIELECTRIC)[0]  # materials.go:91-113
        if k.size:
            ior = sc.m_ior[mat[k]].astype(T)
            eta = np.where(front[k], T(1) / ior, ior)  # :92-95
            ud = unit(dh[k])  # :97
            n_ = normal[k]
            cos_t = nar(np.minimum(wide(dot(ud * T(-1), n_)), 1.0))  # :99
            sin_t = nar(np.sqrt(1.0 - wide(cos_t * cos_t)))  # :100
            tir = sin_t * eta > T(1)  # :101
            r0 = (T(1) - eta) / (T(1) + eta)  # reflectance, :115-119
            r0 = r0 * r0
            refl_p = r0 + (T(1) - r0) * nar(np.power(1.0 - wide(cos_t), 5.0))
            can = np.nonzero(~tir)[0]  # the `||` of :103 draws only when refraction is possible
            uni = np.zeros(len(k), T)
            if can.size:
                uni[can] = u01(block(gh[k[can]], s + 1, 0)[0])
                res.rng_draws[gh[k[can]]] += 1
            schlick = ~tir & (refl_p > uni)
            mirror = ud - n_ * (T(2) * dot(ud, n_))[:, None]  # :104
            cos2 = dot(ud * T(-1), n_)  # refract, vec3.go:216-221
            perp = (ud + n_ * cos2[:, None]) * eta[:, None]
            parl = n_ * (T(-1) * nar(np.sqrt(np.abs(wide(T(1) - dot(perp, perp))))))[:, None]
            newD[k] = np.where((tir | schlick)[:, None], mirror, parl + perp)
            res.abs_used[gh[k]] |= ~(tir | schlick) & (T(1) - dot(perp, perp) < 0)
            cont[k] = True
            A[gh[k]] = T(1)  # :111
            sig[gh[k], 3] = np.where(tir, BR_REFLECT_TIR, np.where(schlick, BR_REFLECT_SCHLICK, BR_REFRACT))

        O[gh[cont]], D[gh[cont]] = point[cont], newD[cont]
        alive[gh[~cont]] = False
        E_list.append(E)
        A_list.append(A)
        sig_list.append(sig)
        if dump:
            res.dump.append({"g": gh, "origin": oh, "dir": dh, "prim": ph, "t": th, "root": root[h], "point": point,
                             "normal": normal, "u": uu, "v": vv, "front": front, "branch": sig[gh, 3],
                             "emit": E[gh], "att": A[gh], "next_dir": newD, "scattered": cont})

    colour = np.zeros((N, 3), T)  # ray.go:48-50: emission + attenuation * GetColor(depth - 1), inside out
    for E, A in zip(reversed(E_list), reversed(A_list)):
        colour = E + A * colour
    res.colour = colour
    res.sig = np.concatenate([disk_att[:, None]] + sig_list, axis=1) if sig_list else disk_att[:, None]


# ---- which samples a float32 implementation is held to --------------------------------------
class Case:
    """Both runs of one window (x0, y0, w, h) at `spp` samples per pixel and what follows from them
    alone.  Per pixel, row-major: `kept` (every sample of the pixel decides alike in float32 and
    float64 and meets no tie), `expected` (the float64 mean of its samples, camera.go:254-263),
    `left_out` (the share of SAMPLES not kept), `spread` (max |float32 pixel - float64 pixel| over
    kept pixels, the float32 pixel summed and scaled as Go does) and
    `tol` = max(4 * spread, 4 float32 ulps of the largest kept colour)."""

    def __init__(self, desc, cam, seed, window, spp: int = 1):
        x0, y0, w, h = window
        self.window, self.spp = tuple(window), spp
        self.samples = grid(x0, y0, w, h, spp)
        sc = Scene(desc)
        self.r32 = trace(sc, cam, seed, self.samples, F32)
        self.r64 = trace(sc, cam, seed, self.samples, F64)
        a, b = self.r32.sig, self.r64.sig
        width = max(a.shape[1], b.shape[1])
        blank = np.array([-2] + [-1] * (SIG_COLS - 1), I64)
        pad = lambda s: np.concatenate(  # noqa: E731
            [s, np.tile(blank, (len(s), (width - s.shape[1]) // SIG_COLS))], axis=1)
        self.sample_kept = (pad(a) == pad(b)).all(axis=1) & ~self.r32.tie & ~self.r64.tie
        self.left_out = float(1.0 - self.sample_kept.mean())
        self.kept = self.sample_kept.reshape(-1, spp).all(axis=1)
        c64 = self.r64.colour.reshape(-1, spp, 3)
        c32 = self.r32.colour.reshape(-1, spp, 3)
        self.expected = c64.sum(axis=1) / spp if spp > 1 else c64[:, 0]
        acc = np.zeros_like(c32[:, 0])
        for k in range(spp):  # sample.Add(s) then Scale(1.0 / float32(spp)), camera.go:259-261
            acc = acc + c32[:, k]
        self.pixel32 = acc * (F32(1.0) / F32(spp))
        k = self.kept
        self.spread = float(np.abs(self.pixel32[k].astype(F64) - self.expected[k]).max()) if k.any() else 0.0
        top = float(np.abs(self.expected[k]).max()) if k.any() else 0.0
        self.tol = max(4.0 * self.spread, 4.0 * float(np.spacing(F32(top))))

    def counters(self) -> dict:
        return self.r64.counters()

    def worst(self, image):
        """max |image - expected| over kept pixels of a [h, w, 3] (or [h * w, 3]) render of the window."""
        img = np.asarray(image, F64).reshape(-1, 3)
        assert img.shape == self.expected.shape, (img.shape, self.expected.shape)
        k = self.kept
        return float(np.abs(img[k] - self.expected[k]).max()) if k.any() else 0.0


def grid(x0, y0, w, h, spp=1):
    """(x, y, k) of every sample of a window, row-major, samples innermost."""
    ys, xs, ks = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ks.ravel()], axis=1)
