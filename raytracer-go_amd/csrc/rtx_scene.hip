// rtx_scene.hip — the host-only half of the C-ABI (include/rtx.h): no HIP, and like rtx_topology.hip and
// rtx_collapse.hip it also compiles as plain C++ (tests/test_pack_layout.py).
//
// Validates the flattened Hittable tree the caller hands over (what a cgo Render would pass), converts it into the
// threaded pre-order entries (rtx_layout.h), plans the walk of a camera, and computes the storage order of a walk on
// the device (pack_layout).  Errors are returned as codes with a thread-local message; nothing throws across the ABI.
#define RTX_HOST_ONLY
#include "rtx_internal.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "rtx_collapse.h"

namespace rtxh {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// Integer knob from the environment (read per call), clamped to [lo, hi].
uint32_t env_knob(const char* name, long dflt, long lo, long hi) {
    const char* e = std::getenv(name);
    const long x = e ? std::strtol(e, nullptr, 10) : dflt;
    return (uint32_t)(x < lo ? lo : (x > hi ? hi : x));
}

namespace {

int check_ref(const rtx_scene_desc* d, int32_t ref) {
    if (ref >= 0) {
        if ((uint32_t)ref >= d->n_nodes) return fail(RTX_ERR_INVALID_ARG, "node ref %d out of range (%u nodes)", ref, d->n_nodes);
        return RTX_OK;
    }
    const uint32_t p = (uint32_t)(~ref);
    const uint32_t type = p >> 28, idx = p & 0x0FFFFFFFu;
    if (type == RTX_PRIM_SPHERE) {
        if (idx >= d->n_spheres) return fail(RTX_ERR_INVALID_ARG, "sphere ref %u out of range (%u spheres)", idx, d->n_spheres);
        return RTX_OK;
    }
    if (type == RTX_PRIM_QUAD) {
        if (idx >= d->n_quads) return fail(RTX_ERR_INVALID_ARG, "quad ref %u out of range (%u quads)", idx, d->n_quads);
        return RTX_OK;
    }
    if (type == RTX_PRIM_LIST) {  // a nested World (ABI 5)
        if (idx >= d->n_lists || !d->lists) return fail(RTX_ERR_INVALID_ARG, "list ref %u out of range (%u lists)", idx, d->n_lists);
        const rtx_list& l = d->lists[idx];
        // (an empty World is a well-defined miss, hittables.go:55-72: it emits no entries)
        if (l.count && (!d->list_refs || (uint64_t)l.first + l.count > d->n_list_refs))
            return fail(RTX_ERR_INVALID_ARG, "list %u items out of range (%u list refs)", idx, d->n_list_refs);
        return RTX_OK;
    }
    return fail(RTX_ERR_INVALID_ARG, "unknown primitive type %u", type);
}

// Graph vertex of a ref for check_acyclic: nodes 0..n_nodes-1, lists after them; -1 for a leaf.
int64_t vertex_of(const rtx_scene_desc* d, int32_t ref) {
    if (ref >= 0) return ref;
    const uint32_t p = (uint32_t)(~ref);
    return (p >> 28) == RTX_PRIM_LIST ? (int64_t)d->n_nodes + (p & 0x0FFFFFFFu) : -1;
}

}  // namespace

// Reject a node / list graph with a cycle (a Go BVH cannot have one, a hand-built table can).
int check_acyclic(const rtx_scene_desc* d) {
    std::vector<uint8_t> state((size_t)d->n_nodes + d->n_lists, 0);  // 0 new, 1 on path, 2 done
    struct F { int64_t v; uint32_t child; };
    auto n_children = [&](int64_t v) -> uint32_t {
        return v < (int64_t)d->n_nodes ? 2u : d->lists[v - d->n_nodes].count;
    };
    auto child = [&](int64_t v, uint32_t k) -> int32_t {
        if (v < (int64_t)d->n_nodes) return k == 0 ? d->nodes[v].left : d->nodes[v].right;
        const rtx_list& l = d->lists[v - d->n_nodes];
        return d->list_refs[l.first + k];
    };
    for (uint32_t r = 0; r < d->n_roots; ++r) {
        if (int rc = check_ref(d, d->roots[r])) return rc;
        const int64_t v0 = vertex_of(d, d->roots[r]);
        if (v0 < 0 || state[v0] == 2) continue;
        std::vector<F> st{{v0, 0}};
        state[v0] = 1;
        while (!st.empty()) {
            F& f = st.back();
            if (f.child == n_children(f.v)) { state[f.v] = 2; st.pop_back(); continue; }
            const int32_t ref = child(f.v, f.child++);
            if (int rc = check_ref(d, ref)) return rc;
            const int64_t v = vertex_of(d, ref);
            if (v < 0 || state[v] == 2) continue;
            if (state[v] == 1) return fail(RTX_ERR_INVALID_ARG, "BVH node / list graph has a cycle through ref %d", ref);
            state[v] = 1;
            st.push_back({v, 0});
        }
    }
    return RTX_OK;
}

// Emit the reference's visit order (bvh.go:220-249) as threaded pre-order entries.
int emit(const rtx_scene_desc* d, int32_t root, std::vector<rtx_entry>& out) {
    struct Frame {
        int32_t ref;
        int64_t node_entry;  // >= 0: close this node's escape when popped
    };
    std::vector<Frame> stack;
    stack.push_back({root, -1});
    const size_t limit = (size_t)1 << 26;  // 2 GiB of entries
    while (!stack.empty()) {
        Frame f = stack.back();
        stack.pop_back();
        if (f.node_entry >= 0) {  // subtree finished
            const int32_t esc = (int32_t)out.size();
            std::memcpy(&out[(size_t)f.node_entry].a[3], &esc, 4);
            continue;
        }
        if (int rc = check_ref(d, f.ref)) return rc;
        if (out.size() >= limit) return fail(RTX_ERR_INVALID_ARG, "BVH expands to more than %zu entries", limit);
        rtx_entry e;
        std::memset(&e, 0, sizeof(e));
        if (f.ref < 0 && (((uint32_t)(~f.ref)) >> 28) == RTX_PRIM_LIST) {
            // a nested World (hittables.go:55-72): its items one after another, each against the
            // running bound — the walk simply continues into the next item's entries
            const rtx_list& l = d->lists[((uint32_t)(~f.ref)) & 0x0FFFFFFFu];
            for (uint32_t k = l.count; k-- > 0;) stack.push_back({d->list_refs[l.first + k], -1});
        } else if (f.ref >= 0) {
            const rtx_bvh_node& n = d->nodes[f.ref];
            // NewAabb orders every axis (bvh.go:36-50); the walk's med3 slab form (box_hit) relies on it: a box with
            // bmin > bmax misses in the reference and would hit there.  (`!(<=)` rejects a NaN bound too.)
            for (int k = 0; k < 3; ++k)
                if (!(n.bmin[k] <= n.bmax[k]))
                    return fail(RTX_ERR_INVALID_ARG, "node %d: box axis %d is not ordered (bmin %g, bmax %g)", f.ref, k,
                                (double)n.bmin[k], (double)n.bmax[k]);
            e.a[0] = n.bmin[0]; e.a[1] = n.bmin[1]; e.a[2] = n.bmin[2];
            e.b[0] = n.bmax[0]; e.b[1] = n.bmax[1]; e.b[2] = n.bmax[2];
            const int32_t tag = RTX_E_NODE;
            std::memcpy(&e.b[3], &tag, 4);
            const int64_t me = (int64_t)out.size();
            out.push_back(e);
            // visit order: left, then right (skipped when left == right, see rtx_layout.h)
            stack.push_back({0, me});
            if (n.right != n.left) stack.push_back({n.right, -1});
            stack.push_back({n.left, -1});
        } else if ((((uint32_t)(~f.ref)) >> 28) == RTX_PRIM_QUAD) {  // (normal, D | quad, tag)
            const uint32_t idx = ((uint32_t)(~f.ref)) & 0x0FFFFFFFu;
            const rtx_quad& q = d->quads[idx];
            e.a[0] = q.normal[0]; e.a[1] = q.normal[1]; e.a[2] = q.normal[2]; e.a[3] = q.d;
            const int32_t qi = (int32_t)idx, tag = RTX_E_QUAD;
            std::memcpy(&e.b[0], &qi, 4);
            std::memcpy(&e.b[3], &tag, 4);
            out.push_back(e);
        } else {
            const uint32_t idx = ((uint32_t)(~f.ref)) & 0x0FFFFFFFu;
            const rtx_sphere& s = d->spheres[idx];
            e.a[0] = s.center[0]; e.a[1] = s.center[1]; e.a[2] = s.center[2]; e.a[3] = s.radius;
            e.b[0] = s.radius * s.radius;  // hittables.go:100
            const int32_t si = (int32_t)idx, mi = (int32_t)s.material;
            std::memcpy(&e.b[1], &si, 4);
            std::memcpy(&e.b[3], &mi, 4);
            out.push_back(e);
        }
    }
    return RTX_OK;
}

// Checks of the tables every scene shares (materials, textures, texels, primitives).
int validate_tables(const rtx_scene_desc* d) {
    if (d->n_spheres && !d->spheres) return fail(RTX_ERR_INVALID_ARG, "spheres is NULL");
    if (d->n_materials && !d->materials) return fail(RTX_ERR_INVALID_ARG, "materials is NULL");
    if (d->n_textures && !d->textures) return fail(RTX_ERR_INVALID_ARG, "textures is NULL");
    if (d->n_texels && !d->texels) return fail(RTX_ERR_INVALID_ARG, "texels is NULL");
    if (d->n_quads && !d->quads) return fail(RTX_ERR_INVALID_ARG, "quads is NULL");
    if (d->n_quads > (1u << 26)) return fail(RTX_ERR_INVALID_ARG, "too many quads");
    for (uint32_t i = 0; i < d->n_quads; ++i)
        if (d->quads[i].material >= d->n_materials)
            return fail(RTX_ERR_INVALID_ARG, "quad %u material %u out of range", i, d->quads[i].material);
    for (uint32_t i = 0; i < d->n_spheres; ++i)
        if (d->spheres[i].material >= d->n_materials)
            return fail(RTX_ERR_INVALID_ARG, "sphere %u material %u out of range", i, d->spheres[i].material);
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const rtx_material& m = d->materials[i];
        if (m.type > RTX_MAT_DIFFUSE_LIGHT) return fail(RTX_ERR_INVALID_ARG, "material %u: unknown type %u", i, m.type);
        if ((m.type == RTX_MAT_LAMBERTIAN || m.type == RTX_MAT_DIFFUSE_LIGHT) && m.texture >= d->n_textures)
            return fail(RTX_ERR_INVALID_ARG, "material %u texture %u out of range", i, m.texture);
    }
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const rtx_texture& t = d->textures[i];
        if (t.type == RTX_TEX_NOISE) {
            if ((uint64_t)t.texel_offset + RTX_NOISE_TEXELS > d->n_texels)
                return fail(RTX_ERR_INVALID_ARG, "texture %u: Perlin tables out of range", i);
            for (uint32_t k = 768; k < RTX_NOISE_TEXELS; ++k)
                if (d->texels[t.texel_offset + k] > 255)
                    return fail(RTX_ERR_INVALID_ARG, "texture %u: Perlin permutation entry out of range", i);
        }
        if (t.type > RTX_TEX_NOISE) return fail(RTX_ERR_INVALID_ARG, "texture %u: unknown type %u", i, t.type);
        if (t.type == RTX_TEX_IMAGE && (int32_t)t.height > 0) {  // RGBA16 raster + border texel (rtx.h)
            if (t.texel_offset & 1u) return fail(RTX_ERR_INVALID_ARG, "texture %u: texel_offset must be even", i);
            if ((uint64_t)t.texel_offset + RTX_IMAGE_TEXEL_WORDS * ((uint64_t)t.width * t.height + 1) > d->n_texels)
                return fail(RTX_ERR_INVALID_ARG, "texture %u texels out of range", i);
        }
    }
    return RTX_OK;
}

// The list of a World for rtx_scene_create_world: NewBVH's input holds spheres and quads only (a node, a nested
// World, an unknown type or an index outside its table is refused; a primitive may be named twice or not at all).
int check_world_items(const rtx_scene_desc* d, const int32_t* items, uint32_t n_items) {
    for (uint32_t i = 0; i < n_items; ++i) {
        const int32_t ref = items[i];
        if (ref >= 0) return fail(RTX_ERR_INVALID_ARG, "item %u: a node ref (%d) is no item of a World", i, ref);
        const uint32_t type = ((uint32_t)(~ref)) >> 28;
        if (type == RTX_PRIM_LIST) return fail(RTX_ERR_INVALID_ARG, "item %u: a nested World is not built on the GPU", i);
        if (type != RTX_PRIM_SPHERE && type != RTX_PRIM_QUAD)
            return fail(RTX_ERR_INVALID_ARG, "item %u: unknown primitive type %u", i, type);
        if (check_ref(d, ref)) {
            const std::string why = g_last_error;
            return fail(RTX_ERR_INVALID_ARG, "item %u: %s", i, why.c_str());
        }
    }
    return RTX_OK;
}

// The quad table of a scene description (rtx_layout.h): (Q, material), (u, 0), (v, 0), (w, 0).
void quad_table(const rtx_scene_desc* d, std::vector<float>& tab) {
    tab.assign((size_t)d->n_quads * 16, 0.0f);
    for (uint32_t i = 0; i < d->n_quads; ++i) {
        const rtx_quad& q = d->quads[i];
        float* o = &tab[(size_t)i * 16];
        std::memcpy(o, q.q, 12);
        std::memcpy(o + 3, &q.material, 4);
        std::memcpy(o + 4, q.u, 12);
        std::memcpy(o + 8, q.v, 12);
        std::memcpy(o + 12, q.w, 12);
    }
}

// The emitter table (rtx.h, "direct light sampling"): the spheres, then the quads, that the walk's
// entries name and whose material is a DiffuseLight, each once, in table order.  Every float operation is float32 and
// rounded on its own (the unit is built without contraction): area = (4 * PiF32) * (r * r), or Len(Cross(u, v)).
int build_lights(const std::vector<rtx_entry>& base, const std::vector<float>& quadtab,
                 const std::vector<rtx_material>& materials, std::vector<rtx_light>& lights, std::vector<float>* tab,
                 std::vector<rtx_prim_light>* prims, uint32_t n_spheres) {
    struct Emitter {
        uint32_t index, material;
        float a[4], u[3], v[3], n[3];  // a: (centre, radius) or (Q, 0)
    };
    std::vector<Emitter> sph, quad;
    for (const rtx_entry& e : base) {
        int32_t tag;
        std::memcpy(&tag, &e.b[3], 4);
        if (tag == RTX_E_NODE) continue;
        Emitter m{};
        if (tag == RTX_E_QUAD) {
            std::memcpy(&m.index, &e.b[0], 4);
            const float* q = &quadtab[(size_t)m.index * 16];
            std::memcpy(&m.material, q + 3, 4);
            std::memcpy(m.a, q, 12);
            std::memcpy(m.u, q + 4, 12);
            std::memcpy(m.v, q + 8, 12);
            std::memcpy(m.n, e.a, 12);
        } else {
            std::memcpy(&m.index, &e.b[1], 4);
            m.material = (uint32_t)tag;
            std::memcpy(m.a, e.a, 16);
        }
        if (m.material >= materials.size() || materials[m.material].type != RTX_MAT_DIFFUSE_LIGHT) continue;
        (tag == RTX_E_QUAD ? quad : sph).push_back(m);
    }
    const auto by_index = [](const Emitter& x, const Emitter& y) { return x.index < y.index; };
    const auto same = [](const Emitter& x, const Emitter& y) { return x.index == y.index; };
    for (std::vector<Emitter>* v : {&sph, &quad}) {
        std::stable_sort(v->begin(), v->end(), by_index);
        v->erase(std::unique(v->begin(), v->end(), same), v->end());
    }
    lights.clear();
    if (tab) tab->clear();
    // the per-primitive lookup (rtx.h, "multiple importance sampling"): the caller's spheres, then its quads
    if (prims) prims->assign((size_t)n_spheres + quadtab.size() / 16, rtx_prim_light{0.0f, RTX_LIGHT_NONE});
    const auto put = [&](const Emitter& m, uint32_t kind, float area) {
        if (!(std::isfinite(area) && area > 0.0f)) return;
        const size_t slot = kind == RTX_PRIM_QUAD ? (size_t)n_spheres + m.index : (size_t)m.index;
        if (prims && (kind == RTX_PRIM_QUAD || m.index < n_spheres)) (*prims)[slot] = rtx_prim_light{area, (uint32_t)lights.size()};
        lights.push_back(rtx_light{(kind << 28) | m.index, area});
        if (!tab) return;
        float rec[16] = {m.a[0], m.a[1], m.a[2], m.a[3], m.u[0], m.u[1], m.u[2], area,
                         m.v[0], m.v[1], m.v[2], 0.0f,   m.n[0], m.n[1], m.n[2], 0.0f};
        std::memcpy(&rec[11], &kind, 4);
        std::memcpy(&rec[15], &m.material, 4);
        tab->insert(tab->end(), rec, rec + 16);
    };
    const float pi32 = 3.14159274101257324f;  // PiF32, math.go:48
    for (const Emitter& m : sph) {
        const float r = m.a[3];
        if (!(r > 0.0f)) continue;
        put(m, RTX_PRIM_SPHERE, (4.0f * pi32) * (r * r));
    }
    for (const Emitter& m : quad) {
        const float cx = m.u[1] * m.v[2] - m.u[2] * m.v[1], cy = m.u[2] * m.v[0] - m.u[0] * m.v[2],
                    cz = m.u[0] * m.v[1] - m.u[1] * m.v[0];  // vec3.go:129-135
        const float lsq = cx * cx + cy * cy + cz * cz;       // vec3.go:115-117
        put(m, RTX_PRIM_QUAD, (float)std::sqrt((double)lsq));  // vec3.go:119-121
    }
    if (lights.size() > (1u << 24)) {
        const size_t L = lights.size();
        lights.clear();
        if (tab) tab->clear();
        if (prims) prims->clear();
        return fail(RTX_ERR_INVALID_ARG, "%zu emitters: more than 2^24 (the light index is drawn from one float32)", L);
    }
    return RTX_OK;
}

int scene_lights(rtx_scene* s) {
    if (s->lights_built) return RTX_OK;
    if (int rc = build_lights(s->base, s->quadtab, s->materials, s->lights, &s->lighttab, &s->primlights,
                              (uint32_t)s->sphere_rank.size()))
        return rc;
    s->lights_built = true;
    return RTX_OK;
}

namespace {

// The walk's tree (rtx_topology.h): 0 = the caller's, 1 = guarded, 2 = unguarded.  Default:
// guarded when the spheres pass rtxd::precise_enough, else the caller's.  RTX_SCENE_REFERENCE_BVH
// or the environment variable RTX_BVH=reference (read per scene) keep the caller's;
// RTX_BVH=guarded / sah force the guarded / unguarded tree (A/B).
int topology_mode(uint32_t flags, const std::vector<rtx_entry>& ref) {
    if (flags & RTX_SCENE_REFERENCE_BVH) return 0;
    const char* e = std::getenv("RTX_BVH");
    if (e && std::strcmp(e, "reference") == 0) return 0;
    if (e && std::strcmp(e, "sah") == 0) return 2;
    if (e && std::strcmp(e, "guarded") == 0) return 1;
    return rtxd::precise_enough(ref) ? 1 : 0;
}

// Quads in a near tree: the walk over another tree meets two quads that report the same t (two
// coplanar quads that overlap: the Cornell box's box bottoms on its floor) in another order than the reference, and
// the quad test has no tie rule.  Such a pair is admitted only when either answer gives the same path and colour:
// the same material (not an image texture, which reads the hit's u, v) and the same normal; else no near tree.
bool quad_ties_harmless(const rtx_scene_desc* d, const std::vector<float>& quadtab) {
    const uint32_t n = d->n_quads;
    if (n > 4096) return false;  // (pairs checked one by one)
    std::vector<std::array<float, 6>> box(n);
    for (uint32_t i = 0; i < n; ++i) rtxd::quad_own_box(&quadtab[16 * (size_t)i], &box[i][0], &box[i][3]);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i + 1; j < n; ++j) {
            const rtx_quad &a = d->quads[i], &b = d->quads[j];
            bool same = true, opp = true;
            for (int k = 0; k < 3; ++k) {
                same &= a.normal[k] == b.normal[k];
                opp &= a.normal[k] == -b.normal[k];
            }
            const bool coplanar = (same && a.d == b.d) || (opp && a.d == -b.d);
            bool overlap = coplanar;
            for (int k = 0; k < 3 && overlap; ++k) overlap = box[i][k] <= box[j][3 + k] && box[j][k] <= box[i][3 + k];
            if (!overlap) continue;
            if (!same || a.material != b.material) return false;
            const rtx_material& m = d->materials[a.material];
            if ((m.type == RTX_MAT_LAMBERTIAN || m.type == RTX_MAT_DIFFUSE_LIGHT) &&
                d->textures[m.texture].type == RTX_TEX_IMAGE)
                return false;
        }
    return true;
}

// The tiered walk: a scene of spheres under one tree also gets a near tree (spheres
// behind their own boxes grown for origins in the near region), unless RTX_SCENE_NO_TIER,
// RTX_SCENE_REFERENCE_BVH or RTX_TIER=0, or a node box does not contain the boxes of the spheres
// below it (the hit check's argument needs that; NewBVH's always do).  Its far tree is the walk's
// other tree: the guarded rebuild, or the caller's.  The region is the core box grown by
// RTX_NEAR_GROW percent of its largest extent: 150 for scenes that pass precise_enough (randSpheres,
// C2 at 100 spp, round 4's margins and FMA walk: 50 / 100 / 150 / 200 / 300 % -> 21.73 / 21.02 / 20.65 /
// 20.73 / 21.05 ms; round 3: 10 / 25 / 40 / 60 / 100 % -> 23.73 / 23.43 / 23.21 / 22.89 / 22.67 ms),
// 1 for the others (config 4's 316-unit slab, whose far corners set every margin anyway: 0 (untiered) /
// 1 / 2 / 5 % -> 100.9 / 76.6 / 77.2 / 78.9 ms).
bool tier_topology(uint32_t flags, const std::vector<rtx_entry>& base, const rtx_scene_desc* d, rtxd::Topology& near) {
    if (flags & (RTX_SCENE_NO_TIER | RTX_SCENE_REFERENCE_BVH)) return false;
    const char* e = std::getenv("RTX_TIER");
    if (e && std::strcmp(e, "0") == 0) return false;
    // quads join a near tree with RTX_TIER_QUADS=1 when their coplanar ties are harmless — off by
    // default: a ray through the edge two quads share ties them too, and the quad test has no rank rule yet (the GPU
    // parity test found 11 of 4.7 M Cornell segments that then differ from the caller's tree)
    std::vector<float> quadtab;
    quad_table(d, quadtab);
    const bool quads = d->n_quads > 0;
    if (quads && (env_knob("RTX_TIER_QUADS", 0, 0, 1) == 0 || !quad_ties_harmless(d, quadtab))) return false;
    if (!rtxd::own_boxes_nested(base, quads ? &quadtab : nullptr)) return false;
    float box[6];
    // a scene with quads grows its region by 150 % too: it must hold the camera (the Cornell box's is 800 units
    // in front of its 555-unit room)
    const double grow = env_knob("RTX_NEAR_GROW", rtxd::precise_enough(base) || quads ? 150 : 1, 0, 1000) / 100.0;
    return rtxd::near_region(base, box, grow, quads ? &quadtab : nullptr) &&
           rtxd::build_topology(base, false, near, box, quads ? &quadtab : nullptr);
}

// A tiered scene walks in two tiers for a camera whose rays all start in the near region (the
// defocus disk's box, with room for rounding, inside it): else the guarded walk alone.
bool camera_in_box(const float* b, const rtx_camera* cam) {
    for (int k = 0; k < 3; ++k) {
        const double c = cam->center[k];
        const double rad = cam->defocus_angle > 0.0f
                               ? std::fabs((double)cam->defocus_disk_u[k]) + std::fabs((double)cam->defocus_disk_v[k])
                               : 0.0;
        const double pad = rad * 1.0e-3 + std::fabs(c) * 1.0e-6 + 1.0e-6;
        if (!(c - rad - pad > (double)b[k] && c + rad + pad < (double)b[3 + k])) return false;
    }
    return true;
}

// Whether walks leave box tests out (rtx_collapse.h): RTX_COLLAPSE=0 in the environment (read
// per plan) or the scene flag RTX_SCENE_EVERY_BOX keep every test.
bool collapse_enabled(bool every_box) {
    if (every_box) return false;
    const char* e = std::getenv("RTX_COLLAPSE");
    return !(e && std::strcmp(e, "0") == 0);
}

// The walk of one tree for one camera: `base` (the caller's tree) or `topo` oriented for octant
// `oct`, less the box tests the collapsed walk leaves out for paths from `cam`.
void plan_walk(const std::vector<rtx_entry>& base, const rtxd::Topology* topo, uint32_t oct,
               const std::vector<float>& quadtab, const rtx_camera& cam, bool collapse, std::vector<rtx_entry>& out,
               std::vector<uint8_t>& skip, std::vector<double>* reads) {
    std::vector<rtx_entry> full;
    if (topo) rtxd::emit_topology(*topo, oct, full);
    const std::vector<rtx_entry>& E = topo ? full : base;
    std::vector<double> pass;
    double walks = 0.0;
    rtxd::sample_node_passes(E, quadtab, cam, pass, &walks);
    rtxd::collapse_layout(E, pass, walks, collapse, out, skip, reads);
}

}  // namespace

bool camera_in_near(const rtx_scene* s, const rtx_camera* cam) {
    return s->tiered && camera_in_box(s->near_topo.near_box, cam);
}

// Each sphere's place in the reference walk of the caller's tree (its first entry in `base`): the walk's
// tie rule (sphere_test RANKED / RANK_WORD) for walks over another tree or in another storage order.
void rank_spheres(rtx_scene* s) {
    s->sphere_rank.clear();
    uint32_t k = 0;
    for (const rtx_entry& e : s->base) {
        int32_t tag, si;
        std::memcpy(&tag, &e.b[3], 4);
        std::memcpy(&si, &e.b[1], 4);
        if (tag < 0) continue;
        if (s->sphere_rank.size() <= (size_t)si) s->sphere_rank.resize((size_t)si + 1, 0xFFFFFFFFu);
        if (s->sphere_rank[(size_t)si] == 0xFFFFFFFFu) s->sphere_rank[(size_t)si] = k;
        ++k;
    }
}

// A scene whose base holds the reference's walk of one tree: take the walk's own tree when it
// qualifies (spheres only; rtxd::build_topology), and its near tree.
void adopt_topology(rtx_scene* s, uint32_t flags, const rtx_scene_desc* d) {
    s->every_box = (flags & RTX_SCENE_EVERY_BOX) != 0;
    const int mode = topology_mode(flags, s->base);
    if (mode != 0 && rtxd::build_topology(s->base, mode == 1, s->topo)) s->rebuilt = true;
    s->tiered = tier_topology(flags, s->base, d, s->near_topo);
}

// Layout slot of a camera: its octant for a rebuilt scene, else 0; near walks of a tiered scene
// at 8 + octant.
uint32_t layout_slot(const rtx_scene* s, const rtx_camera* cam, bool near) {
    return near ? 8u + rtxd::camera_octant(*cam) : (s->rebuilt ? rtxd::camera_octant(*cam) : 0u);
}

// The walk for `cam` as threaded entries (s->mu held), planned on the slot's first use.
int scene_layout(rtx_scene* s, const rtx_camera* cam, const std::vector<rtx_entry>** out, bool near) {
    const uint32_t k = layout_slot(s, cam, near);
    if (near && !s->tiered) return fail(RTX_ERR_INVALID_ARG, "scene has no near walk");
    if (!s->planned[k]) {
        const rtxd::Topology* t = near ? &s->near_topo : (s->rebuilt ? &s->topo : nullptr);
        plan_walk(s->base, t, k & 7u, s->quadtab, *cam, collapse_enabled(s->every_box), s->layouts[k], s->skips[k],
                  &s->reads[k]);
        s->planned[k] = true;
    }
    *out = &s->layouts[k];
    return RTX_OK;
}

uint64_t walk_layout(const rtx_scene* s, const rtx_camera* cam, bool tiered) {
    return (s->rebuilt ? rtxd::camera_octant(*cam) : RTX_LAYOUT_REFERENCE) | (tiered ? RTX_LAYOUT_TIERED : 0u);
}

int check_camera(const rtx_camera* cam) {
    if (!cam) return fail(RTX_ERR_INVALID_ARG, "camera is NULL");
    if (cam->image_width == 0 || cam->image_height == 0) return fail(RTX_ERR_INVALID_ARG, "empty image");
    if (cam->samples_per_pixel == 0) return fail(RTX_ERR_INVALID_ARG, "samples_per_pixel must be > 0");
    if ((uint64_t)cam->image_width * cam->image_height > 0xFFFFFFFFull)
        return fail(RTX_ERR_INVALID_ARG, "image has more than 2^32 pixels (RNG counter is 32-bit)");
    // the kernel's scratch slot of a pixel (64 per tile, tiles padded: at most 64 columns and 64 rows) is 32-bit
    if (((uint64_t)cam->image_width + 64) * ((uint64_t)cam->image_height + 64) > 0xFFFFFFFFull)
        return fail(RTX_ERR_INVALID_ARG, "image too large: its padded tiles exceed 2^32 pixel slots");
    return RTX_OK;
}

int check_region(const rtx_camera* cam, const rtx_region* r) {
    if (!r) return fail(RTX_ERR_INVALID_ARG, "region is NULL");
    if (r->world == 0 || r->rank >= r->world) return fail(RTX_ERR_INVALID_ARG, "bad shard %u/%u", r->rank, r->world);
    if (r->stripe > 4096 || (r->stripe & (r->stripe - 1)) != 0)
        return fail(RTX_ERR_INVALID_ARG, "stripe %u: 0 or a power of two up to 4096", r->stripe);
    if ((uint64_t)r->x0 + r->width > cam->image_width || (uint64_t)r->y0 + r->height > cam->image_height)
        return fail(RTX_ERR_INVALID_ARG, "region [%u+%u, %u+%u] outside %ux%u image", r->x0, r->width, r->y0, r->height,
                    cam->image_width, cam->image_height);
    return RTX_OK;
}

uint32_t region_rows(const rtx_region* r) {
    if (r->world == 0 || r->rank >= r->world) return 0;
    const uint32_t S = r->stripe > 1u ? r->stripe : 1u;
    const uint32_t nst = (r->height + S - 1) / S;  // stripes, the last one maybe partial
    if (r->rank >= nst) return 0;
    const uint32_t k = (nst - r->rank + r->world - 1) / r->world;  // this shard's stripes
    uint32_t rows = k * S;
    if ((nst - 1) % r->world == r->rank && r->height % S) rows -= S - r->height % S;  // it holds the partial one
    return rows;
}

// Stripe rows for the bands of rtx_render(n_gpus > 1): single rows (RTX_STRIPE = 2^k for A/B).  Every rank of
// the 4- and 8-GPU headline measured slowest-rank-fastest with single rows (profiles/r05_stripe_sweep.jsonl:
// N = 8 12.55 ms against 12.78 / 12.83 / 13.05 for 2 / 4 / 8-row stripes).
uint32_t band_stripe(int n) {
    const uint32_t v = n > 1 ? env_knob("RTX_STRIPE", 1, 1, 4096) : 1u;
    return 1u << (31 - __builtin_clz(v));  // a power of two
}

// The walk E in device form: all 'a' halves, then all 'b' halves (rtxd::SceneRef), each ending
// with the sentinel entry (rtx_layout.h).  Every entry names its successor (node: next
// and escape, primitive: next), so the storage order is free: a scene too big for the
// LDS copy stores its top levels first (out.hot entries), which v3 caches in LDS; a scene
// in the LDS copy stores its primitives first (below out.prim_end), so the asm walk knows
// an entry's kind from its position before the entry's read returns (walk_phase_asm).
PackedLayout pack_layout(const std::vector<rtx_entry>& E, const std::vector<double>* reads,
                         const std::vector<float>& quadtab, const std::vector<uint32_t>& sphere_rank,
                         uint32_t hot_cap) {
    PackedLayout out;
    out.n_entries = (uint32_t)E.size();
    const size_t n = E.size(), m = n + 1;
    std::vector<uint32_t> pos(m);  // storage index of entry i; the sentinel stays last
    for (size_t i = 0; i <= n; ++i) pos[i] = (uint32_t)i;
    if (m * 16 > rtxd::LDS_B) {
        std::vector<uint32_t> depth(n), ends, per_depth;
        for (size_t i = 0; i < n; ++i) {  // depth = nodes whose subtree holds entry i
            while (!ends.empty() && ends.back() <= i) ends.pop_back();
            depth[i] = (uint32_t)ends.size();
            if (per_depth.size() <= depth[i]) per_depth.resize(depth[i] + 1, 0);
            ++per_depth[depth[i]];
            int32_t tag, esc;
            std::memcpy(&tag, &E[i].b[3], 4);
            if (tag == RTX_E_NODE) {
                std::memcpy(&esc, &E[i].a[3], 4);
                ends.push_back((uint32_t)esc);
            }
        }
        const uint32_t cap = hot_cap;
        static const std::vector<double> none;
        const std::vector<double>& R = reads ? *reads : none;
        std::vector<uint8_t> in_hot(n, 0);
        uint32_t hot = 0;
        if (R.size() == n) {
            // the entries the walk reads most (the plan's sample estimate), in walk order
            std::vector<uint32_t> idx(n);
            for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
            const size_t take = std::min<size_t>(cap, n);
            std::partial_sort(idx.begin(), idx.begin() + take, idx.end(), [&](uint32_t a, uint32_t b) {
                return R[a] != R[b] ? R[a] > R[b] : depth[a] != depth[b] ? depth[a] < depth[b] : a < b;
            });
            for (size_t q = 0; q < take; ++q) in_hot[idx[q]] = 1;
            hot = (uint32_t)take;
        } else {  // the top levels
            uint32_t levels = 0;
            while (levels < per_depth.size() && hot + per_depth[levels] <= cap) hot += per_depth[levels++];
            for (size_t i = 0; i < n; ++i) in_hot[i] = depth[i] < levels;
        }
        uint32_t k = 0;
        for (size_t i = 0; i < n; ++i)
            if (in_hot[i]) pos[i] = k++;
        for (size_t i = 0; i < n; ++i)
            if (!in_hot[i]) pos[i] = k++;
        out.hot = hot;
    } else {
        // primitives first, in the reference walk's order (the caller's tree walks them in that
        // order; a rebuilt tree's are sorted back into it): the walk's tie rule compares entry
        // indices for that order (sphere_test RANKED, rtx_device.h)
        std::vector<uint32_t> prims;
        for (size_t i = 0; i < n; ++i) {
            int32_t tag;
            std::memcpy(&tag, &E[i].b[3], 4);
            if (tag != RTX_E_NODE) prims.push_back((uint32_t)i);
        }
        // quads before the spheres (in the walk's order: they have no tie rule), so a sphere never wins a tie
        // with a quad by the entry-index rule, as in the oracle (hit_rank: a quad's hit ranks 0)
        auto rank = [&](uint32_t i) -> int64_t {
            int32_t tag, si;
            std::memcpy(&tag, &E[i].b[3], 4);
            if (tag < 0) return -1;
            std::memcpy(&si, &E[i].b[1], 4);
            return (int64_t)sphere_rank[(uint32_t)si];
        };
        std::stable_sort(prims.begin(), prims.end(), [&](uint32_t a, uint32_t b) { return rank(a) < rank(b); });
        uint32_t k = 0;
        for (uint32_t i : prims) pos[i] = k++;
        for (size_t i = 0; i < n; ++i) {
            int32_t tag;
            std::memcpy(&tag, &E[i].b[3], 4);
            if (tag == RTX_E_NODE) pos[i] = k++;
        }
        for (size_t i = 0; i < n; ++i) {
            int32_t tag;
            std::memcpy(&tag, &E[i].b[3], 4);
            if (tag != RTX_E_NODE) out.prim_end = 16 * (pos[i] + 1) > out.prim_end ? 16 * (pos[i] + 1) : out.prim_end;
        }
    }
    out.start = 16 * pos[0];
    std::vector<float>& soa = out.soa;
    soa.assign(m * 8 + quadtab.size(), 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const size_t j = pos[i];
        std::memcpy(&soa[4 * j], E[i].a, 16);
        std::memcpy(&soa[4 * (m + j)], E[i].b, 16);
        int32_t tag, esc;  // the device recoding, rtx_layout.h
        std::memcpy(&tag, &E[i].b[3], 4);
        const int32_t next = (int32_t)(16 * pos[i + 1]);
        if (tag == RTX_E_NODE) {
            std::memcpy(&esc, &E[i].a[3], 4);
            esc = (int32_t)(16 * pos[esc]);
            std::memcpy(&soa[4 * j + 3], &esc, 4);
            std::memcpy(&soa[4 * (m + j) + 3], &next, 4);
        } else {
            std::memcpy(&soa[4 * (m + j) + 2], &next, 4);  // a primitive's successor
            if (tag >= 0) {
                const int32_t sph = RTX_DEV_SPHERE(tag);
                std::memcpy(&soa[4 * (m + j) + 3], &sph, 4);
                int32_t si;  // the sphere's rank word (sphere_test RANK_WORD) in place of its index
                std::memcpy(&si, &E[i].b[1], 4);
                std::memcpy(&soa[4 * (m + j) + 1], &sphere_rank[(uint32_t)si], 4);
            }
        }
    }
    // the sentinel: box min +inf, max -inf, escape = next = its own position
    const float inf = std::numeric_limits<float>::infinity();
    const int32_t self = (int32_t)(16 * n);
    for (int k = 0; k < 3; ++k) {
        soa[4 * n + k] = inf;
        soa[4 * (m + n) + k] = -inf;
    }
    std::memcpy(&soa[4 * n + 3], &self, 4);
    std::memcpy(&soa[4 * (m + n) + 3], &self, 4);
    if (!quadtab.empty()) std::memcpy(&soa[8 * m], quadtab.data(), quadtab.size() * sizeof(float));
    return out;
}

namespace {

// The checks of a scene description and its entries in the reference's visit order, for the queries that build no scene.
int flatten(const rtx_scene_desc* d, std::vector<rtx_entry>& base) {
    if (d->n_roots == 0 || !d->roots) return fail(RTX_ERR_INVALID_ARG, "scene has no root");
    if (d->n_nodes && !d->nodes) return fail(RTX_ERR_INVALID_ARG, "nodes is NULL");
    if (int rc = validate_tables(d)) return rc;
    if (int rc = check_acyclic(d)) return rc;
    for (uint32_t i = 0; i < d->n_roots; ++i)
        if (int rc = emit(d, d->roots[i], base)) return rc;
    return RTX_OK;
}

// A walk tree oriented for `octant` into the caller's nodes; t == nullptr: the scene has no such tree.
int copy_tree(const rtxd::Topology* t, uint32_t octant, rtx_bvh_node* nodes, uint32_t cap, uint32_t* n_nodes, int32_t* root) {
    std::vector<rtx_bvh_node> v;
    if (t) rtxd::orient_topology(*t, octant, v);
    *n_nodes = (uint32_t)v.size();
    *root = t ? t->root : -1;
    if (t && nodes && cap >= v.size()) std::memcpy(nodes, v.data(), v.size() * sizeof(rtx_bvh_node));
    return RTX_OK;
}

int copy_skip(const std::vector<uint8_t>& v, uint8_t* skip, uint32_t cap, uint32_t* n) {
    *n = (uint32_t)v.size();
    if (skip && cap >= v.size() && !v.empty()) std::memcpy(skip, v.data(), v.size());
    return RTX_OK;
}

// rtx_scene_walk_skip / rtx_scene_near_skip: the walk (or near walk) for `cam` planned, its skip flags copied out.
int scene_skip(rtx_scene* s, const rtx_camera* cam, bool near, uint8_t* skip, uint32_t cap, uint32_t* n) {
    g_last_error.clear();
    if (!s || !n) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_camera(cam)) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    const std::vector<rtx_entry>* E = nullptr;
    if (int rc = scene_layout(s, cam, &E, near)) return rc;
    return copy_skip(s->skips[layout_slot(s, cam, near)], skip, cap, n);
}

}  // namespace

}  // namespace rtxh

using namespace rtxh;

extern "C" {

uint32_t rtx_region_rows(const rtx_region* region) { return region ? region_rows(region) : 0; }
uint32_t rtx_region_row(const rtx_region* region, uint32_t i) {
    if (!region || region->world == 0) return 0;
    const uint32_t S = region->stripe > 1u ? region->stripe : 1u;
    return ((i / S) * region->world + region->rank) * S + i % S;
}

uint64_t rtx_scene_export(const rtx_scene* s, void* out, uint64_t cap) {
    if (!s) return 0;
    const uint64_t bytes = s->base.size() * sizeof(rtx_entry);
    if (out && cap >= bytes) std::memcpy(out, s->base.data(), bytes);
    return bytes;
}

int rtx_scene_topology(const rtx_scene* s, uint32_t octant, rtx_bvh_node* nodes, uint32_t cap, uint32_t* n_nodes,
                       int32_t* root) {
    g_last_error.clear();
    const bool near = (octant & RTX_TREE_NEAR) != 0;
    octant &= ~RTX_TREE_NEAR;
    if (!s || !n_nodes || !root || octant > 7) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    const bool has = near ? s->tiered : s->rebuilt;
    return copy_tree(has ? (near ? &s->near_topo : &s->topo) : nullptr, octant, nodes, cap, n_nodes, root);
}

uint32_t rtx_camera_octant(const rtx_camera* cam) { return cam ? rtxd::camera_octant(*cam) : 0u; }

int rtx_scene_walk_skip(rtx_scene* s, const rtx_camera* cam, uint8_t* skip, uint32_t cap, uint32_t* n) {
    return scene_skip(s, cam, false, skip, cap, n);
}

int rtx_scene_near_skip(rtx_scene* s, const rtx_camera* cam, uint8_t* skip, uint32_t cap, uint32_t* n) {
    return scene_skip(s, cam, true, skip, cap, n);
}

int rtx_scene_near_region(rtx_scene* s, const rtx_camera* cam, float box[6], uint32_t* active) {
    g_last_error.clear();
    if (!s || !box || !active) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_camera(cam)) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    *active = 0;
    if (!s->tiered) return RTX_OK;
    std::memcpy(box, s->near_topo.near_box, 6 * sizeof(float));
    *active = camera_in_near(s, cam) && !s->has_noise;
    return RTX_OK;
}

int rtx_walk_near_region(const rtx_scene_desc* d, uint32_t flags, const rtx_camera* cam, float box[6],
                         uint32_t* active) {
    g_last_error.clear();
    if (!d || !box || !active) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_camera(cam)) return rc;
    std::vector<rtx_entry> base;
    if (int rc = flatten(d, base)) return rc;
    *active = 0;
    rtxd::Topology nt;
    if (d->n_roots != 1 || !tier_topology(flags, base, d, nt)) return RTX_OK;
    std::memcpy(box, nt.near_box, 6 * sizeof(float));
    bool noise = false;
    for (uint32_t i = 0; i < d->n_textures; ++i) noise |= d->textures[i].type == RTX_TEX_NOISE;
    *active = camera_in_box(nt.near_box, cam) && !noise;
    return RTX_OK;
}

int rtx_walk_skip(const rtx_scene_desc* d, uint32_t flags, const rtx_camera* cam, uint8_t* skip, uint32_t cap,
                  uint32_t* n) {
    g_last_error.clear();
    if (!d || !n) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_camera(cam)) return rc;
    std::vector<rtx_entry> base;
    if (int rc = flatten(d, base)) return rc;
    rtxd::Topology t;
    const bool rebuilt = d->n_roots == 1 && topology_mode(flags, base) != 0 &&
                         rtxd::build_topology(base, topology_mode(flags, base) == 1, t);
    std::vector<float> quadtab;
    quad_table(d, quadtab);
    std::vector<rtx_entry> walk;
    std::vector<uint8_t> v;
    plan_walk(base, rebuilt ? &t : nullptr, rtxd::camera_octant(*cam), quadtab, *cam,
              collapse_enabled((flags & RTX_SCENE_EVERY_BOX) != 0), walk, v, nullptr);
    return copy_skip(v, skip, cap, n);
}

int rtx_walk_tree(const rtx_scene_desc* d, uint32_t flags, uint32_t octant, rtx_bvh_node* nodes, uint32_t cap,
                  uint32_t* n_nodes, int32_t* root) {
    g_last_error.clear();
    const bool near = (octant & RTX_TREE_NEAR) != 0;
    octant &= ~RTX_TREE_NEAR;
    if (!d || !n_nodes || !root || octant > 7) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    std::vector<rtx_entry> ref;
    if (int rc = flatten(d, ref)) return rc;
    rtxd::Topology t;
    const int mode = topology_mode(flags, ref);
    const bool has = d->n_roots == 1 &&
                     (near ? tier_topology(flags, ref, d, t) : (mode != 0 && rtxd::build_topology(ref, mode == 1, t)));
    return copy_tree(has ? &t : nullptr, octant, nodes, cap, n_nodes, root);
}

namespace {
int copy_lights(const std::vector<rtx_light>& v, rtx_light* out, uint32_t cap, uint32_t* n) {
    *n = (uint32_t)v.size();
    if (out && cap >= v.size() && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(rtx_light));
    return RTX_OK;
}
}  // namespace

namespace {
// The emitter table of a description and, when prims != nullptr, its per-primitive lookup (rtx_lights, rtx_prim_lights).
int desc_lights(const rtx_scene_desc* d, std::vector<rtx_light>& lights, std::vector<rtx_prim_light>* prims) {
    if (d->n_lists && !d->lists) return fail(RTX_ERR_INVALID_ARG, "lists is NULL");
    if (d->n_list_refs && !d->list_refs) return fail(RTX_ERR_INVALID_ARG, "list_refs is NULL");
    std::vector<rtx_entry> base;
    if (int rc = flatten(d, base)) return rc;
    std::vector<float> quadtab;
    quad_table(d, quadtab);
    return build_lights(base, quadtab, std::vector<rtx_material>(d->materials, d->materials + d->n_materials), lights, nullptr,
                        prims, d->n_spheres);
}
}  // namespace

int rtx_lights(const rtx_scene_desc* d, rtx_light* out, uint32_t cap, uint32_t* n) {
    g_last_error.clear();
    if (!d || !n) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    *n = 0;
    std::vector<rtx_light> lights;
    if (int rc = desc_lights(d, lights, nullptr)) return rc;
    return copy_lights(lights, out, cap, n);
}

int rtx_prim_lights(const rtx_scene_desc* d, rtx_prim_light* out, uint32_t cap, uint32_t* n_spheres, uint32_t* n) {
    g_last_error.clear();
    if (!d || !n || !n_spheres) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    *n = *n_spheres = 0;
    std::vector<rtx_light> lights;
    std::vector<rtx_prim_light> prims;
    if (int rc = desc_lights(d, lights, &prims)) return rc;
    *n_spheres = d->n_spheres;
    *n = (uint32_t)prims.size();
    if (out && cap >= prims.size() && !prims.empty()) std::memcpy(out, prims.data(), prims.size() * sizeof(rtx_prim_light));
    return RTX_OK;
}

int rtx_scene_lights(const rtx_scene* scene, rtx_light* out, uint32_t cap, uint32_t* n) {
    g_last_error.clear();
    if (!scene || !n) return fail(RTX_ERR_INVALID_ARG, "bad argument");
    *n = 0;
    rtx_scene* s = const_cast<rtx_scene*>(scene);  // (the table is made on first use, under the scene's mutex)
    std::lock_guard<std::mutex> lk(s->mu);
    if (int rc = scene_lights(s)) return rc;
    return copy_lights(s->lights, out, cap, n);
}

uint64_t rtx_scene_device_bytes(const rtx_scene* s) {
    if (!s) return 0;
    return s->base.size() * sizeof(rtx_entry) + s->quadtab.size() * sizeof(float) +
           s->materials.size() * sizeof(rtx_material) +
           s->textures.size() * sizeof(rtx_texture) + s->texels.size() * sizeof(uint32_t);
}

// MinF32 / MaxF32 (math.go:38-44): math.Min / math.Max of float32 values.
static float min_f32(float x, float y) {
    if ((std::isinf(x) && x < 0) || (std::isinf(y) && y < 0)) return -std::numeric_limits<float>::infinity();
    if (std::isnan(x) || std::isnan(y)) return std::numeric_limits<float>::quiet_NaN();
    if (x == 0 && x == y) return std::signbit(x) ? x : y;
    return x < y ? x : y;
}
static float max_f32(float x, float y) {
    if ((std::isinf(x) && x > 0) || (std::isinf(y) && y > 0)) return std::numeric_limits<float>::infinity();
    if (std::isnan(x) || std::isnan(y)) return std::numeric_limits<float>::quiet_NaN();
    if (x == 0 && x == y) return std::signbit(x) ? y : x;
    return x > y ? x : y;
}

// NewQuad (hittables.go:149-165) in float32, every operation rounded on its own (the unit is built without
// contraction): Cross vec3.go:129-135, Dot :137-139 (summed left to right), Unit :103-107 (the length through float64).
int rtx_quad_init(const float q[3], const float u[3], const float v[3], uint32_t material, rtx_quad* out) {
    g_last_error.clear();
    if (!q || !u || !v || !out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    const float n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const float nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const float inv_len = 1.0f / (float)std::sqrt((double)nn);
    const float inv = 1.0f / nn;
    rtx_quad r;
    std::memset(&r, 0, sizeof(r));
    for (int k = 0; k < 3; ++k) {
        r.q[k] = q[k];
        r.u[k] = u[k];
        r.v[k] = v[k];
        r.normal[k] = n[k] * inv_len;
        r.w[k] = n[k] * inv;
    }
    r.d = r.normal[0] * q[0] + r.normal[1] * q[1] + r.normal[2] * q[2];
    r.material = material;
    *out = r;
    return RTX_OK;
}

// Box (hittables.go:200-216): the six sides in its order, Scale(dz, -1) and Scale(dx, -1) as written (their zero
// components become -0).
int rtx_box_quads(const float a[3], const float b[3], uint32_t material, rtx_quad out[6]) {
    g_last_error.clear();
    if (!a || !b || !out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = min_f32(a[k], b[k]);
        mx[k] = max_f32(a[k], b[k]);
    }
    const float dx[3] = {mx[0] - mn[0], 0.0f, 0.0f}, dy[3] = {0.0f, mx[1] - mn[1], 0.0f}, dz[3] = {0.0f, 0.0f, mx[2] - mn[2]};
    const float ndx[3] = {dx[0] * -1.0f, dx[1] * -1.0f, dx[2] * -1.0f}, ndz[3] = {dz[0] * -1.0f, dz[1] * -1.0f, dz[2] * -1.0f};
    const float q0[3] = {mn[0], mn[1], mx[2]}, q1[3] = {mx[0], mn[1], mx[2]}, q2[3] = {mx[0], mn[1], mn[2]},
                q3[3] = {mn[0], mn[1], mn[2]}, q4[3] = {mn[0], mx[1], mx[2]};
    rtx_quad_init(q0, dx, dy, material, &out[0]);
    rtx_quad_init(q1, ndz, dy, material, &out[1]);
    rtx_quad_init(q2, ndx, dy, material, &out[2]);
    rtx_quad_init(q3, dz, dy, material, &out[3]);
    rtx_quad_init(q4, dx, ndz, material, &out[4]);
    rtx_quad_init(q3, dx, dz, material, &out[5]);
    return RTX_OK;
}

}  // extern "C"
