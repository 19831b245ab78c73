// rtx_capi.hip — the C-ABI of librtx.so (include/rtx.h): version, build info, the last error, and a scene's life.
//
// Host-side half of the drop-in boundary: the caller's flattened Hittable tree is validated and converted once into
// the threaded pre-order layout (rtx_scene.hip), kept resident in HBM per device and rendered by the megakernel
// (rtx_render.hip and the units rtx_internal.h lists).  Errors are returned as codes with a thread-local message;
// nothing throws across the ABI.
#include <cstring>

#include "rtx_bvh.h"
#include "rtx_internal.h"

using namespace rtxh;

namespace {

// Quad table, materials, textures and texels of a scene whose entries are built; then
// the copy on the current device.  Takes ownership of s (deleted on failure).
int finish_scene(rtx_scene* s, const rtx_scene_desc* d, rtx_scene** out) {
    quad_table(d, s->quadtab);
    s->materials.assign(d->materials, d->materials + d->n_materials);
    s->textures.assign(d->textures, d->textures + d->n_textures);
    for (const rtx_texture& t : s->textures) {
        s->has_image |= t.type == RTX_TEX_IMAGE;
        s->has_noise |= t.type == RTX_TEX_NOISE;
    }
    if (d->n_texels) s->texels.assign(d->texels, d->texels + d->n_texels);
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) {
        delete s;
        return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    }
    DeviceCopy* c = nullptr;
    if (int rc = ensure_device(s, cur, &c)) {
        for (auto& kv : s->copies) drop_copy(*kv.second);
        delete s;
        return rc;
    }
    *out = s;
    return RTX_OK;
}

}  // namespace

extern "C" {

int rtx_version(void) { return RTX_ABI_VERSION; }

// (No build date: the library's bytes depend on its sources only, so the PMC profiles bench.py ties to the
// library's hash stay valid across rebuilds of the same sources.)
const char* rtx_build_info(void) {
    return "librtx gfx950 megakernel (ABI 9: persistent (pixel, sample) item waves, LDS scene, threaded pre-order BVH "
           "(binned-SAH walk trees per camera octant: tiered near / guarded, or the caller's), collapsed walk, "
           "RGBA16 image texels, RCCL band gather, PPM on device 0 for any band count)";
}

const char* rtx_last_error(void) { return g_last_error.c_str(); }

int rtx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rtx_scene_create(const rtx_scene_desc* d, rtx_scene** out) { return rtx_scene_create_ex(d, 0u, out); }

int rtx_scene_create_ex(const rtx_scene_desc* d, uint32_t flags, rtx_scene** out) {
    g_last_error.clear();
    if (!d || !out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (d->n_roots == 0 || !d->roots) return fail(RTX_ERR_INVALID_ARG, "scene has no root");
    if (d->n_nodes && !d->nodes) return fail(RTX_ERR_INVALID_ARG, "nodes is NULL");
    if (d->n_lists && !d->lists) return fail(RTX_ERR_INVALID_ARG, "lists is NULL");
    if (d->n_list_refs && !d->list_refs) return fail(RTX_ERR_INVALID_ARG, "list_refs is NULL");
    if (int rc = validate_tables(d)) return rc;
    if (int rc = check_acyclic(d)) return rc;
    rtx_scene* s = new rtx_scene();
    for (uint32_t i = 0; i < d->n_roots; ++i) {
        if (int rc = emit(d, d->roots[i], s->base)) {
            delete s;
            return rc;
        }
    }
    rank_spheres(s);
    if (d->n_roots == 1) adopt_topology(s, flags, d);
    else s->every_box = (flags & RTX_SCENE_EVERY_BOX) != 0;
    return finish_scene(s, d, out);
}

int rtx_scene_create_spheres(const rtx_sphere* spheres, uint32_t n_spheres, const rtx_material* materials,
                             uint32_t n_materials, const rtx_texture* textures, uint32_t n_textures,
                             const uint32_t* texels, uint64_t n_texels, uint64_t bvh_seed, uint64_t bvh_draw0,
                             rtx_scene** out, double* build_ms) {
    g_last_error.clear();
    if (!out || !spheres) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (n_spheres == 0) return fail(RTX_ERR_INVALID_ARG, "empty World (NewBVH indexes h[0], bvh.go:164)");
    if (n_spheres > (1u << 25)) return fail(RTX_ERR_INVALID_ARG, "too many spheres for the GPU BVH build");
    rtx_scene_desc d{};
    d.spheres = spheres;
    d.n_spheres = n_spheres;
    d.materials = materials;
    d.n_materials = n_materials;
    d.textures = textures;
    d.n_textures = n_textures;
    d.texels = texels;
    d.n_texels = n_texels;
    if (int rc = validate_tables(&d)) return rc;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    rtx_scene* s = new rtx_scene();
    double ms = 0;
    hipError_t e = rtxd::build_sphere_bvh(spheres, n_spheres, bvh_seed, bvh_draw0, s->base, &ms);
    if (e != hipSuccess) {
        delete s;
        return hip_fail(e, "GPU BVH build");
    }
    if (build_ms) *build_ms = ms;
    rank_spheres(s);
    adopt_topology(s, 0u, &d);
    return finish_scene(s, &d, out);
}

int rtx_scene_create_world(const int32_t* items, uint32_t n_items, const rtx_sphere* spheres, uint32_t n_spheres,
                           const rtx_quad* quads, uint32_t n_quads, const rtx_material* materials, uint32_t n_materials,
                           const rtx_texture* textures, uint32_t n_textures, const uint32_t* texels, uint64_t n_texels,
                           uint64_t bvh_seed, uint64_t bvh_draw0, rtx_scene** out, double* build_ms) {
    g_last_error.clear();
    if (!out) return fail(RTX_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (n_items == 0) return fail(RTX_ERR_INVALID_ARG, "empty World (NewBVH indexes h[0], bvh.go:163)");
    if (n_items > (1u << 25)) return fail(RTX_ERR_INVALID_ARG, "too many items for the GPU BVH build");
    if (!items && (uint64_t)n_spheres + n_quads != n_items)
        return fail(RTX_ERR_INVALID_ARG, "items is NULL: n_items %u is not n_spheres + n_quads (%u + %u)", n_items,
                    n_spheres, n_quads);
    rtx_scene_desc d{};
    d.spheres = spheres;
    d.n_spheres = n_spheres;
    d.quads = quads;
    d.n_quads = n_quads;
    d.materials = materials;
    d.n_materials = n_materials;
    d.textures = textures;
    d.n_textures = n_textures;
    d.texels = texels;
    d.n_texels = n_texels;
    if (int rc = validate_tables(&d)) return rc;
    std::vector<int32_t> every;
    if (!items) {  // every sphere in table order, then every quad
        every.reserve(n_items);
        for (uint32_t i = 0; i < n_spheres; ++i) every.push_back(RTX_REF_PRIM(RTX_PRIM_SPHERE, i));
        for (uint32_t i = 0; i < n_quads; ++i) every.push_back(RTX_REF_PRIM(RTX_PRIM_QUAD, i));
        items = every.data();
    }
    if (int rc = check_world_items(&d, items, n_items)) return rc;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return fail(RTX_ERR_NO_DEVICE, "no HIP device");
    rtx_scene* s = new rtx_scene();
    double ms = 0;
    hipError_t e = rtxd::build_world_bvh(items, n_items, spheres, n_spheres, quads, n_quads, bvh_seed, bvh_draw0,
                                         s->base, &ms);
    if (e != hipSuccess) {
        delete s;
        return hip_fail(e, "GPU BVH build");
    }
    if (build_ms) *build_ms = ms;
    rank_spheres(s);
    adopt_topology(s, 0u, &d);
    return finish_scene(s, &d, out);
}

void rtx_scene_destroy(rtx_scene* s) {
    if (!s) return;
    for (auto& kv : s->copies) drop_copy(*kv.second);
    delete s;
}


}  // extern "C"
