// pack_layout_check.cpp — the stand-alone checker of tests/test_pack_layout.py: rtxh::pack_layout (rtx_scene.hip), the
// storage order of a walk on the device, on three scenes built here.  Host code only: no HIP, nothing loaded.
// Exits 0 and prints one line per scene, or exits 1 with a message.
#define RTX_HOST_ONLY
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <tuple>

#include "../raytracer-go_amd/csrc/rtx_internal.h"

namespace {

[[noreturn]] void die(const char* scene, const char* fmt, ...) {
    std::fprintf(stderr, "pack_layout_check: %s: ", scene);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "\n");
    std::exit(1);
}
#define CHECK(cond, ...) \
    do {                 \
        if (!(cond)) die(scene, __VA_ARGS__); \
    } while (0)

int32_t word(const float& f) {
    int32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}
void set_word(float& f, int32_t w) { std::memcpy(&f, &w, 4); }

// Entries in the input form (rtx_layout.h): pre-order, a node names its escape by entry index.
rtx_entry node_entry(size_t k) {  // (the escape is closed by the caller)
    rtx_entry e{};
    for (int c = 0; c < 3; ++c) {
        e.a[c] = -1.0f - (float)k - 0.25f * c;
        e.b[c] = 1.0f + (float)k + 0.25f * c;
    }
    set_word(e.b[3], RTX_E_NODE);
    return e;
}
rtx_entry sphere_entry(uint32_t sphere, uint32_t material) {
    rtx_entry e{};
    e.a[0] = 0.5f * sphere;
    e.a[1] = 1.0f + sphere;
    e.a[2] = -2.0f * sphere;
    e.a[3] = 0.5f + sphere;  // radius
    e.b[0] = e.a[3] * e.a[3];
    set_word(e.b[1], (int32_t)sphere);
    set_word(e.b[3], (int32_t)material);
    return e;
}
rtx_entry quad_entry(uint32_t quad) {
    rtx_entry e{};
    e.a[0] = 0.0f;
    e.a[1] = 1.0f;
    e.a[2] = 0.0f;
    e.a[3] = 3.0f + quad;
    set_word(e.b[0], (int32_t)quad);
    set_word(e.b[3], RTX_E_QUAD);
    return e;
}
int32_t tag_of(const rtx_entry& e) { return word(e.b[3]); }

// A balanced tree over spheres [lo, hi); depth[i]: the nodes whose subtree holds entry i.
void balanced(uint32_t lo, uint32_t hi, uint32_t d, std::vector<rtx_entry>& E, std::vector<uint32_t>& depth) {
    if (hi - lo == 1) {
        E.push_back(sphere_entry(lo, lo % 7));
        depth.push_back(d);
        return;
    }
    const size_t me = E.size();
    E.push_back(node_entry(me));
    depth.push_back(d);
    const uint32_t mid = lo + (hi - lo) / 2;
    balanced(lo, mid, d + 1, E, depth);
    balanced(mid, hi, d + 1, E, depth);
    set_word(E[me].a[3], (int32_t)E.size());
}

// What holds of every packed layout.  Returns pos: the storage position of every entry (pos[n] = n, the sentinel).
std::vector<uint32_t> check_common(const char* scene, const std::vector<rtx_entry>& E, const std::vector<float>& quadtab,
                                   const std::vector<uint32_t>& rank, const rtxh::PackedLayout& P) {
    const size_t n = E.size(), m = n + 1;
    CHECK(P.n_entries == n, "n_entries %u, expected %zu", P.n_entries, n);
    CHECK(P.soa.size() == 8 * m + quadtab.size(), "%zu floats, expected %zu", P.soa.size(), 8 * m + quadtab.size());
    const float* A = P.soa.data();
    const float* B = P.soa.data() + 4 * m;
    // following start and each stored next visits the entries in the input's pre-order
    std::vector<uint32_t> pos(m, 0xFFFFFFFFu);
    std::vector<uint8_t> taken(m, 0);
    uint32_t at = P.start;
    for (size_t i = 0; i < n; ++i) {
        CHECK(at % 16 == 0 && at / 16 < n, "step %zu of the walk is at position %u (of %zu entries)", i, at, n);
        const uint32_t j = at / 16;
        CHECK(!taken[j], "position %u is reached twice (entry %zu)", j, i);
        taken[j] = 1;
        pos[i] = j;
        const int32_t tag = tag_of(E[i]);
        const bool is_node = tag == RTX_E_NODE;
        CHECK(std::memcmp(&A[4 * j], E[i].a, 12) == 0, "entry %zu: 'a' half at position %u differs", i, j);
        CHECK(std::memcmp(&B[4 * j], E[i].b, 4) == 0, "entry %zu: b[0] at position %u differs", i, j);
        if (is_node) {
            CHECK(std::memcmp(&B[4 * j + 1], &E[i].b[1], 8) == 0, "node %zu: box max differs", i);
            CHECK(word(B[4 * j + 3]) >= 0, "node %zu: stored b.w %d is no position", i, word(B[4 * j + 3]));
            at = (uint32_t)word(B[4 * j + 3]);
        } else {
            CHECK(A[4 * j + 3] == E[i].a[3], "primitive %zu: a[3] differs", i);
            if (tag >= 0) {  // a sphere: its rank word and the device recoding of its material
                const uint32_t si = (uint32_t)word(E[i].b[1]);
                CHECK((uint32_t)word(B[4 * j + 1]) == rank[si], "sphere entry %zu: b[1] %d, rank word %u expected", i,
                      word(B[4 * j + 1]), rank[si]);
                CHECK(word(B[4 * j + 3]) == RTX_DEV_SPHERE(tag), "sphere entry %zu: b[3] %d, RTX_DEV_SPHERE(%d) = %d expected",
                      i, word(B[4 * j + 3]), tag, RTX_DEV_SPHERE(tag));
            } else {
                CHECK(word(B[4 * j + 3]) == RTX_E_QUAD, "quad entry %zu: b[3] %d", i, word(B[4 * j + 3]));
            }
            at = (uint32_t)word(B[4 * j + 2]);
        }
    }
    // the stored positions are a permutation with the sentinel last, naming itself in both halves
    CHECK(at == 16 * n, "the walk ends at position %u, not at the sentinel %zu", at, 16 * n);
    pos[n] = (uint32_t)n;
    const float inf = std::numeric_limits<float>::infinity();
    for (int c = 0; c < 3; ++c)
        CHECK(A[4 * n + c] == inf && B[4 * n + c] == -inf, "the sentinel's box is not empty (component %d)", c);
    CHECK(word(A[4 * n + 3]) == (int32_t)(16 * n) && word(B[4 * n + 3]) == (int32_t)(16 * n),
          "the sentinel names %d / %d, not itself (%zu)", word(A[4 * n + 3]), word(B[4 * n + 3]), 16 * n);
    CHECK(P.start == 16 * pos[0], "start %u, the root is at %u", P.start, 16 * pos[0]);
    // each node's stored escape is 16 times the position of the entry that the input's escape names
    for (size_t i = 0; i < n; ++i)
        if (tag_of(E[i]) == RTX_E_NODE) {
            const int32_t esc = word(E[i].a[3]);
            CHECK(esc > (int32_t)i && (size_t)esc <= n, "scene bug: node %zu escapes to %d", i, esc);
            CHECK(word(A[4 * pos[i] + 3]) == (int32_t)(16 * pos[esc]), "node %zu: stored escape %d, expected %u", i,
                  word(A[4 * pos[i] + 3]), 16 * pos[esc]);
        }
    // the quad table follows at float offset 8 * (n + 1)
    CHECK(quadtab.empty() || std::memcmp(&P.soa[8 * m], quadtab.data(), quadtab.size() * sizeof(float)) == 0,
          "the quad table at float offset %zu differs", 8 * m);
    return pos;
}

// A scene in the LDS copy: primitives first (quads, then spheres by rank), then the nodes.
void check_lds(const char* scene, const std::vector<rtx_entry>& E, const std::vector<float>& quadtab,
               const std::vector<uint32_t>& rank) {
    CHECK((E.size() + 1) * 16 <= rtxd::LDS_B, "scene bug: %zu entries do not take the LDS branch", E.size());
    const rtxh::PackedLayout P = rtxh::pack_layout(E, nullptr, quadtab, rank, 64);
    const std::vector<uint32_t> pos = check_common(scene, E, quadtab, rank, P);
    const size_t n = E.size();
    size_t prims = 0, quads = 0;
    for (const rtx_entry& e : E) {
        prims += tag_of(e) != RTX_E_NODE;
        quads += tag_of(e) == RTX_E_QUAD;
    }
    CHECK(P.hot == 0, "hot %u in the LDS branch", P.hot);
    CHECK(P.prim_end == 16 * prims, "prim_end %u, expected %zu", P.prim_end, 16 * prims);
    // by position: the key every primitive must be sorted by — quads (-1) before spheres, spheres by rank, ties and
    // quads in the walk's order
    std::vector<std::pair<int64_t, size_t>> key(prims, {0, 0});
    for (size_t i = 0; i < n; ++i) {
        const int32_t tag = tag_of(E[i]);
        if (tag == RTX_E_NODE) {
            CHECK(16 * pos[i] >= P.prim_end, "node %zu at position %u, below prim_end %u", i, pos[i], P.prim_end);
            continue;
        }
        CHECK(16 * pos[i] < P.prim_end, "primitive %zu at position %u, not below prim_end %u", i, pos[i], P.prim_end);
        CHECK(tag != RTX_E_QUAD || pos[i] < quads, "quad entry %zu at position %u: not before the spheres", i, pos[i]);
        key[pos[i]] = {tag == RTX_E_QUAD ? -1 : (int64_t)rank[(uint32_t)word(E[i].b[1])], i};
    }
    for (size_t j = 1; j < prims; ++j)
        CHECK(key[j - 1] < key[j], "positions %zu and %zu (entries %zu, %zu) are out of sphere_rank order", j - 1, j,
              key[j - 1].second, key[j].second);
    std::printf("%s: ok (%zu entries, prim_end %u)\n", scene, n, P.prim_end);
}

// A scene too big for the LDS copy: the chosen entries first, in walk order, then the others.
void check_big(const char* scene, const std::vector<rtx_entry>& E, const std::vector<uint32_t>& depth,
               const std::vector<uint32_t>& rank, const std::vector<double>* reads, uint32_t cap) {
    const size_t n = E.size();
    CHECK((n + 1) * 16 > rtxd::LDS_B, "scene bug: %zu entries do not take the big-scene branch", n);
    const std::vector<float> no_quads;
    const rtxh::PackedLayout P = rtxh::pack_layout(E, reads, no_quads, rank, cap);
    const std::vector<uint32_t> pos = check_common(scene, E, no_quads, rank, P);
    CHECK(P.prim_end == 0, "prim_end %u in the big-scene branch", P.prim_end);
    CHECK(P.hot <= cap, "hot %u exceeds the cap %u", P.hot, cap);
    std::vector<uint8_t> chosen(n, 0);
    if (reads) {  // the cap's most-read entries: by reads, then depth, then index
        std::vector<std::tuple<double, uint32_t, uint32_t>> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = {-(*reads)[i], depth[i], (uint32_t)i};
        std::sort(order.begin(), order.end());
        CHECK(P.hot == std::min<size_t>(cap, n), "hot %u, expected %zu", P.hot, std::min<size_t>(cap, n));
        for (uint32_t q = 0; q < P.hot; ++q) chosen[std::get<2>(order[q])] = 1;
    } else {  // whole top levels, as many as fit
        std::vector<uint32_t> per_depth;
        for (uint32_t d : depth) {
            if (per_depth.size() <= d) per_depth.resize(d + 1, 0);
            ++per_depth[d];
        }
        uint32_t levels = 0, hot = 0;
        while (levels < per_depth.size() && hot + per_depth[levels] <= cap) hot += per_depth[levels++];
        CHECK(levels > 0 && hot < n, "scene bug: the cap %u holds %u levels", cap, levels);
        CHECK(P.hot == hot, "hot %u, the %u whole levels that fit hold %u", P.hot, levels, hot);
        for (size_t i = 0; i < n; ++i) chosen[i] = depth[i] < levels;
    }
    // exactly the first `hot` positions hold the chosen entries; both groups in walk order
    uint32_t next_hot = 0, next_cold = P.hot;
    for (size_t i = 0; i < n; ++i) {
        uint32_t& expect = chosen[i] ? next_hot : next_cold;
        CHECK(pos[i] == expect, "entry %zu (%s) at position %u, expected %u", i, chosen[i] ? "hot" : "not hot", pos[i], expect);
        ++expect;
    }
    CHECK(next_hot == P.hot, "%u entries chosen, hot %u", next_hot, P.hot);
    std::printf("%s: ok (%zu entries, hot %u)\n", scene, n, P.hot);
}

}  // namespace

int main() {
    {  // 1. three spheres and one quad under two nodes: the LDS branch
        std::vector<rtx_entry> E = {node_entry(0),      node_entry(1),      sphere_entry(0, 4),
                                    quad_entry(0),      sphere_entry(1, 0), sphere_entry(2, 9)};
        set_word(E[0].a[3], 6);
        set_word(E[1].a[3], 4);
        std::vector<float> quadtab(16);
        for (size_t k = 0; k < quadtab.size(); ++k) quadtab[k] = 100.0f + (float)k;
        check_lds("spheres and a quad", E, quadtab, {2, 0, 1});
    }
    {  // 2. one sphere referenced twice
        std::vector<rtx_entry> E = {node_entry(0), node_entry(1), sphere_entry(1, 3), sphere_entry(0, 2), sphere_entry(1, 3)};
        set_word(E[0].a[3], 5);
        set_word(E[1].a[3], 4);
        check_lds("a sphere referenced twice", E, {}, {1, 0});
    }
    {  // 3. a balanced tree of 1025 spheres, 2049 entries: the smallest that takes the big-scene branch
        std::vector<rtx_entry> E;
        std::vector<uint32_t> depth, rank(1025);
        balanced(0, 1025, 0, E, depth);
        const char* scene = "1025 spheres";
        CHECK(E.size() == 2049, "scene bug: %zu entries", E.size());
        for (uint32_t i = 0; i < 1025; ++i) rank[i] = (i * 7u) % 1025u;  // (a permutation: 7 and 1025 are coprime)
        std::vector<double> reads(E.size());  // many ties, so that depth and index decide too
        for (size_t i = 0; i < E.size(); ++i) reads[i] = (double)((i * 2654435761ull >> 7) % 23);
        check_big("1025 spheres, by reads", E, depth, rank, &reads, 64);
        check_big("1025 spheres, top levels", E, depth, rank, nullptr, 64);
    }
    return 0;
}
