// query_harness.cpp — csrc/host_query.h and csrc/mesh_args_query.h on the host (tests/test_query_host.py); a stand-alone program, so
// it may be built with -fsanitize=address,undefined and run as it is.
//
//   query_harness lookup    query_mesh_of against a linear search: offsets with empty meshes (first, middle, last, several in a row),
//                           one-triangle meshes, the first and last triangle of each mesh, indices past the end, no mesh at all; and
//                           the layout
//   query_harness compose   the four surface kernels' arguments over a query allocation that is real host memory, filled as capi.hip
//                           fills the device's (so the sanitizer sees every read of a lent table), and made-up bases for the others:
//                           with and without emission maps, material maps, textures, mesh lights and smooth meshes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_query.h"
#include "../rust-pathtracer_amd/csrc/mesh_args_query.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static uint32_t linear_mesh_of(const std::vector<uint32_t>& first, uint32_t index)
{
    for (uint32_t m = 0; m + 1u < first.size(); ++m)
        if (first[m] <= index && index < first[m + 1u]) return m;
    return kQueryNone;
}

static int lookup()
{
    const std::vector<std::vector<uint32_t>> counts = {
        {1}, {5}, {1, 1, 1}, {0, 3}, {3, 0}, {2, 0, 4}, {0, 0, 1}, {1, 0, 0}, {0, 0, 0, 7, 0, 0, 1, 0}, {4, 1, 9, 1, 1, 300, 2}, {0}, {0, 0}, {},
    };
    uint32_t checked = 0;
    for (const std::vector<uint32_t>& c : counts) {
        std::vector<uint32_t> first(1, 0u);
        for (uint32_t n : c) first.push_back(first.back() + n);
        const uint32_t n_meshes = (uint32_t)c.size(), total = first.back();
        for (uint32_t k = 0; k < total + 3u; ++k) {                  // every triangle — so the first and last of each mesh — and past the end
            const uint32_t got = query_mesh_of(first.data(), n_meshes, k), want = linear_mesh_of(first, k);
            if (got != want) { printf("FAILED: %u meshes, index %u: got %u want %u\n", n_meshes, k, got, want); return 1; }
            if (got != kQueryNone) REQUIRE(c[got] != 0u && k - first[got] < c[got]);
            checked += 1;
        }
        REQUIRE(query_mesh_of(first.data(), n_meshes, 0xFFFFFFFFu) == kQueryNone);
    }
    // a large scene: 1000 meshes of 0 .. 6 triangles
    {
        std::vector<uint32_t> first(1, 0u);
        uint32_t x = 12345u;
        for (int m = 0; m < 1000; ++m) { x = x * 1664525u + 1013904223u; first.push_back(first.back() + (x >> 24) % 7u); }
        for (uint32_t k = 0; k < first.back(); ++k) REQUIRE(query_mesh_of(first.data(), 1000u, k) == linear_mesh_of(first, k));
    }
    // the layout: nothing overlaps, everything 16-byte aligned
    for (uint32_t n_meshes : {0u, 1u, 3u, 1000u}) for (uint32_t n_tris : {0u, 1u, 31u, 32u, 33u, 100000u}) {
        const QueryLayout ql(n_meshes, n_tris);
        REQUIRE(ql.off_tri_first == 0 && ql.off_none >= 4u * (n_meshes + 1u) && ql.off_flat_bits >= ql.off_none + 4u * (size_t)n_tris);
        REQUIRE(ql.off_zero >= ql.off_flat_bits + 4u * ((n_tris + 31u) / 32u) && ql.total >= ql.off_zero + kQueryDescBytes * (n_meshes + 1u));
        REQUIRE(ql.off_none % 16 == 0 && ql.off_flat_bits % 16 == 0 && ql.off_zero % 16 == 0 && ql.total % 16 == 0);
    }
    printf("lookup OK %u\n", checked);
    return 0;
}

// ---- the composer --------------------------------------------------------------------------------------------------------------------
using namespace rptargs;
constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3, kMeshes = 2;

// the query allocation as capi.hip's ensure_query fills the device's
static std::vector<unsigned char> query_allocation(const RefitPlan& rp)
{
    const QueryLayout ql(rp.n_meshes(), kTris);
    std::vector<unsigned char> a(ql.total, 0);
    memset(a.data() + ql.off_none, 0xFF, 4u * kTris);
    memcpy(a.data() + ql.off_tri_first, rp.tri_first.data(), 4u * rp.tri_first.size());
    return a;
}

template <class S> static int compose_one(const MeshView& v, const MmapView& m, bool material_maps, const EmapView& e, bool emission_maps, const QueryView& qv, const char* name)
{
    using MapS = typename emit_base_of<S>::type;
    using Base = typename map_base_of<MapS>::type;
    const S s = mesh_query_scene_of<S>(v, m, material_maps, e, emission_maps, qv);
    unsigned char* base = static_cast<unsigned char*>(qv.query);
    const unsigned char* none = base + qv.layout.off_none;
    const unsigned char* zero = base + qv.layout.off_zero;
    Base want = mesh_scene_of<Base>(v);
    if (!v.has_smooth()) want.smooth_bits = reinterpret_cast<const uint32_t*>(base + qv.layout.off_flat_bits);
    if (!v.has_lights()) want.tri_light = reinterpret_cast<const uint32_t*>(none);
    if (!v.has_tex()) want.tri_tex = reinterpret_cast<const uint32_t*>(none);
    REQUIRE(memcmp(static_cast<const Base*>(&s), &want, sizeof(Base)) == 0);              // every base field, padding included (S s{} zeroes it)
    REQUIRE((reinterpret_cast<const unsigned char*>(s.map_desc) == zero) == !material_maps);
    REQUIRE((reinterpret_cast<const unsigned char*>(s.emit_desc) == zero) == !emission_maps);
    if (material_maps) REQUIRE(reinterpret_cast<const unsigned char*>(s.map_desc) >= static_cast<const unsigned char*>(m.mmap));
    if (emission_maps) REQUIRE(reinterpret_cast<const unsigned char*>(s.emit_desc) >= static_cast<const unsigned char*>(e.emap));
    // what a lent table holds, read through the argument's own pointers (real memory: the sanitizer checks every read)
    if (!material_maps) for (uint32_t j = 0; j <= kMeshes; ++j) REQUIRE(s.map_desc[j].flags == 0u);
    if (!emission_maps) for (uint32_t j = 0; j <= kMeshes; ++j) REQUIRE(s.emit_desc[j].flags == 0u && s.emit_light_desc[j].flags == 0u);
    if (!v.has_smooth()) for (uint32_t w = 0; w < (kTris + 31) / 32; ++w) REQUIRE(s.smooth_bits[w] == 0u);
    if (!v.has_lights()) { for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_light[k] == kLightNone); REQUIRE(s.n_pick >= s.n_lights); }
    if (!v.has_tex()) for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_tex[k] == kTexNone);
    REQUIRE(s.tri_light != nullptr && s.tri_tex != nullptr && s.smooth_bits != nullptr && s.map_desc != nullptr && s.emit_desc != nullptr);
    REQUIRE(s.n_tris == kTris && s.n_lights == kSceneLights);
    printf("%s emap %s mmap %s tex %s lights %s smooth %s\n", name, emission_maps ? "own" : "lent", material_maps ? "own" : "lent", v.has_tex() ? "own" : "lent",
           v.has_lights() ? "own" : "lent", v.has_smooth() ? "own" : "lent");
    return 0;
}

static int compose()
{
    for (int bits = 0; bits < 32; ++bits) {
        const bool emaps = bits & 1, maps = bits & 2, lights = bits & 4, tex = bits & 8, smooth = bits & 16;
        if ((emaps || maps) && !tex) continue;                       // a map needs a texture
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        RefitPlan rp; SmoothPlan sp; LightPlan lp; TexPlan tp; EnvPlan ep; CutPlan cp; NrmPlan np; MmapPlan mp; EmapPlan emp;
        rp.ok = true; rp.mesh_first = {0, 5, kVertices}; rp.tri_first = {0, 20, kTris}; rp.n_slots = kTris; rp.mesh_material = {0, 1};
        void* const refit = (void*)(1ull << 40);
        void *smooth_a = nullptr, *light_a = nullptr, *tex_a = nullptr, *mmap_a = nullptr, *emap_a = nullptr;
        if (smooth) { sp.mode = {1, 0}; sp.n_tris = kTris; smooth_a = (void*)(2ull << 40); }
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        if (tex) { tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4; tex_a = (void*)(4ull << 40); }
        cp.mask.resize(2); cp.mask[0].width = cp.mask[0].height = 3; cp.n_meshes = 2; cp.n_tris = kTris; cp.n_words = 1;
        void* const cut_a = (void*)(6ull << 40);
        np.map.resize(2); np.map[0].width = np.map[0].height = 3; np.n_meshes = 2; np.n_tris = kTris; np.n_texels = 9;
        void* const nrm_a = (void*)(7ull << 40);
        if (maps) { mp.map.resize(2); mp.map[0].width = 3; mp.map[0].height = 5; mp.n_meshes = 2; mp.n_tris = kTris; mp.n_texels = 15; mmap_a = (void*)(8ull << 40); }
        if (emaps) {
            std::vector<EmapMap> em(2);
            em[0].width = 4; em[0].height = 6;
            build_emap_plan(rp, em, emp);
            emap_a = (void*)(9ull << 40);
        }
        std::vector<unsigned char> query_mem = query_allocation(rp);
        const MmapView m{mmap_a, mp};
        const EmapView e{emap_a, emp};
        const QueryView qv{query_mem.data(), QueryLayout(rp.n_meshes(), kTris)};
        const bool material_maps = mmap_a && mp.any(), emission_maps = emap_a && emp.any();
        REQUIRE(material_maps == maps && emission_maps == emaps);
        // (the cutout and normal-map kernels are only taken while those features are present, and they need a texture)
        const MeshView plain{scene, refit, smooth_a, light_a, tex_a, nullptr, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_cut{scene, refit, smooth_a, light_a, tex_a, nullptr, cut_a, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_nrm{scene, refit, smooth_a, light_a, tex_a, nullptr, nullptr, nrm_a, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_all{scene, refit, smooth_a, light_a, tex_a, nullptr, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};
        printf("bits %d\n", bits);
        REQUIRE(compose_one<SceneMeshEmit>(plain, m, material_maps, e, emission_maps, qv, "surface") == 0);
        if (tex) {
            REQUIRE(compose_one<SceneMeshEmitCut>(with_cut, m, material_maps, e, emission_maps, qv, "surface_cut") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrm>(with_nrm, m, material_maps, e, emission_maps, qv, "surface_nrm") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrmCut>(with_all, m, material_maps, e, emission_maps, qv, "surface_nrm_cut") == 0);
        }
        // the first-triangle offsets the kernels search are the plan's
        const uint32_t* first = reinterpret_cast<const uint32_t*>(query_mem.data() + qv.layout.off_tri_first);
        REQUIRE(query_mesh_of(first, kMeshes, 0) == 0 && query_mesh_of(first, kMeshes, 19) == 0 && query_mesh_of(first, kMeshes, 20) == 1 &&
                query_mesh_of(first, kMeshes, kTris - 1) == 1 && query_mesh_of(first, kMeshes, kTris) == kQueryNone);
    }
    REQUIRE(query_surface_kind_of(false, false) == 0u && query_surface_kind_of(true, false) == kQueryCut && query_surface_kind_of(false, true) == kQueryNrm &&
            query_surface_kind_of(true, true) == (kQueryCut | kQueryNrm));
    printf("compose OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "lookup")) return lookup();
    if (argc == 2 && !strcmp(argv[1], "compose")) return compose();
    fprintf(stderr, "usage: query_harness lookup | compose\n");
    return 2;
}
