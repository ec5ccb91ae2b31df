// emap_harness.cpp — csrc/host_emap.h and csrc/mesh_args_emap.h on the host (tests/test_mesh_emission_map_host.py); a stand-alone
// program, so it may be built with -fsanitize=address,undefined and run as it is.
//
//   emap_harness decode IN OUT   IN:  u32 n_texels, f32 gamma, then n_texels x 4 bytes RGBA
//                                OUT: n_texels x 4 f32 (tex_decode_reference: the decode is "mesh textures"')
//   emap_harness apply IN OUT    IN:  u32 width, height, wrap, filter, n, f32 gamma, then width*height x 4 bytes RGBA, then n x 11 f32
//                                     {u, v, sa, ta, sb, tb, sc, tc, e.r, e.g, e.b}
//                                OUT: n x 3 f32 (emap_reference: decode, lookup, apply)
//   emap_harness sample IN OUT   IN:  u32 width, height, wrap, filter, n, then width*height x 4 f32 decoded texels, then n x 12 f32
//                                     {r1, r2, sa, ta, sb, tb, sc, tc, m.emission r, g, b, N_f}
//                                OUT: n x 5 f32 {bu, bv, emission r, g, b} (emap_sample_uv, emap_lookup, emap_sample_emission)
//   emap_harness checks          every host check of rpt_set_mesh_emission_maps, in its order; the plan, the layout, both descriptor tables
//   emap_harness forms           for bits 0 .. 255 (smooth, lights, textured, environment, cutouts, normal_maps, material_maps,
//                                emission_maps from the lowest bit up) one line: "<bits> <mesh_form_ext_of's form> <mesh_form_emit_of's form>"
//   emap_harness compose         the eight emission-mapped forms' arguments over made-up allocation bases, with and without a material
//                                map, mesh lights and an environment: every base field against mesh_map_scene_of<Base>, the zero
//                                block lent exactly when no material map is ON, the map's pointers against its allocation and layout
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_emap.h"
#include "../rust-pathtracer_amd/csrc/mesh_args_emap.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int write_floats(const char* path, const std::vector<float>& out)
{
    FILE* f = fopen(path, "wb");
    REQUIRE(f);
    REQUIRE(out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size());
    fclose(f);
    return 0;
}

static int decode(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t n32;
    float gamma;
    REQUIRE(fread(&n32, 4, 1, f) == 1 && fread(&gamma, 4, 1, f) == 1);
    const size_t n = n32;
    std::vector<uint8_t> bytes(4 * n);                               // exactly the map's bytes: anything outside is the sanitizer's to find
    REQUIRE(n == 0 || fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
    std::vector<TexTexel> texels(n);
    tex_decode_reference(bytes.data(), n, gamma, texels.data());
    std::vector<float> out(4 * n);
    if (n) memcpy(out.data(), texels.data(), 16 * n);
    REQUIRE(write_floats(out_path, out) == 0);
    printf("decode OK\n");
    return 0;
}

static int apply(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[5];
    float gamma;
    REQUIRE(fread(head, 4, 5, f) == 5 && fread(&gamma, 4, 1, f) == 1);
    const uint32_t w = head[0], h = head[1], n = head[4];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    std::vector<uint8_t> bytes(4 * (size_t)w * h);
    REQUIRE(fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
    std::vector<float> in(11 * (size_t)n), out(3 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[11 * i];
        float e[3] = {r[8], r[9], r[10]};
        emap_reference(bytes.data(), w, h, gamma, head[2], head[3], r[0], r[1], r + 2, r + 4, r + 6, e);
        memcpy(&out[3 * i], e, 12);
    }
    REQUIRE(write_floats(out_path, out) == 0);
    printf("apply OK\n");
    return 0;
}

static int sample(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[5];
    REQUIRE(fread(head, 4, 5, f) == 5);
    const uint32_t w = head[0], h = head[1], n = head[4];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    std::vector<TexTexel> texels((size_t)w * h);
    REQUIRE(fread(texels.data(), 16, texels.size(), f) == texels.size());
    std::vector<float> in(12 * (size_t)n), out(5 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    EmapDesc d;
    d.first = 0; d.width = w; d.height = h;
    d.flags = 1u | (head[2] == RPT_TEX_WRAP_CLAMP ? 2u : 0u) | (head[3] == RPT_TEX_FILTER_BILINEAR ? 4u : 0u);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[12 * i];
        float bu, bv, E[3];
        emap_sample_uv(r[0], r[1], bu, bv);
        emap_lookup_desc(d, texels.data(), bu, bv, r + 2, r + 4, r + 6, E);
        out[5 * i] = bu; out[5 * i + 1] = bv;
        emap_sample_emission(r + 8, E, r[11], &out[5 * i + 2]);
    }
    REQUIRE(write_floats(out_path, out) == 0);
    printf("sample OK\n");
    return 0;
}

static int checks()
{
    // three meshes of 4, 0 and 2 vertices; the second has no triangle.  Meshes 0 and 2 are textured (ordinals 0 and 1), mesh 2 CLAMP.
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first = {0u, 4u, 4u, 6u};
    plan.tri_first = {0u, 2u, 2u, 3u};
    plan.mesh_material = {0u, 1u, 2u};
    plan.n_slots = 3;
    TexPlan tex;
    {
        std::vector<TexImage> image(3);
        image[0].width = 3; image[0].height = 5; image[0].wrap = RPT_TEX_WRAP_REPEAT;
        image[2].width = 1; image[2].height = 1; image[2].wrap = RPT_TEX_WRAP_CLAMP;
        build_tex_plan(plan, image, std::vector<float>(), tex);
        REQUIRE(tex.n_tex() == 2 && tex.textured(0) && !tex.textured(1) && tex.textured(2));
    }
    const std::vector<EmapMap> none;
    std::vector<EmapMap> map;
    std::string err;
    const uint8_t px[4] = {1, 2, 3, 4};                              // (never read by the checks: any non-NULL pointer says "set")
    const auto on = [&](uint32_t mesh, uint32_t w, uint32_t h, uint32_t filter = RPT_TEX_FILTER_BILINEAR, float gamma = 1.0f) {
        rpt_mesh_emission_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_EMISSION_MAP_ON; it.width = w; it.height = h; it.texels = px; it.filter = filter; it.gamma = gamma;
        return it;
    };
    const auto off = [&](uint32_t mesh) {
        rpt_mesh_emission_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_EMISSION_MAP_OFF;
        return it;
    };
    const auto run = [&](const rpt_mesh_emission_map* items, uint32_t n, const std::vector<EmapMap>& cur = std::vector<EmapMap>()) {
        return check_mesh_emission_maps(plan, true, tex, items, n, cur, map, err);
    };
    const auto says = [&](const char* what) { return err.find(what) != std::string::npos; };
    const int INVALID = RPT_ERR_INVALID_ARG;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    // no scene comes before everything else, then NULL items
    REQUIRE(check_mesh_emission_maps(plan, false, tex, nullptr, 1, none, map, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_emission_maps: ") == 0);
    REQUIRE(run(nullptr, 1) == INVALID && says("items is NULL") && err.find("rpt_set_mesh_emission_maps: ") == 0);
    REQUIRE(run(nullptr, 0) == RPT_OK && map.size() == 3 && !map[0].width && !map[2].width);
    rpt_mesh_emission_map good[2] = {on(0, 5, 3, RPT_TEX_FILTER_NEAREST, 2.2f), on(2, 33, 7, RPT_TEX_FILTER_BILINEAR, 16.0f)};
    REQUIRE(run(good, 2) == RPT_OK && map[0].width == 5 && map[0].height == 3 && map[0].filter == RPT_TEX_FILTER_NEAREST && map[0].gamma == 2.2f &&
            !map[1].width && map[2].width == 33 && map[2].gamma == 16.0f);
    const std::vector<EmapMap> held = map;
    // per item, in order: the first fault of the first faulty item answers.  Each case carries the NEXT check's fault as well.
    rpt_mesh_emission_map it[2];
    it[0] = on(3, 0, 0); it[0].mode = 7;                             // the mesh before the mode
    REQUIRE(run(it, 1) == INVALID && says("item 0: mesh 3 out of range"));
    it[0] = on(0, 2, 2); it[1] = on(0, 0, 0); it[1].mode = 7;         // named twice before the mode
    REQUIRE(run(it, 2) == INVALID && says("item 1: mesh 0 is named twice"));
    it[0] = on(0, 0, 2); it[0].mode = 2;                             // the mode before the size
    REQUIRE(run(it, 1) == INVALID && says("mode 2"));
    it[0] = on(0, 0, 2); it[0].texels = nullptr;                     // the size before the pointer
    REQUIRE(run(it, 1) == INVALID && says("a map of 0 x 2"));
    it[0] = on(0, 2, 16385); it[0].texels = nullptr;
    REQUIRE(run(it, 1) == INVALID && says("a map of 2 x 16385"));
    it[0] = on(0, 2, 2, 2u); it[0].texels = nullptr;                 // the pointer before the filter
    REQUIRE(run(it, 1) == INVALID && says("texels is NULL"));
    it[0] = on(0, 2, 2, 2u, 0.0f);                                   // the filter before the gamma
    REQUIRE(run(it, 1) == INVALID && says("filter 2"));
    for (const float g : {0.0f, -1.0f, 16.5f, inf, nan}) {           // the gamma before "untextured" (mesh 1 is)
        it[0] = on(1, 2, 2, RPT_TEX_FILTER_NEAREST, g);
        REQUIRE(run(it, 1) == INVALID && says("gamma") && says("finite, above 0 and at most 16"));
    }
    it[0] = off(0); it[0].width = 1; it[0].gamma = nan;               // an OFF item's gamma is not looked at
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_EMISSION_MAP_OFF takes"));
    it[0] = off(0); it[0].texels = px;
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_EMISSION_MAP_OFF takes"));
    it[0] = off(0); it[0].filter = 2u;                               // ... but its filter is, as rpt_set_mesh_material_maps'
    REQUIRE(run(it, 1) == INVALID && says("filter 2"));
    it[0] = on(1, 16384, 16384);                                     // "untextured" before the total
    REQUIRE(run(it, 1) == INVALID && says("mesh 1 is untextured") && says("1 x 1 white texture"));
    it[0] = on(0, 8192, 8192); it[1] = on(2, 1, 1);                   // 2^26 + 1
    REQUIRE(run(it, 2) == RPT_ERR_UNSUPPORTED && says("2^26"));
    it[0] = on(0, 8192, 8192);
    REQUIRE(run(it, 1) == RPT_OK);                                   // exactly 2^26
    REQUIRE(run(it, 1, held) == RPT_ERR_UNSUPPORTED && says("2^26"));     // mesh 2 keeps its 33 x 7
    // a rejected call leaves `map` alone; OFF removes; a mesh not named keeps its map; ON replaces
    map = held;
    it[0] = on(1, 2, 2);
    REQUIRE(run(it, 1, held) == INVALID && map.size() == 3 && map[0].width == 5 && map[2].width == 33);
    it[0] = off(0);
    REQUIRE(run(it, 1, held) == RPT_OK && !map[0].width && map[2].width == 33 && map[2].height == 7 && map[2].gamma == 16.0f);
    it[0] = off(1);                                                  // removing what is not there (even from an untextured mesh) is no error
    REQUIRE(run(it, 1, held) == RPT_OK && map[0].width == 5);
    it[0] = on(0, 2, 9, RPT_TEX_FILTER_BILINEAR, 0.5f);
    REQUIRE(run(it, 1, held) == RPT_OK && map[0].width == 2 && map[0].height == 9 && map[0].gamma == 0.5f && map[2].width == 33);
    // the plan after set, replace and remove; the layout; the descriptors
    EmapPlan ep;
    build_emap_plan(plan, held, ep);
    REQUIRE(ep.any() && ep.on(0) && !ep.on(1) && ep.on(2) && !ep.on(3) && ep.n_meshes == 3 && ep.n_tris == 3);
    REQUIRE(ep.map[0].first == 0 && ep.map[2].first == 15 && ep.n_texels == 15 + 231);
    REQUIRE(!ep.zero.any() && ep.zero.n_meshes == 3 && ep.zero.n_tris == 3 && ep.zero.n_texels == 0);
    const EmapLayout el = ep.layout();
    const MmapLayout zl = ep.zero.layout();
    REQUIRE(zl.off_desc == 0 && zl.off_none == 48 && zl.off_texels == 64 && zl.total == 64);
    REQUIRE(el.off_desc == 0 && el.off_light_desc == 48 && el.off_zero == 96 && el.off_texels == 160 && el.total == 160 + 16 * 246 && sizeof(EmapDesc) == 16);
    REQUIRE(el.zero.off_none == zl.off_none && el.zero.total == zl.total);
    const std::vector<uint32_t> d = emap_desc_table(ep, tex);
    const std::vector<uint32_t> want = {0u, 5u, 3u, 1u, 15u, 33u, 7u, 7u, 0u, 0u, 0u, 0u};      // by texture ordinal; mesh 2 is CLAMP and BILINEAR
    REQUIRE(d == want);
    {                                                                // by light ordinal: mesh 2 ON alone, then meshes 1 and 2, then 0 and 2
        LightPlan lp;
        REQUIRE(emap_light_desc_table(ep, tex, lp) == std::vector<uint32_t>(12, 0u));
        lp.on_mesh = {2u};
        const std::vector<uint32_t> w1 = {15u, 33u, 7u, 7u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        REQUIRE(emap_light_desc_table(ep, tex, lp) == w1);
        lp.on_mesh = {1u, 2u};
        const std::vector<uint32_t> w2 = {0u, 0u, 0u, 0u, 15u, 33u, 7u, 7u, 0u, 0u, 0u, 0u};
        REQUIRE(emap_light_desc_table(ep, tex, lp) == w2);
        lp.on_mesh = {0u, 2u};
        REQUIRE(emap_light_desc_table(ep, tex, lp) == want);
    }
    {
        EmapPlan replaced;                                           // mesh 0 replaced by 2 x 9: mesh 2's texels move down
        build_emap_plan(plan, map, replaced);
        REQUIRE(replaced.map[0].first == 0 && replaced.map[2].first == 18 && replaced.n_texels == 18 + 231);
        std::vector<EmapMap> only2 = held;
        only2[0] = EmapMap();
        EmapPlan removed;
        build_emap_plan(plan, only2, removed);
        REQUIRE(removed.any() && !removed.on(0) && removed.map[2].first == 0 && removed.n_texels == 231 && removed.layout().total == 160 + 16 * 231);
    }
    {                                                                // mesh 1 textured as well, all CLAMP: ordinals move, texels do not
        std::vector<TexImage> image(3);
        for (TexImage& im : image) { im.width = 2; im.height = 2; im.wrap = RPT_TEX_WRAP_CLAMP; }
        TexPlan t3;
        build_tex_plan(plan, image, std::vector<float>(), t3);
        const std::vector<uint32_t> want3 = {0u, 5u, 3u, 3u, 0u, 0u, 0u, 0u, 15u, 33u, 7u, 7u};
        REQUIRE(emap_desc_table(ep, t3) == want3);
    }
    EmapPlan empty;
    build_emap_plan(plan, none, empty);
    REQUIRE(!empty.any() && empty.n_texels == 0 && empty.map.size() == 3);
    printf("checks OK\n");
    return 0;
}

// ---- the composer --------------------------------------------------------------------------------------------------------------------
using namespace rptargs;
constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3;

template <class S> static int compose_one(const MeshView& v, const MmapView& m, bool material_maps, const EmapView& e, const char* name)
{
    using Base = typename emit_base_of<S>::type;
    static_assert(sizeof(S) == sizeof(Base) + 24, "the map's part is three pointers");
    const S s = mesh_emit_scene_of<S>(v, m, material_maps, e);
    const EmapLayout el = e.emap_plan.layout();
    unsigned char* base = static_cast<unsigned char*>(e.emap);
    // what the base would be bound with: the device's material maps while one is ON, else the zero block in the emission maps' allocation
    const MmapView lent{base + el.off_zero, e.emap_plan.zero};
    const Base want = mesh_map_scene_of<Base>(v, material_maps ? m : lent);
    REQUIRE(memcmp(static_cast<const Base*>(&s), &want, sizeof(Base)) == 0);              // every base field, padding included (S s{} zeroes it)
    const unsigned char* desc = reinterpret_cast<const unsigned char*>(s.map_desc);
    const bool zero = desc == base + el.off_zero;
    REQUIRE(zero == !material_maps);
    if (!zero) REQUIRE(desc == static_cast<const unsigned char*>(m.mmap));
    else REQUIRE(reinterpret_cast<const unsigned char*>(s.map_texels) == base + el.off_zero + el.zero.total && el.off_zero + el.zero.total <= el.off_texels);
    REQUIRE(reinterpret_cast<const unsigned char*>(s.emit_desc) == base + el.off_desc);
    REQUIRE(reinterpret_cast<const unsigned char*>(s.emit_light_desc) == base + el.off_light_desc);
    REQUIRE(reinterpret_cast<const unsigned char*>(s.emit_texels) == base + el.off_texels);
    REQUIRE(el.off_desc + 16u * e.emap_plan.n_meshes <= el.off_light_desc && el.off_light_desc + 16u * e.emap_plan.n_meshes <= el.off_zero);
    REQUIRE(el.off_texels + 16u * e.emap_plan.n_texels == el.total);
    REQUIRE(s.tri_light != nullptr && s.tri_tex != nullptr && s.smooth_bits != nullptr);
    printf("%s %s\n", name, zero ? "zero" : "own");
    return 0;
}

static int compose()
{
    for (int maps = 0; maps < 2; ++maps) for (int lights = 0; lights < 2; ++lights) for (int env = 0; env < 3; ++env) {
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        RefitPlan rp; SmoothPlan sp; LightPlan lp; TexPlan tp; EnvPlan ep; CutPlan cp; NrmPlan np; MmapPlan mp;
        rp.mesh_first = {0, 5, kVertices}; rp.tri_first = {0, 20, kTris}; rp.n_slots = kTris;
        void* const refit = (void*)(1ull << 40);
        void *light_a = nullptr, *env_a = nullptr, *mmap_a = nullptr;
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4;
        void* const tex_a = (void*)(4ull << 40);
        if (env) { ep.size = 4; ep.mode = env == 2 ? RPT_ENV_SAMPLED : RPT_ENV_BACKGROUND_ONLY; ep.scale = 1.5f; ep.n_tris = kTris; ep.q_total = env == 2 ? 12345u : 0u; env_a = (void*)(5ull << 40); }
        cp.mask.resize(2); cp.mask[0].width = cp.mask[0].height = 3; cp.n_meshes = 2; cp.n_tris = kTris; cp.n_words = 1;
        void* const cut_a = (void*)(6ull << 40);
        np.map.resize(2); np.map[0].width = np.map[0].height = 3; np.n_meshes = 2; np.n_tris = kTris; np.n_texels = 9;
        void* const nrm_a = (void*)(7ull << 40);
        if (maps) { mp.map.resize(2); mp.map[0].width = 3; mp.map[0].height = 5; mp.n_meshes = 2; mp.n_tris = kTris; mp.n_texels = 15; mmap_a = (void*)(8ull << 40); }
        EmapPlan emp;
        {
            std::vector<EmapMap> em(2);
            em[0].width = 4; em[0].height = 6;
            build_emap_plan(rp, em, emp);
        }
        void* const emap_a = (void*)(9ull << 40);
        const MmapView m{mmap_a, mp};
        const EmapView e{emap_a, emp};
        const bool material_maps = mmap_a && mp.any();
        const MeshView plain{scene, refit, nullptr, light_a, tex_a, nullptr, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_env{scene, refit, nullptr, light_a, tex_a, env_a, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_cut{scene, refit, nullptr, light_a, tex_a, env_a, cut_a, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_nrm{scene, refit, nullptr, light_a, tex_a, env_a, nullptr, nrm_a, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_all{scene, refit, nullptr, light_a, tex_a, env_a, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};
        printf("maps %d lights %d env %d\n", maps, lights, env);
        if (!env) {
            REQUIRE(compose_one<SceneMeshEmit>(plain, m, material_maps, e, "light_tex") == 0);
            REQUIRE(compose_one<SceneMeshEmitCut>(with_cut, m, material_maps, e, "cut") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrm>(with_nrm, m, material_maps, e, "nrm") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrmCut>(with_all, m, material_maps, e, "nrm_cut") == 0);
        } else {
            REQUIRE(compose_one<SceneMeshEmitEnv>(with_env, m, material_maps, e, "env") == 0);
            REQUIRE(compose_one<SceneMeshEmitCutEnv>(with_cut, m, material_maps, e, "cut_env") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrmEnv>(with_nrm, m, material_maps, e, "nrm_env") == 0);
            REQUIRE(compose_one<SceneMeshEmitNrmCutEnv>(with_all, m, material_maps, e, "nrm_cut_env") == 0);
        }
    }
    printf("compose OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "apply")) return apply(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "sample")) return sample(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    if (argc == 2 && !strcmp(argv[1], "forms")) {
        for (unsigned b = 0; b < 256; ++b)
            printf("%u %u %u\n", b, mesh_form_ext_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64),
                   mesh_form_emit_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64, b & 128));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "compose")) return compose();
    fprintf(stderr, "usage: emap_harness decode IN OUT | apply IN OUT | sample IN OUT | checks | forms | compose\n");
    return 2;
}
