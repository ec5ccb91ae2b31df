// mmap_harness.cpp — csrc/host_mmap.h and csrc/mesh_args_mmap.h on the host (tests/test_mesh_material_map_host.py); a stand-alone
// program, so it may be built with -fsanitize=address,undefined and run as it is.
//
//   mmap_harness decode IN OUT   IN:  u32 n_texels, roughness_channel, metallic_channel, then n_texels x 4 bytes RGBA
//                                OUT: n_texels x 4 f32 (mmap_decode_reference)
//   mmap_harness factors IN OUT  IN:  u32 width, height, wrap, filter, n, then width*height x 4 f32 decoded texels, then n x 10 f32
//                                     {u, v, sa, ta, sb, tb, sc, tc, roughness, metallic}
//                                OUT: n x 2 f32 (mmap_factors, then mmap_apply)
//   mmap_harness bilinear        tex_lookup BILINEAR over every 2 x 2 image of the decoded bytes (a, b) and 65 weights: prints
//                                "above_one N", "below_zero N", "constant_inexact N", "constant_inexact_0_255 N", "taps N"
//   mmap_harness checks          every host check of rpt_set_mesh_material_maps, in its order; the plan, the layout, the descriptors
//   mmap_harness forms           for bits 0 .. 127 (smooth, lights, textured, environment, cutouts, normal_maps, material_maps from the
//                                lowest bit up) one line: "<bits> <mesh_form_of's form> <mesh_form_ext_of's form>"
//   mmap_harness compose         the eight material-mapped forms' arguments over made-up allocation bases, with and without mesh
//                                lights and in both environment modes: every base field against mesh_scene_of<Base>, the map's
//                                pointers against its allocation and layout
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_mmap.h"
#include "../rust-pathtracer_amd/csrc/mesh_args_mmap.h"

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
    uint32_t head[3];
    REQUIRE(fread(head, 4, 3, f) == 3);
    const size_t n = head[0];
    std::vector<uint8_t> bytes(4 * n);                               // exactly the map's bytes: anything outside is the sanitizer's to find
    REQUIRE(n == 0 || fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
    std::vector<TexTexel> texels(n);
    mmap_decode_reference(bytes.data(), n, head[1], head[2], texels.data());
    std::vector<float> out(4 * n);
    if (n) memcpy(out.data(), texels.data(), 16 * n);
    REQUIRE(write_floats(out_path, out) == 0);
    printf("decode OK\n");
    return 0;
}

static int factors(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[5];
    REQUIRE(fread(head, 4, 5, f) == 5);
    const uint32_t w = head[0], h = head[1], n = head[4];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    std::vector<TexTexel> texels((size_t)w * h);
    REQUIRE(fread(texels.data(), 16, texels.size(), f) == texels.size());
    std::vector<float> in(10 * (size_t)n), out(2 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[10 * i];
        float fac[2];
        mmap_factors(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], texels.data(), w, h, head[2], head[3], fac);
        out[2 * i] = r[8]; out[2 * i + 1] = r[9];
        mmap_apply(out[2 * i], out[2 * i + 1], fac);
    }
    REQUIRE(write_floats(out_path, out) == 0);
    printf("factors OK\n");
    return 0;
}

// The two questions of include/rpt.h, "lookup at the hit", over tex_lookup itself: the 2 x 2 CLAMP image {c(a), c(b); c(b), c(a)} (its
// second channel the other way round) looked up at s = t = (0.5 + w) / 2 blends its texels with a weight near w along x, then the
// two rows with the same weight along y, so both blends of the statement run on unequal operands.  The 65 weights (i + 0.37) / 65
// are no short dyadic fractions: the weight that reaches the blend has as many bits as tex_bilinear_taps can give it.  (It prints how
// often 1 - f was rounded: never, include/rpt.h says why.)
static int bilinear()
{
    uint64_t above = 0, below = 0, inexact = 0, inexact_ends = 0, taps = 0, rounded_complements = 0;
    float c[256];
    for (uint32_t k = 0; k < 256u; ++k) c[k] = mmap_decode_value(k);
    REQUIRE(c[0] == 0.0f && c[255] == 1.0f);
    float st[65];
    for (uint32_t i = 0; i < 65u; ++i) {
        st[i] = (0.5f + ((float)i + 0.37f) / 65.0f) / 2.0f;
        uint32_t i0, i1;
        float f;
        tex_bilinear_taps(tex_wrap(st[i], RPT_TEX_WRAP_CLAMP), 2u, RPT_TEX_WRAP_CLAMP, i0, i1, f);
        REQUIRE(i0 == 0u && i1 == 1u && f > 0.0f && f < 1.0f);       // two different texels and a weight strictly inside
        if ((double)(1.0f - f) != 1.0 - (double)f) ++rounded_complements;
    }
    for (uint32_t a = 0; a < 256u; ++a) for (uint32_t b = 0; b < 256u; ++b) {
        const TexTexel A{c[a], c[b], 0.0f, 0.0f}, B{c[b], c[a], 0.0f, 0.0f};
        const TexTexel im[4] = {A, B, B, A};
        for (uint32_t i = 0; i < 65u; ++i) {
            float out[3];
            tex_lookup(im, 2u, 2u, RPT_TEX_WRAP_CLAMP, RPT_TEX_FILTER_BILINEAR, st[i], st[i], out);
            for (int ch = 0; ch < 2; ++ch) {
                ++taps;
                if (!(out[ch] <= 1.0f)) ++above;
                if (!(out[ch] >= 0.0f)) ++below;
            }
            if (a == b && out[0] != c[a]) { ++inexact; if (a == 0u || a == 255u) ++inexact_ends; }
        }
    }
    printf("above_one %llu\nbelow_zero %llu\nconstant_inexact %llu\nconstant_inexact_0_255 %llu\ntaps %llu\nrounded_complements %llu\n",
           (unsigned long long)above, (unsigned long long)below, (unsigned long long)inexact, (unsigned long long)inexact_ends, (unsigned long long)taps,
           (unsigned long long)rounded_complements);
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
    const uint32_t NONE = RPT_MATERIAL_MAP_CHANNEL_NONE;
    const std::vector<MmapMap> none;
    std::vector<MmapMap> map;
    std::string err;
    const uint8_t px[4] = {1, 2, 3, 4};                              // (never read by the checks: any non-NULL pointer says "set")
    const auto on = [&](uint32_t mesh, uint32_t w, uint32_t h, uint32_t filter = RPT_TEX_FILTER_BILINEAR, uint32_t rc = 1u, uint32_t mc = 2u) {
        rpt_mesh_material_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_MATERIAL_MAP_ON; it.width = w; it.height = h; it.texels = px; it.filter = filter;
        it.roughness_channel = rc; it.metallic_channel = mc;
        return it;
    };
    const auto off = [&](uint32_t mesh) {
        rpt_mesh_material_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_MATERIAL_MAP_OFF; it.roughness_channel = it.metallic_channel = NONE;
        return it;
    };
    const auto run = [&](const rpt_mesh_material_map* items, uint32_t n, const std::vector<MmapMap>& cur = std::vector<MmapMap>()) {
        return check_mesh_material_maps(plan, true, tex, items, n, cur, map, err);
    };
    const auto says = [&](const char* what) { return err.find(what) != std::string::npos; };
    const int INVALID = RPT_ERR_INVALID_ARG;
    // no scene comes before everything else, then NULL items
    REQUIRE(check_mesh_material_maps(plan, false, tex, nullptr, 1, none, map, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_material_maps: ") == 0);
    REQUIRE(run(nullptr, 1) == INVALID && says("items is NULL") && err.find("rpt_set_mesh_material_maps: ") == 0);
    REQUIRE(run(nullptr, 0) == RPT_OK && map.size() == 3 && !map[0].width && !map[2].width);
    rpt_mesh_material_map good[2] = {on(0, 5, 3, RPT_TEX_FILTER_NEAREST, 0u, NONE), on(2, 33, 7, RPT_TEX_FILTER_BILINEAR, 3u, 3u)};
    REQUIRE(run(good, 2) == RPT_OK && map[0].width == 5 && map[0].height == 3 && map[0].filter == RPT_TEX_FILTER_NEAREST && map[0].roughness_channel == 0u &&
            map[0].metallic_channel == NONE && !map[1].width && map[2].width == 33 && map[2].roughness_channel == 3u && map[2].metallic_channel == 3u);
    const std::vector<MmapMap> held = map;
    // per item, in order: the first fault of the first faulty item answers.  Each case carries the NEXT check's fault as well.
    rpt_mesh_material_map it[2];
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
    it[0] = on(0, 2, 2, 2u, 4u);                                     // the filter before the channels
    REQUIRE(run(it, 1) == INVALID && says("filter 2"));
    it[0] = on(1, 2, 2, RPT_TEX_FILTER_NEAREST, 4u, NONE);           // a channel before "both NONE" and before "untextured" (mesh 1 is)
    REQUIRE(run(it, 1) == INVALID && says("channels 4 and"));
    it[0] = on(1, 2, 2, RPT_TEX_FILTER_NEAREST, NONE, 0xFFFFFFFEu);
    REQUIRE(run(it, 1) == INVALID && says("channels"));
    it[0] = off(0); it[0].width = 1; it[0].metallic_channel = 9u;     // an OFF item's channels are checked before its size
    REQUIRE(run(it, 1) == INVALID && says("channels"));
    it[0] = on(1, 2, 2, RPT_TEX_FILTER_NEAREST, NONE, NONE);         // both NONE before "untextured"
    REQUIRE(run(it, 1) == INVALID && says("both channels are RPT_MATERIAL_MAP_CHANNEL_NONE"));
    it[0] = off(0); it[0].width = 1;                                 // (an OFF item may say NONE twice: that is its natural form)
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_MATERIAL_MAP_OFF takes"));
    it[0] = off(0); it[0].texels = px;
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_MATERIAL_MAP_OFF takes"));
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
    REQUIRE(run(it, 1, held) == RPT_OK && !map[0].width && map[2].width == 33 && map[2].height == 7 && map[2].roughness_channel == 3u);
    it[0] = off(1);                                                  // removing what is not there (even from an untextured mesh) is no error
    REQUIRE(run(it, 1, held) == RPT_OK && map[0].width == 5);
    it[0] = on(0, 2, 9, RPT_TEX_FILTER_BILINEAR, NONE, 2u);
    REQUIRE(run(it, 1, held) == RPT_OK && map[0].width == 2 && map[0].height == 9 && map[0].roughness_channel == NONE && map[0].metallic_channel == 2u && map[2].width == 33);
    // the plan after set, replace and remove; the layout; the descriptors
    MmapPlan mp;
    build_mmap_plan(plan, held, mp);
    REQUIRE(mp.any() && mp.on(0) && !mp.on(1) && mp.on(2) && !mp.on(3) && mp.n_meshes == 3 && mp.n_tris == 3);
    REQUIRE(mp.map[0].first == 0 && mp.map[2].first == 15 && mp.n_texels == 15 + 231);
    const MmapLayout ml = mp.layout();
    REQUIRE(ml.off_desc == 0 && ml.off_none == 48 && ml.off_texels == 64 && ml.total == 64 + 16 * 246 && sizeof(MmapDesc) == 16 && sizeof(TexTexel) == 16);
    const std::vector<uint32_t> d = mmap_desc_table(mp, tex);
    const std::vector<uint32_t> want = {0u, 5u, 3u, 1u, 15u, 33u, 7u, 7u, 0u, 0u, 0u, 0u};      // by texture ordinal; mesh 2 is CLAMP and BILINEAR
    REQUIRE(d == want);
    {
        MmapPlan replaced;                                           // mesh 0 replaced by 2 x 9: mesh 2's texels move down
        build_mmap_plan(plan, map, replaced);
        REQUIRE(replaced.map[0].first == 0 && replaced.map[2].first == 18 && replaced.n_texels == 18 + 231);
        std::vector<MmapMap> only2 = held;
        only2[0] = MmapMap();
        MmapPlan removed;
        build_mmap_plan(plan, only2, removed);
        REQUIRE(removed.any() && !removed.on(0) && removed.map[2].first == 0 && removed.n_texels == 231 && removed.layout().total == 64 + 16 * 231);
    }
    {                                                                // mesh 1 textured as well, all CLAMP: ordinals move, texels do not
        std::vector<TexImage> image(3);
        for (TexImage& im : image) { im.width = 2; im.height = 2; im.wrap = RPT_TEX_WRAP_CLAMP; }
        TexPlan t3;
        build_tex_plan(plan, image, std::vector<float>(), t3);
        const std::vector<uint32_t> d3 = mmap_desc_table(mp, t3);
        const std::vector<uint32_t> want3 = {0u, 5u, 3u, 3u, 0u, 0u, 0u, 0u, 15u, 33u, 7u, 7u};
        REQUIRE(d3 == want3);
    }
    MmapPlan empty;
    build_mmap_plan(plan, none, empty);
    REQUIRE(!empty.any() && empty.n_texels == 0 && empty.map.size() == 3);
    // the decode's stated exact values
    REQUIRE(mmap_decode_value(0) == 0.0f && mmap_decode_value(255) == 1.0f && mmap_decode_channel(0x01020304u, NONE) == 1.0f);
    printf("checks OK\n");
    return 0;
}

// ---- the composer --------------------------------------------------------------------------------------------------------------------
using namespace rptargs;
constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3;

template <class S> static int compose_one(const MeshView& v, const MmapView& m, const char* name, bool expect_lent)
{
    using Base = typename map_base_of<S>::type;
    static_assert(sizeof(S) == sizeof(Base) + 16, "the map's part is two pointers");
    const S s = mesh_map_scene_of<S>(v, m);
    Base want = mesh_scene_of<Base>(v);
    const MmapLayout ml = m.mmap_plan.layout();
    const unsigned char* base = static_cast<const unsigned char*>(m.mmap);
    const bool lent = want.tri_light == nullptr;
    REQUIRE(lent == expect_lent);
    if (lent) want.tri_light = reinterpret_cast<const uint32_t*>(base + ml.off_none);      // the one table the map's allocation lends
    REQUIRE(memcmp(static_cast<const Base*>(&s), &want, sizeof(Base)) == 0);              // every base field, padding included (S s{} zeroes it)
    REQUIRE(reinterpret_cast<const unsigned char*>(s.map_desc) == base + ml.off_desc);
    REQUIRE(reinterpret_cast<const unsigned char*>(s.map_texels) == base + ml.off_texels);
    REQUIRE(ml.off_desc < ml.off_none && ml.off_none + 4u * kTris <= ml.off_texels && ml.off_texels + 16u * m.mmap_plan.n_texels == ml.total);
    REQUIRE(s.tri_light != nullptr && s.tri_tex != nullptr && s.smooth_bits != nullptr);
    printf("%s %s\n", name, lent ? "lent" : "own");
    return 0;
}

static int compose()
{
    for (int lights = 0; lights < 2; ++lights) for (int env = 0; env < 3; ++env) for (int smooth = 0; smooth < 2; ++smooth) {
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        RefitPlan rp; SmoothPlan sp; LightPlan lp; TexPlan tp; EnvPlan ep; CutPlan cp; NrmPlan np; MmapPlan mp;
        rp.mesh_first = {0, 5, kVertices}; rp.n_slots = kTris;
        void* const refit = (void*)(1ull << 40);
        void *smooth_a = nullptr, *light_a = nullptr, *env_a = nullptr;
        if (smooth) { sp.mode = {RPT_MESH_SHADING_SMOOTH, RPT_MESH_SHADING_FLAT}; sp.n_vertices = kVertices; sp.n_tris = kTris; sp.n_faces = 20; sp.n_adj = 60; smooth_a = (void*)(2ull << 40); }
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4;
        void* const tex_a = (void*)(4ull << 40);
        if (env) { ep.size = 4; ep.mode = env == 2 ? RPT_ENV_SAMPLED : RPT_ENV_BACKGROUND_ONLY; ep.scale = 1.5f; ep.n_tris = kTris; ep.q_total = env == 2 ? 12345u : 0u; env_a = (void*)(5ull << 40); }
        cp.mask.resize(2); cp.mask[0].width = cp.mask[0].height = 3; cp.n_meshes = 2; cp.n_tris = kTris; cp.n_words = 1;
        void* const cut_a = (void*)(6ull << 40);
        np.map.resize(2); np.map[0].width = np.map[0].height = 3; np.n_meshes = 2; np.n_tris = kTris; np.n_texels = 9;
        void* const nrm_a = (void*)(7ull << 40);
        mp.map.resize(2); mp.map[0].width = 3; mp.map[0].height = 5; mp.n_meshes = 2; mp.n_tris = kTris; mp.n_texels = 15;
        void* const mmap_a = (void*)(8ull << 40);
        const MmapView m{mmap_a, mp};
        // each form over a view that holds exactly the allocations its base form is taken with
        const MeshView plain{scene, refit, smooth_a, light_a, tex_a, nullptr, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_env{scene, refit, smooth_a, light_a, tex_a, env_a, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_cut{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_nrm{scene, refit, smooth_a, light_a, tex_a, env_a, nullptr, nrm_a, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_all{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};
        printf("lights %d env %d smooth %d\n", lights, env, smooth);
        if (!env) {
            REQUIRE(compose_one<SceneMeshMap>(plain, m, "light_tex", !lights) == 0);       // the only base with no part to borrow from
            REQUIRE(compose_one<SceneMeshMapCut>(with_cut, m, "cut", false) == 0);
            REQUIRE(compose_one<SceneMeshMapNrm>(with_nrm, m, "nrm", false) == 0);
            REQUIRE(compose_one<SceneMeshMapNrmCut>(with_all, m, "nrm_cut", false) == 0);
        } else {
            REQUIRE(compose_one<SceneMeshMapEnv>(with_env, m, "env", false) == 0);
            REQUIRE(compose_one<SceneMeshMapCutEnv>(with_cut, m, "cut_env", false) == 0);
            REQUIRE(compose_one<SceneMeshMapNrmEnv>(with_nrm, m, "nrm_env", false) == 0);
            REQUIRE(compose_one<SceneMeshMapNrmCutEnv>(with_all, m, "nrm_cut_env", false) == 0);
        }
    }
    printf("compose OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "factors")) return factors(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "bilinear")) return bilinear();
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    if (argc == 2 && !strcmp(argv[1], "forms")) {
        for (unsigned b = 0; b < 128; ++b)
            printf("%u %u %u\n", b, (unsigned)mesh_form_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32), mesh_form_ext_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "compose")) return compose();
    fprintf(stderr, "usage: mmap_harness decode IN OUT | factors IN OUT | bilinear | checks | forms | compose\n");
    return 2;
}
