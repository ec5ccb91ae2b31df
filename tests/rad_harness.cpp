// rad_harness.cpp — csrc/host_rad.h and csrc/mesh_args_rad.h on the host (tests/test_radiance_f64.py); a stand-alone program, so it
// may be built with -fsanitize=address,undefined and run as it is.
//
//   rad_harness forms     rad_form_of over the eight combinations, and the cut of a call's samples into launches: every sample in
//                         exactly one launch, in order, no launch above the limit, for sample counts around its multiples
//   rad_harness compose   the radiance forms' arguments over a radiance allocation that is real host memory, filled as capi.hip fills
//                         the device's (so the sanitizer sees every read of a lent table), and made-up bases for the others: with and
//                         without media, emission maps, material maps, textures, mesh lights and smooth meshes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_rad.h"
#include "../rust-pathtracer_amd/csrc/mesh_args_rad.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int forms()
{
    uint32_t seen = 0;
    for (int bits = 0; bits < 8; ++bits) {
        const bool nrm = bits & 4, cut = bits & 2, env = bits & 1;
        const uint32_t f = rad_form_of(nrm, cut, env);
        REQUIRE(f < kRadForms && ((f & kRadNrm) != 0) == nrm && ((f & kRadCut) != 0) == cut && ((f & kRadEnv) != 0) == env);
        seen |= 1u << f;
    }
    REQUIRE(seen == 0xFFu);
    uint32_t checked = 0;
    for (uint32_t max_spp : {1u, 7u, 96u, 512u})
        for (uint32_t spp : {0u, 1u, max_spp - 1u, max_spp, max_spp + 1u, max_spp + 3u, 2u * max_spp, 2u * max_spp + 1u, 5u * max_spp - 1u, 0xFFFFFFFFu / 64u}) {
            const uint32_t launches = rad_launches(spp, max_spp);
            REQUIRE((spp == 0) == (launches == 0));
            uint64_t next = 0;
            for (uint32_t k = 0; k < launches; ++k) {
                const uint32_t n = rad_launch_spp(spp, max_spp, k);
                REQUIRE(n >= 1u && n <= max_spp && (uint64_t)k * max_spp == next);
                REQUIRE(k + 1u == launches || n == max_spp);         // only the last launch is short
                next += n;
            }
            REQUIRE(next == spp);
            checked += 1;
        }
    printf("forms OK %u\n", checked);
    return 0;
}

// ---- the composer --------------------------------------------------------------------------------------------------------------------
using namespace rptargs;
constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3, kMeshes = 2;

// the radiance allocation as capi.hip's ensure_rad fills the device's
static std::vector<unsigned char> rad_allocation(const MedPlan& plan)
{
    const MedLayout ml = plan.layout();
    std::vector<unsigned char> a(ml.total, 0);
    for (const RadFill& f : rad_fills(ml)) memset(a.data() + f.off, f.value, f.bytes);
    if (!plan.tri_medium.empty()) memcpy(a.data() + ml.off_tri_medium, plan.tri_medium.data(), 4u * plan.tri_medium.size());
    return a;
}

template <class S> static int compose_one(const MeshView& v, const MmapView& m, bool material_maps, const EmapView& e, bool emission_maps, const MedView& meds, bool media,
                                          const RadView& rv, const char* name)
{
    const S s = mesh_rad_scene_of<S>(v, m, material_maps, e, emission_maps, meds, media, rv);
    // with media it is the media form's own argument, field for field (padding included: S s{} zeroes it)
    if (media) {
        const S want = mesh_med_scene_of<S>(v, m, material_maps, e, emission_maps, meds);
        REQUIRE(memcmp(&s, &want, sizeof(S)) == 0);
        REQUIRE(reinterpret_cast<const unsigned char*>(s.tri_medium) >= static_cast<const unsigned char*>(meds.med));
    } else {
        // without: the media part and every absent feature come from the radiance allocation — real memory, read here
        unsigned char* base = static_cast<unsigned char*>(rv.rad);
        const MedLayout ml = rv.rad_plan.layout();
        const unsigned char* p = reinterpret_cast<const unsigned char*>(s.tri_medium);
        REQUIRE(p == base + ml.off_tri_medium);
        for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_medium[k] == kMedNone);
        if (!emission_maps) for (uint32_t j = 0; j < kMeshes; ++j) REQUIRE(s.emit_desc[j].flags == 0u && s.emit_light_desc[j].flags == 0u);
        if (!material_maps && !emission_maps) for (uint32_t j = 0; j < kMeshes; ++j) REQUIRE(s.map_desc[j].flags == 0u);
        if (!v.has_smooth()) for (uint32_t w = 0; w < (kTris + 31) / 32; ++w) REQUIRE(s.smooth_bits[w] == 0u);
        if (!v.has_lights()) { for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_light[k] == kLightNone); REQUIRE(s.n_pick >= s.n_lights); }
        if (!v.has_tex()) for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_tex[k] == kTexNone);
    }
    REQUIRE(s.tri_light != nullptr && s.tri_tex != nullptr && s.smooth_bits != nullptr && s.map_desc != nullptr && s.emit_desc != nullptr && s.tri_medium != nullptr);
    REQUIRE(s.n_tris == kTris && s.n_lights == kSceneLights);
    printf("%s media %s emap %s mmap %s tex %s lights %s smooth %s\n", name, media ? "own" : "lent", emission_maps ? "own" : "lent", material_maps ? "own" : "lent",
           v.has_tex() ? "own" : "lent", v.has_lights() ? "own" : "lent", v.has_smooth() ? "own" : "lent");
    return 0;
}

static int compose()
{
    for (int bits = 0; bits < 64; ++bits) {
        const bool emaps = bits & 1, maps = bits & 2, lights = bits & 4, tex = bits & 8, smooth = bits & 16, media = bits & 32;
        if ((emaps || maps) && !tex) continue;                       // a map needs a texture
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        RefitPlan rp; SmoothPlan sp; LightPlan lp; TexPlan tp; EnvPlan ep; CutPlan cp; NrmPlan np; MmapPlan mp; EmapPlan emp; MedPlan medp, radp;
        rp.ok = true; rp.mesh_first = {0, 5, kVertices}; rp.tri_first = {0, 20, kTris}; rp.n_slots = kTris; rp.mesh_material = {0, 1};
        void* const refit = (void*)(1ull << 40);
        void *smooth_a = nullptr, *light_a = nullptr, *tex_a = nullptr, *mmap_a = nullptr, *emap_a = nullptr, *med_a = nullptr;
        if (smooth) { sp.mode = {1, 0}; sp.n_tris = kTris; smooth_a = (void*)(2ull << 40); }
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        if (tex) { tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4; tex_a = (void*)(4ull << 40); }
        ep.size = 4;
        void* const env_a = (void*)(5ull << 40);
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
        if (media) {
            std::vector<MedEntry> md(2);
            md[1].type = RPT_MEDIUM_SCATTER; md[1].density = 2.0f;
            build_med_plan(rp, md, medp);
            med_a = (void*)(10ull << 40);
        }
        build_rad_plan(rp, radp);
        REQUIRE(!radp.any() && radp.n_media() == 0u && radp.n_tris == kTris && radp.tri_medium.size() == kTris);
        std::vector<unsigned char> rad_mem = rad_allocation(radp);
        const MmapView m{mmap_a, mp};
        const EmapView e{emap_a, emp};
        const MedView meds{med_a, medp};
        const RadView rv{rad_mem.data(), radp};
        const bool material_maps = mmap_a && mp.any(), emission_maps = emap_a && emp.any(), has_media = med_a && medp.any();
        REQUIRE(material_maps == maps && emission_maps == emaps && has_media == media);
        // (the environment, cutout and normal-map forms are only taken while those features are present; the last two need a texture)
        const MeshView plain{scene, refit, smooth_a, light_a, tex_a, nullptr, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_env{scene, refit, smooth_a, light_a, tex_a, env_a, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_cut{scene, refit, smooth_a, light_a, tex_a, nullptr, cut_a, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_nrm{scene, refit, smooth_a, light_a, tex_a, nullptr, nullptr, nrm_a, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_all{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};
        printf("bits %d\n", bits);
        REQUIRE(compose_one<SceneMeshMed>(plain, m, material_maps, e, emission_maps, meds, has_media, rv, "radiance") == 0);
        REQUIRE(compose_one<SceneMeshMedEnv>(with_env, m, material_maps, e, emission_maps, meds, has_media, rv, "radiance_env") == 0);
        if (tex) {
            REQUIRE(compose_one<SceneMeshMedCut>(with_cut, m, material_maps, e, emission_maps, meds, has_media, rv, "radiance_cut") == 0);
            REQUIRE(compose_one<SceneMeshMedNrm>(with_nrm, m, material_maps, e, emission_maps, meds, has_media, rv, "radiance_nrm") == 0);
            REQUIRE(compose_one<SceneMeshMedNrmCutEnv>(with_all, m, material_maps, e, emission_maps, meds, has_media, rv, "radiance_nrm_cut_env") == 0);
        }
    }
    printf("compose OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "forms")) return forms();
    if (argc == 2 && !strcmp(argv[1], "compose")) return compose();
    fprintf(stderr, "usage: rad_harness forms | compose\n");
    return 2;
}
