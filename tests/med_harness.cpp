// med_harness.cpp — csrc/host_med.h and csrc/mesh_args_med.h on the host (tests/test_mesh_media_host.py); a stand-alone program, so
// it may be built with -fsanitize=address,undefined and run as it is.
//
//   med_harness checks    every host check of rpt_set_mesh_media, in its order, each printed as "<code> <message>"; the clamp; that a
//                         rejected call leaves the table as it was; the plan, the rows and tri_medium of a three-mesh scene whose
//                         middle mesh carries the medium; the layout
//   med_harness forms     for bits 0 .. 511 (smooth, lights, textured, environment, cutouts, normal_maps, material_maps,
//                         emission_maps, media from the lowest bit up) one line: "<bits> <mesh_form_emit_of's form> <mesh_form_med_of's form>"
//   med_harness compose   the eight media forms' arguments over a media allocation that is real host memory, filled as capi.hip fills
//                         the device's (so the sanitizer sees every read of a lent table), and made-up bases for the others: with and
//                         without emission maps, material maps, textures, mesh lights, smooth meshes and an environment
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_med.h"
#include "../rust-pathtracer_amd/csrc/mesh_args_med.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static rpt_mesh_medium item(uint32_t mesh, uint32_t type, float density = 1.0f, float r = 0.5f, float g = 0.25f, float b = 0.125f, float aniso = 0.0f)
{
    rpt_mesh_medium it;
    memset(&it, 0, sizeof(it));
    it.mesh = mesh; it.medium_type = type; it.density = density; it.color[0] = r; it.color[1] = g; it.color[2] = b; it.anisotropy = aniso;
    return it;
}

static bool same(const std::vector<MedEntry>& a, const std::vector<MedEntry>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].type != b[i].type || memcmp(&a[i].density, &b[i].density, 4) || memcmp(a[i].color, b[i].color, 12) || memcmp(&a[i].anisotropy, &b[i].anisotropy, 4)) return false;
    return true;
}

static int checks()
{
    // three meshes of 2, 3 and 1 triangles
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first = {0u, 4u, 9u, 12u};
    plan.tri_first = {0u, 2u, 5u, 6u};
    plan.mesh_material = {0u, 1u, 2u};
    plan.n_slots = 6;
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    std::vector<MedEntry> current, medium;
    std::string err;
    // the table the rejected calls must leave: mesh 1 carries a fog
    {
        const rpt_mesh_medium it = item(1, RPT_MEDIUM_SCATTER, 2.5f, 0.1f, 0.2f, 0.3f, 0.97f);
        REQUIRE(check_mesh_media(plan, true, &it, 1, current, medium, err) == RPT_OK);
        REQUIRE(medium.size() == 3 && medium[1].type == RPT_MEDIUM_SCATTER && medium[1].anisotropy == 0.9f && medium[0].type == RPT_MEDIUM_NONE);
        current = medium;
    }
    const std::vector<MedEntry> held = current;
    const auto answer = [&](const char* what, bool mesh_scene, const RefitPlan& p, const rpt_mesh_medium* items, uint32_t n) {
        std::vector<MedEntry> out = held;
        out[0].density = 77.0f;                                      // a marker: a rejected call must not write `out`
        const std::vector<MedEntry> before = out;
        err.clear();
        const int rc = check_mesh_media(p, mesh_scene, items, n, current, out, err);
        printf("%s: %d %s\n", what, rc, err.c_str());
        return rc != RPT_OK && same(out, before) && same(current, held);
    };
    // each case but the last carries the NEXT check's fault as well, so the order itself is held
    RefitPlan huge = plan;
    huge.ok = false;
    const rpt_mesh_medium bad_mesh[1] = {item(3, 9)};
    const rpt_mesh_medium twice[2] = {item(0, RPT_MEDIUM_ABSORB), item(0, 9)};
    const rpt_mesh_medium type[1] = {item(0, 4, -1.0f)};
    const rpt_mesh_medium dneg[1] = {item(0, RPT_MEDIUM_ABSORB, -1.0f, nan)};
    const rpt_mesh_medium dinf[1] = {item(0, RPT_MEDIUM_ABSORB, inf, nan)};
    const rpt_mesh_medium dnan[1] = {item(0, RPT_MEDIUM_ABSORB, nan, nan)};
    const rpt_mesh_medium col[1] = {item(0, RPT_MEDIUM_ABSORB, 1.0f, 0.5f, inf, 0.5f, nan)};
    const rpt_mesh_medium ani[1] = {item(0, RPT_MEDIUM_ABSORB, 1.0f, 0.5f, 0.5f, 0.5f, nan)};
    const rpt_mesh_medium later[2] = {item(2, RPT_MEDIUM_EMISSIVE), item(0, RPT_MEDIUM_ABSORB, 1.0f, 0.5f, 0.5f, 0.5f, -inf)};
    REQUIRE(answer("no scene", false, huge, nullptr, 1));
    REQUIRE(answer("2^32 vertices", true, huge, nullptr, 1));
    REQUIRE(answer("NULL items", true, plan, nullptr, 1));
    REQUIRE(answer("mesh out of range", true, plan, bad_mesh, 1));
    REQUIRE(answer("named twice", true, plan, twice, 2));
    REQUIRE(answer("type", true, plan, type, 1));
    REQUIRE(answer("negative density", true, plan, dneg, 1));
    REQUIRE(answer("infinite density", true, plan, dinf, 1));
    REQUIRE(answer("nan density", true, plan, dnan, 1));
    REQUIRE(answer("colour", true, plan, col, 1));
    REQUIRE(answer("anisotropy", true, plan, ani, 1));
    REQUIRE(answer("a later item", true, plan, later, 2));
    // too many media: a scene of kMedMaxMedia + 2 one-triangle meshes, kMedMaxMedia - 1 of them already carrying a medium
    {
        const uint32_t n = kMedMaxMedia + 2u;
        RefitPlan big;
        big.ok = true;
        big.n_slots = n;
        for (uint32_t m = 0; m <= n; ++m) { big.mesh_first.push_back(3u * m); big.tri_first.push_back(m); }
        big.mesh_material.assign(n, 0u);
        std::vector<MedEntry> full(n), out;
        for (uint32_t m = 0; m + 3u < n; ++m) { full[m].type = RPT_MEDIUM_ABSORB; full[m].density = 1.0f; }
        const rpt_mesh_medium one_more[1] = {item(n - 2u, RPT_MEDIUM_ABSORB)};
        REQUIRE(check_mesh_media(big, true, one_more, 1, full, out, err) == RPT_OK && out.size() == n);       // exactly kMedMaxMedia
        const rpt_mesh_medium two_more[2] = {item(n - 2u, RPT_MEDIUM_ABSORB), item(n - 1u, RPT_MEDIUM_EMISSIVE)};
        out.clear();
        const int rc = check_mesh_media(big, true, two_more, 2, full, out, err);
        printf("too many: %d %s\n", rc, err.c_str());
        REQUIRE(rc == RPT_ERR_UNSUPPORTED && out.empty());
        const rpt_mesh_medium swap[2] = {item(0, RPT_MEDIUM_NONE), item(n - 1u, RPT_MEDIUM_EMISSIVE)};          // one leaves, one comes: kMedMaxMedia - 1 still
        REQUIRE(check_mesh_media(big, true, swap, 2, full, out, err) == RPT_OK);
    }
    // the clamp, and what is accepted at the edges
    {
        const float in[] = {0.0f, -0.0f, 0.9f, -0.9f, 0.90000004f, -0.90000004f, 1.0f, -1.0f, 3.0e38f, -3.0e38f, 0.5f, 1e-45f};
        for (float g : in) {
            const float c = med_clamp_anisotropy(g);
            uint32_t gb, cb;
            memcpy(&gb, &g, 4); memcpy(&cb, &c, 4);
            printf("clamp %08x %08x\n", gb, cb);
        }
        const rpt_mesh_medium edge[3] = {item(0, RPT_MEDIUM_EMISSIVE, 0.0f, -3.0f, 1e30f, 0.0f, 5.0f), item(1, RPT_MEDIUM_NONE, 9.0f, 1.0f, 1.0f, 1.0f, -5.0f),
                                         item(2, RPT_MEDIUM_ABSORB, 3.0e38f, 1.0f, 1.0f, 1.0f, -0.95f)};
        REQUIRE(check_mesh_media(plan, true, edge, 3, current, medium, err) == RPT_OK);
        REQUIRE(medium[0].type == RPT_MEDIUM_EMISSIVE && medium[0].density == 0.0f && medium[0].color[0] == -3.0f && medium[0].anisotropy == 0.9f);
        REQUIRE(medium[1].type == RPT_MEDIUM_NONE && medium[1].density == 0.0f && medium[1].color[0] == 0.0f && medium[1].anisotropy == 0.0f);   // NONE drops its fields
        REQUIRE(medium[2].type == RPT_MEDIUM_ABSORB && medium[2].anisotropy == -0.9f);
        REQUIRE(same(current, held));
        REQUIRE(check_mesh_media(plan, true, nullptr, 0, current, medium, err) == RPT_OK && same(medium, held));           // n_items == 0: the table as it is
    }
    // the plan of the held table: the middle mesh carries the medium
    MedPlan mp;
    build_med_plan(plan, held, mp);
    REQUIRE(mp.any() && mp.n_media() == 1 && mp.on_mesh[0] == 1 && !mp.on(0) && mp.on(1) && !mp.on(2) && mp.n_meshes == 3 && mp.n_tris == 6);
    printf("tri_medium");
    for (uint32_t k : mp.tri_medium) printf(" %u", k);
    printf("\n");
    REQUIRE(mp.rows.size() == kMedRowWords);
    MedRow row;
    memcpy(&row, mp.rows.data(), sizeof(row));
    REQUIRE(row.type == RPT_MEDIUM_SCATTER && row.density == 2.5f && row.color[0] == 0.1f && row.color[1] == 0.2f && row.color[2] == 0.3f && row.anisotropy == 0.9f && row.mesh == 1);
    // two media: ordinals in ascending mesh order whatever the order of the items
    {
        const rpt_mesh_medium two[2] = {item(2, RPT_MEDIUM_ABSORB), item(0, RPT_MEDIUM_EMISSIVE)};
        REQUIRE(check_mesh_media(plan, true, two, 2, held, medium, err) == RPT_OK);
        MedPlan p3;
        build_med_plan(plan, medium, p3);
        REQUIRE(p3.n_media() == 3 && p3.on_mesh[0] == 0 && p3.on_mesh[1] == 1 && p3.on_mesh[2] == 2);
        const uint32_t want[6] = {0, 0, 1, 1, 1, 2};
        REQUIRE(memcmp(p3.tri_medium.data(), want, sizeof(want)) == 0);
        rpt_mesh_medium out;
        med_item_of(p3, 1, out);
        REQUIRE(out.mesh == 1 && out.medium_type == RPT_MEDIUM_SCATTER && out.anisotropy == 0.9f);
        p3.release_staging();
        REQUIRE(p3.rows.empty() && p3.tri_medium.empty() && p3.any() && p3.n_media() == 3);
    }
    // the layout: nothing overlaps, everything 16-byte aligned, the all-ones table inside the empty emission-map block
    const MedLayout ml = mp.layout();
    REQUIRE(ml.off_rows == 0 && ml.off_tri_medium >= sizeof(MedRow) * mp.n_media() && ml.off_flat_bits >= ml.off_tri_medium + 4u * 6u);
    REQUIRE(ml.off_emap >= ml.off_flat_bits + 4u && ml.total >= ml.off_emap + ml.emap.total);
    REQUIRE(ml.off_tri_medium % 16 == 0 && ml.off_flat_bits % 16 == 0 && ml.off_emap % 16 == 0 && ml.total % 16 == 0);
    REQUIRE(ml.off_all_ones() >= ml.off_emap && ml.off_all_ones() + 4u * 6u <= ml.total);
    MedPlan none;
    REQUIRE(!none.any() && none.n_media() == 0);
    printf("checks OK\n");
    return 0;
}

// ---- the composer --------------------------------------------------------------------------------------------------------------------
using namespace rptargs;
constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3;

// the media allocation as capi.hip's med_device fills the device's
static std::vector<unsigned char> med_allocation(const MedPlan& mp)
{
    const MedLayout ml = mp.layout();
    std::vector<unsigned char> a(ml.total, 0);
    for (const MapFill& f : ml.emap.fills())
        if (f.bytes && f.value) memset(a.data() + ml.off_emap + f.off, f.value, f.bytes);
    if (!mp.rows.empty()) memcpy(a.data() + ml.off_rows, mp.rows.data(), 4 * mp.rows.size());
    if (!mp.tri_medium.empty()) memcpy(a.data() + ml.off_tri_medium, mp.tri_medium.data(), 4 * mp.tri_medium.size());
    return a;
}

template <class S> static int compose_one(const MeshView& v, const MmapView& m, bool material_maps, const EmapView& e, bool emission_maps, const MedView& md, const char* name)
{
    using Base = typename med_base_of<S>::type;
    static_assert(sizeof(S) == sizeof(Base) + 16, "the media's part is two pointers");
    static_assert(S::kMedia && !Base::kMedia, "WithMedia<> over the emission-mapped form");
    const S s = mesh_med_scene_of<S>(v, m, material_maps, e, emission_maps, md);
    const MedLayout ml = md.med_plan.layout();
    unsigned char* base = static_cast<unsigned char*>(md.med);
    const unsigned char* ones = base + ml.off_all_ones();
    const EmapView lent{base + ml.off_emap, md.med_plan.zero_emap};
    Base want = mesh_emit_scene_of<Base>(v, m, material_maps, emission_maps ? e : lent);
    if (!v.has_smooth()) want.smooth_bits = reinterpret_cast<const uint32_t*>(base + ml.off_flat_bits);
    if (!v.has_lights()) want.tri_light = reinterpret_cast<const uint32_t*>(ones);
    if (!v.has_tex()) want.tri_tex = reinterpret_cast<const uint32_t*>(ones);
    REQUIRE(memcmp(static_cast<const Base*>(&s), &want, sizeof(Base)) == 0);              // every base field, padding included (S s{} zeroes it)
    REQUIRE(reinterpret_cast<const unsigned char*>(s.med_rows) == base + ml.off_rows);
    REQUIRE(reinterpret_cast<const unsigned char*>(s.tri_medium) == base + ml.off_tri_medium);
    const bool own_emap = reinterpret_cast<const unsigned char*>(s.emit_desc) == static_cast<const unsigned char*>(e.emap);
    REQUIRE(own_emap == emission_maps);
    // what a lent table holds, read through the argument's own pointers (real memory: the sanitizer checks every read)
    if (!emission_maps) {
        for (uint32_t j = 0; j < md.med_plan.n_meshes; ++j) REQUIRE(s.emit_desc[j].flags == 0u && s.emit_light_desc[j].flags == 0u);
        REQUIRE(reinterpret_cast<const unsigned char*>(s.emit_texels) <= base + ml.total);
        if (!material_maps) for (uint32_t j = 0; j < md.med_plan.n_meshes; ++j) REQUIRE(s.map_desc[j].flags == 0u);
    }
    if (!v.has_smooth()) for (uint32_t w = 0; w < (kTris + 31) / 32; ++w) REQUIRE(s.smooth_bits[w] == 0u);
    if (!v.has_lights()) { for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_light[k] == kLightNone); REQUIRE(s.n_pick >= s.n_lights); }
    if (!v.has_tex()) for (uint32_t k = 0; k < kTris; ++k) REQUIRE(s.tri_tex[k] == kTexNone);
    for (uint32_t k = 0; k < kTris; ++k) REQUIRE(med_ordinal_of(s.tri_medium, k) == (k < 20 ? kMedNone : 0u));
    REQUIRE(s.med_rows[0].type == RPT_MEDIUM_ABSORB && s.med_rows[0].mesh == 1);
    REQUIRE(s.tri_light != nullptr && s.tri_tex != nullptr && s.smooth_bits != nullptr);
    printf("%s emap %s tex %s lights %s smooth %s\n", name, emission_maps ? "own" : "lent", v.has_tex() ? "own" : "lent", v.has_lights() ? "own" : "lent",
           v.has_smooth() ? "own" : "lent");
    return 0;
}

static int compose()
{
    for (int bits = 0; bits < 32; ++bits) for (int env = 0; env < 3; ++env) {
        const bool emaps = bits & 1, maps = bits & 2, lights = bits & 4, tex = bits & 8, smooth = bits & 16;
        if ((emaps || maps) && !tex) continue;                       // a map needs a texture
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        RefitPlan rp; SmoothPlan sp; LightPlan lp; TexPlan tp; EnvPlan ep; CutPlan cp; NrmPlan np; MmapPlan mp; EmapPlan emp;
        rp.ok = true; rp.mesh_first = {0, 5, kVertices}; rp.tri_first = {0, 20, kTris}; rp.n_slots = kTris; rp.mesh_material = {0, 1};
        void* const refit = (void*)(1ull << 40);
        void *smooth_a = nullptr, *light_a = nullptr, *tex_a = nullptr, *env_a = nullptr, *mmap_a = nullptr, *emap_a = nullptr;
        if (smooth) { sp.mode = {1, 0}; sp.n_tris = kTris; smooth_a = (void*)(2ull << 40); }
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        if (tex) { tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4; tex_a = (void*)(4ull << 40); }
        if (env) { ep.size = 4; ep.mode = env == 2 ? RPT_ENV_SAMPLED : RPT_ENV_BACKGROUND_ONLY; ep.scale = 1.5f; ep.n_tris = kTris; ep.q_total = env == 2 ? 12345u : 0u; env_a = (void*)(5ull << 40); }
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
        MedPlan medp;
        {
            std::vector<MedEntry> me(2);
            me[1].type = RPT_MEDIUM_ABSORB; me[1].density = 2.0f;
            build_med_plan(rp, me, medp);
        }
        std::vector<unsigned char> med_mem = med_allocation(medp);
        const MmapView m{mmap_a, mp};
        const EmapView e{emap_a, emp};
        const MedView md{med_mem.data(), medp};
        const bool material_maps = mmap_a && mp.any(), emission_maps = emap_a && emp.any();
        REQUIRE(material_maps == maps && emission_maps == emaps);
        // (the cutout and normal-map forms are only taken while those features are present, and they need a texture)
        const MeshView plain{scene, refit, smooth_a, light_a, tex_a, env_a, nullptr, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_cut{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nullptr, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_nrm{scene, refit, smooth_a, light_a, tex_a, env_a, nullptr, nrm_a, rp, sp, lp, tp, ep, cp, np};
        const MeshView with_all{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};
        printf("bits %d env %d\n", bits, env);
        if (!env) {
            REQUIRE(compose_one<SceneMeshMed>(plain, m, material_maps, e, emission_maps, md, "light_tex") == 0);
            if (tex) {
                REQUIRE(compose_one<SceneMeshMedCut>(with_cut, m, material_maps, e, emission_maps, md, "cut") == 0);
                REQUIRE(compose_one<SceneMeshMedNrm>(with_nrm, m, material_maps, e, emission_maps, md, "nrm") == 0);
                REQUIRE(compose_one<SceneMeshMedNrmCut>(with_all, m, material_maps, e, emission_maps, md, "nrm_cut") == 0);
            }
        } else {
            REQUIRE(compose_one<SceneMeshMedEnv>(plain, m, material_maps, e, emission_maps, md, "env") == 0);
            if (tex) {
                REQUIRE(compose_one<SceneMeshMedCutEnv>(with_cut, m, material_maps, e, emission_maps, md, "cut_env") == 0);
                REQUIRE(compose_one<SceneMeshMedNrmEnv>(with_nrm, m, material_maps, e, emission_maps, md, "nrm_env") == 0);
                REQUIRE(compose_one<SceneMeshMedNrmCutEnv>(with_all, m, material_maps, e, emission_maps, md, "nrm_cut_env") == 0);
            }
        }
    }
    printf("compose OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    if (argc == 2 && !strcmp(argv[1], "forms")) {
        for (unsigned b = 0; b < 512; ++b)
            printf("%u %u %u\n", b, mesh_form_emit_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64, b & 128),
                   mesh_form_med_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32, b & 64, b & 128, b & 256));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "compose")) return compose();
    fprintf(stderr, "usage: med_harness checks | forms | compose\n");
    return 2;
}
