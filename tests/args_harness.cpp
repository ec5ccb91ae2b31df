// args_harness.cpp — csrc/mesh_args.h on the host (tests/test_mesh_args_host.py); a stand-alone program, so it may be built with
// -fsanitize=address,undefined and run as it is.  It binds arguments over made-up allocation bases and prints what it bound; the test
// holds the properties.
//
//   args_harness forms     for bits 0 .. 63 (smooth, lights, textured, environment, cutouts, normal_maps from the lowest bit up) one line:
//                          "<bits> <mesh_form_of's form as a number>"
//   args_harness states    for every reachable state — smooth, lights, textures free; the environment absent, BACKGROUND_ONLY or SAMPLED;
//                          cutouts and normal maps only with textures — one JSON object per line: the state, the form mesh_form_of
//                          picks, every allocation's base, total and offsets (the plan's own layout()), the empty tables the live
//                          allocations carry, and every field mesh_scene_of<that form> bound beyond SceneMesh's own
#include <cstdio>
#include <cstring>
#include <string>

#include "../rust-pathtracer_amd/csrc/mesh_args.h"

using namespace rptargs;

constexpr uint32_t kTris = 37, kVertices = 11, kSceneLights = 3;

static std::string g_out;
static void put(const char* name, const void* p) { char b[96]; snprintf(b, sizeof(b), "\"%s\": %llu, ", name, (unsigned long long)(uintptr_t)p); g_out += b; }
static void put(const char* name, uint64_t v) { char b[96]; snprintf(b, sizeof(b), "\"%s\": %llu, ", name, (unsigned long long)v); g_out += b; }
static void put(const char* name, uint32_t v) { put(name, (uint64_t)v); }
static void put(const char* name, float v) { char b[96]; snprintf(b, sizeof(b), "\"%s\": %.9g, ", name, (double)v); g_out += b; }
#define PUT(f) put(#f, s.f)

static void fields(const SceneMesh& s) { PUT(n_lights); PUT(n_lights_f); PUT(n_tris); }
static void fields(const SceneMeshSmooth& s) { fields((const SceneMesh&)s); PUT(slot_vertex); PUT(vnormals); PUT(smooth_bits); }
static void fields(const SceneMeshLight& s)
{
    fields((const SceneMeshSmooth&)s);
    PUT(vertices); PUT(face_vertex); PUT(light_desc); PUT(light_cdf); PUT(tri_light); PUT(n_faces); PUT(n_pick);
}
template <class B> static void fields(const SceneMeshTexT<B>& s) { fields((const B&)s); PUT(tex_desc); PUT(tri_tex); PUT(uvs); PUT(texels); }
template <class B> static void fields(const SceneMeshEnvT<B>& s)
{
    fields((const B&)s);
    PUT(env_texels); PUT(env_cdf); PUT(env_q); PUT(env_q_f); PUT(env_scale); PUT(env_size); PUT(env_pick);
}
template <class B> static void fields(const SceneMeshCutT<B>& s) { fields((const B&)s); PUT(cut_desc); PUT(cut_bits); }
template <class B> static void fields(const SceneMeshNrmT<B>& s) { fields((const B&)s); PUT(nrm_desc); PUT(nrm_texels); }

template <class S> static void bound(const MeshView& v)
{
    g_out += "\"arg\": {";
    fields(mesh_scene_of<S>(v));
    g_out += "\"size\": " + std::to_string(sizeof(S)) + "}";
}

// an allocation: "name": {"base": .., "total": .., "<offset>": .., ..}
#define OFF(f) put(#f, (uint64_t)lay.f)
#define ALLOC(name, base, ...) do { g_out += "\"" name "\": {"; put("base", base); __VA_ARGS__; g_out += "\"total\": " + std::to_string(lay.total) + "}, "; } while (0)
// an empty table a live allocation carries: [kind, allocation, offset, bytes]
static void empty(const char* kind, const char* alloc, size_t off, size_t bytes)
{
    char b[128];
    snprintf(b, sizeof(b), "[\"%s\", \"%s\", %zu, %zu], ", kind, alloc, off, bytes);
    g_out += b;
}

static int states()
{
    for (int smooth = 0; smooth < 2; ++smooth) for (int lights = 0; lights < 2; ++lights) for (int env = 0; env < 3; ++env)
    for (int tex = 0; tex < 2; ++tex) for (int cut = 0; cut <= tex; ++cut) for (int nrm = 0; nrm <= tex; ++nrm) {
        // two meshes, 37 triangles; mesh 0 SMOOTH, textured, with a cutout and a normal map, mesh 1 ON
        SceneMesh scene;
        memset(&scene, 0, sizeof(scene));
        scene.n_lights = kSceneLights; scene.n_lights_f = (float)kSceneLights; scene.n_tris = kTris;
        rpthost::RefitPlan rp; rpthost::SmoothPlan sp; rpthost::LightPlan lp; rpthost::TexPlan tp; rpthost::EnvPlan ep; rpthost::CutPlan cp; rpthost::NrmPlan np;
        rp.mesh_first = {0, 5, kVertices}; rp.n_slots = kTris;
        // present allocations far apart, absent ones null: a pointer made from a null base lies below every allocation
        void* const refit = (void*)(1ull << 40);
        void *smooth_a = nullptr, *light_a = nullptr, *tex_a = nullptr, *env_a = nullptr, *cut_a = nullptr, *nrm_a = nullptr;
        if (smooth) { sp.mode = {RPT_MESH_SHADING_SMOOTH, RPT_MESH_SHADING_FLAT}; sp.n_vertices = kVertices; sp.n_tris = kTris; sp.n_faces = 20; sp.n_adj = 60; smooth_a = (void*)(2ull << 40); }
        if (lights) { lp.mode = {RPT_MESH_LIGHT_OFF, RPT_MESH_LIGHT_ON}; lp.on_mesh = {1}; lp.on_first = {0, 17}; lp.n_tris = kTris; lp.n_faces = 17; light_a = (void*)(3ull << 40); }
        if (tex) { tp.image.resize(2); tp.image[0].width = tp.image[0].height = 2; tp.tex_mesh = {0}; tp.n_tris = kTris; tp.n_vertices = kVertices; tp.n_texels = 4; tex_a = (void*)(4ull << 40); }
        if (env) { ep.size = 4; ep.mode = env == 2 ? RPT_ENV_SAMPLED : RPT_ENV_BACKGROUND_ONLY; ep.scale = 1.5f; ep.n_tris = kTris; ep.q_total = env == 2 ? 12345u : 0u; env_a = (void*)(5ull << 40); }
        if (cut) { cp.mask.resize(2); cp.mask[0].width = cp.mask[0].height = 3; cp.n_meshes = 2; cp.n_tris = kTris; cp.n_words = 1; cut_a = (void*)(6ull << 40); }
        if (nrm) { np.map.resize(2); np.map[0].width = np.map[0].height = 3; np.n_meshes = 2; np.n_tris = kTris; np.n_texels = 9; nrm_a = (void*)(7ull << 40); }
        const MeshView v{scene, refit, smooth_a, light_a, tex_a, env_a, cut_a, nrm_a, rp, sp, lp, tp, ep, cp, np};

        g_out = "{";
        put("smooth", (uint32_t)smooth); put("lights", (uint32_t)lights); put("tex", (uint32_t)tex); put("env", (uint32_t)env);
        put("cut", (uint32_t)cut); put("nrm", (uint32_t)nrm); put("n_on", lp.n_on());
        { const rpthost::RefitLayout lay(rp.n_vertices(), rp.n_slots, rp.n_nodes); ALLOC("refit_a", refit, OFF(off_vertices), OFF(off_slot_vertex)); }
        { const rpthost::SmoothLayout lay = sp.layout(); ALLOC("smooth_a", smooth_a, OFF(off_normals), OFF(off_bits)); }
        { const rpthost::LightLayout lay = lp.layout(); ALLOC("light_a", light_a, OFF(off_desc), OFF(off_cdf), OFF(off_face_vertex), OFF(off_tri_light)); }
        { const rpthost::TexLayout lay = tp.layout(); ALLOC("tex_a", tex_a, OFF(off_desc), OFF(off_tri_tex), OFF(off_uvs), OFF(off_texels)); }
        { const rpthost::EnvLayout lay = ep.layout(); ALLOC("env_a", env_a, OFF(off_texels), OFF(off_cdf)); }
        { const rpthost::CutLayout lay = cp.layout(); ALLOC("cut_a", cut_a, OFF(off_desc), OFF(off_bits)); }
        { const rpthost::NrmLayout lay = np.layout(); ALLOC("nrm_a", nrm_a, OFF(off_desc), OFF(off_texels)); }
        // (host_*.h: what follows each empty table in its layout bounds it)
        g_out += "\"empties\": [";
        if (light_a) { const auto l = lp.layout(); empty("zeros", "light_a", l.off_flat_bits, l.total - l.off_flat_bits); }
        if (tex_a) { const auto l = tp.layout(); empty("zeros", "tex_a", l.off_flat_bits, l.off_texels - l.off_flat_bits); }
        if (env_a) { const auto l = ep.layout(); empty("zeros", "env_a", l.off_flat_bits, l.total - l.off_flat_bits); empty("ones", "env_a", l.off_none, l.off_flat_bits - l.off_none); }
        if (cut_a) { const auto l = cp.layout(); empty("ones", "cut_a", l.off_none, l.off_bits - l.off_none); }
        if (nrm_a) { const auto l = np.layout(); empty("ones", "nrm_a", l.off_none, l.off_texels - l.off_none); }
        g_out += "[]], ";

        const MeshForm form = mesh_form_of(smooth, lights, tex, env != 0, cut, nrm);
        put("form", (uint32_t)form);
        switch (form) {
        case MeshForm::nrm_cut_env: bound<SceneMeshNrmCutEnv>(v); break;
        case MeshForm::nrm_cut: bound<SceneMeshNrmCut>(v); break;
        case MeshForm::nrm_env: bound<SceneMeshNrmEnv>(v); break;
        case MeshForm::nrm: bound<SceneMeshNrm>(v); break;
        case MeshForm::cut_env: bound<SceneMeshCutEnv>(v); break;
        case MeshForm::cut: bound<SceneMeshCut>(v); break;
        case MeshForm::env: bound<SceneMeshEnv>(v); break;
        case MeshForm::light_tex: bound<SceneMeshLightTex>(v); break;
        case MeshForm::tex: bound<SceneMeshTex>(v); break;
        case MeshForm::light: bound<SceneMeshLight>(v); break;
        case MeshForm::smooth: bound<SceneMeshSmooth>(v); break;
        case MeshForm::flat: bound<SceneMesh>(v); break;
        }
        printf("%s}\n", g_out.c_str());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "forms")) {
        for (unsigned b = 0; b < 64; ++b) printf("%u %u\n", b, (unsigned)mesh_form_of(b & 1, b & 2, b & 4, b & 8, b & 16, b & 32));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "states")) return states();
    fprintf(stderr, "usage: args_harness forms|states\n");
    return 2;
}
