// light_harness.cpp — csrc/host_light.h on the host, under the address and undefined-behaviour sanitizers
// (tests/test_mesh_light_host.py).
//
//   light_harness tables IN OUT   IN:  u32 n_meshes, then per mesh u32 n_vertices, u32 n_triangles, u32 mode, u32 material,
//                                      3 n_vertices f32 positions, 3 n_triangles u32 indices (the mesh's own)
//                                 OUT: u32 n_on, u32 n_faces, u32 n_tris (of the scene), on_mesh [n_on], on_first [n_on + 1], desc
//                                      [8 n_on], face_vertex [3][n_faces], face_mesh [n_faces], tri_light [n_tris], then per ON mesh
//                                      in ordinal order i32 E, f32 A_tot, u64 C [its triangles] = light_table_reference.
//   light_harness checks          every host check of rpt_set_mesh_lights, in its order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_light.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int tables(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t n_meshes = 0;
    REQUIRE(fread(&n_meshes, 4, 1, f) == 1);
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first.assign(1, 0u);
    plan.tri_first.assign(1, 0u);
    std::vector<uint8_t> mode;
    std::vector<float> vertices;
    std::vector<uint32_t> flat;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        uint32_t head[4];
        REQUIRE(fread(head, 4, 4, f) == 4);
        const uint32_t first = plan.mesh_first.back();
        const size_t v0 = vertices.size(), t0 = flat.size();
        vertices.resize(v0 + 3 * (size_t)head[0]);
        flat.resize(t0 + 3 * (size_t)head[1]);
        REQUIRE(head[0] == 0 || fread(&vertices[v0], 4, 3 * (size_t)head[0], f) == 3 * (size_t)head[0]);
        REQUIRE(head[1] == 0 || fread(&flat[t0], 4, 3 * (size_t)head[1], f) == 3 * (size_t)head[1]);
        for (size_t i = t0; i < flat.size(); ++i) { REQUIRE(flat[i] < head[0]); flat[i] += first; }
        plan.mesh_first.push_back(first + head[0]);
        plan.tri_first.push_back(plan.tri_first.back() + head[1]);
        plan.mesh_material.push_back(head[3]);
        mode.push_back((uint8_t)head[2]);
    }
    fclose(f);
    plan.n_slots = (uint32_t)(flat.size() / 3);
    LightPlan lp;
    build_light_plan(plan, flat.data(), mode, lp);
    const LightLayout ll(lp.n_on(), lp.n_faces, lp.n_tris);
    REQUIRE(ll.total % 16 == 0 && ll.off_cdf % 16 == 0 && ll.off_part % 16 == 0 && ll.off_block % 16 == 0);
    REQUIRE(ll.off_flat_bits + 4 * (((size_t)lp.n_tris + 31) / 32) <= ll.total && ll.off_tri_light + 4 * (size_t)lp.n_tris <= ll.off_flat_bits);
    REQUIRE(ll.n_blocks == (lp.n_faces + 255u) / 256u);
    REQUIRE(lp.any() == (lp.n_on() > 0));
    for (uint32_t j = 0; j < lp.n_on(); ++j) REQUIRE(lp.on(lp.on_mesh[j]) && lp.ordinal(lp.on_mesh[j]) == j);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    const uint32_t head[3] = {lp.n_on(), lp.n_faces, lp.n_tris};
    const auto put = [&](const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; };
    REQUIRE(put(head, 12) && put(lp.on_mesh.data(), 4 * lp.on_mesh.size()) && put(lp.on_first.data(), 4 * lp.on_first.size()) &&
            put(lp.desc.data(), 4 * lp.desc.size()) && put(lp.face_vertex.data(), 4 * lp.face_vertex.size()) &&
            put(lp.face_mesh.data(), 4 * lp.face_mesh.size()) && put(lp.tri_light.data(), 4 * lp.tri_light.size()));
    for (uint32_t j = 0; j < lp.n_on(); ++j) {
        const size_t n = lp.on_first[j + 1u] - lp.on_first[j];
        std::vector<uint64_t> cdf(n, ~0ull);
        int32_t e = 77;
        float area = -1.0f;
        light_table_reference(vertices.data(), lp, j, cdf.data(), &e, &area);
        REQUIRE(put(&e, 4) && put(&area, 4) && put(cdf.data(), 8 * n));
    }
    fclose(f);
    printf("tables OK\n");
    return 0;
}

static int checks()
{
    // three meshes of 4, 0 and 2 vertices; the second has no triangle
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first = {0u, 4u, 4u, 6u};
    plan.tri_first = {0u, 2u, 2u, 3u};
    plan.mesh_material = {0u, 1u, 2u};
    plan.n_slots = 3;
    const uint32_t MAXD = RPT_SCENE_ANYHIT_USES_MAX_DIST;
    const std::vector<uint8_t> none;
    std::vector<uint8_t> mode;
    std::string err;
    rpt_mesh_light it[3] = {{0u, RPT_MESH_LIGHT_ON}, {1u, RPT_MESH_LIGHT_ON}, {2u, RPT_MESH_LIGHT_OFF}};
    // no scene comes before everything else, then the flag, then 2^32 vertices, then the 2^24 rule, then NULL items
    REQUIRE(check_mesh_lights(plan, false, 0u, 0xFFFFFFFFu, nullptr, 1, none, mode, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_lights: ") == 0);
    REQUIRE(check_mesh_lights(plan, false, MAXD, 1u, nullptr, 0, none, mode, err) == RPT_ERR_NO_SCENE);
    REQUIRE(check_mesh_lights(plan, true, 0u, 0xFFFFFFFFu, nullptr, 1, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("RPT_SCENE_ANYHIT_USES_MAX_DIST") != std::string::npos);
    REQUIRE(check_mesh_lights(plan, true, ~MAXD, 1u, it, 3, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("RPT_SCENE_ANYHIT_USES_MAX_DIST") != std::string::npos);
    RefitPlan huge = plan;
    huge.ok = false;
    REQUIRE(check_mesh_lights(huge, true, MAXD, 1u, nullptr, 1, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("2^32") != std::string::npos);
    // the 2^24 rule: n_lights + ON meshes must stay below 2^24; it comes before the items' own checks
    const uint32_t M = 1u << 24;
    REQUIRE(check_mesh_lights(plan, true, MAXD, M - 2u, it, 3, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("2^24") != std::string::npos);
    REQUIRE(check_mesh_lights(plan, true, MAXD, M - 3u, it, 3, none, mode, err) == RPT_OK && mode == std::vector<uint8_t>({1, 1, 0}));
    REQUIRE(check_mesh_lights(plan, true, MAXD, M, nullptr, 1, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("2^24") != std::string::npos);
    REQUIRE(check_mesh_lights(plan, true, MAXD, M - 1u, nullptr, 1, none, mode, err) == RPT_ERR_INVALID_ARG);       // (no mesh ON: N = 2^24 - 1)
    {   // meshes that are ON already count, and one the call turns OFF does not
        const std::vector<uint8_t> current = {1, 0, 1};
        rpt_mesh_light off = {0u, RPT_MESH_LIGHT_OFF}, on = {1u, RPT_MESH_LIGHT_ON};
        REQUIRE(check_mesh_lights(plan, true, MAXD, M - 2u, &on, 1, current, mode, err) == RPT_ERR_UNSUPPORTED);
        REQUIRE(check_mesh_lights(plan, true, MAXD, M - 2u, &off, 1, current, mode, err) == RPT_OK && mode == std::vector<uint8_t>({0, 0, 1}));
        REQUIRE(check_mesh_lights(plan, true, MAXD, M - 2u, nullptr, 0, current, mode, err) == RPT_ERR_UNSUPPORTED);  // (even a call that names nothing)
        REQUIRE(check_mesh_lights(plan, true, MAXD, M - 3u, nullptr, 0, current, mode, err) == RPT_OK);               // (two ON: N = 2^24 - 1)
    }
    REQUIRE(check_mesh_lights(plan, true, MAXD, 1u, nullptr, 1, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("items is NULL") != std::string::npos);
    REQUIRE(check_mesh_lights(plan, true, MAXD, 1u, nullptr, 0, none, mode, err) == RPT_OK && mode == std::vector<uint8_t>({0, 0, 0}));
    // per item: out of range, then named twice, then the mode; the first fault of the first faulty item answers
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, it, 3, none, mode, err) == RPT_OK && mode == std::vector<uint8_t>({1, 1, 0}));
    rpt_mesh_light bad[3] = {{0u, RPT_MESH_LIGHT_ON}, {3u, 7u}, {0u, 7u}};
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mesh 3 out of range") != std::string::npos);
    bad[1].mesh = 0u;
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mesh 0 is named twice") != std::string::npos);
    bad[1].mesh = 2u;
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mode 7") != std::string::npos);
    bad[1].mode = RPT_MESH_LIGHT_OFF;
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 2: mesh 0 is named twice") != std::string::npos);
    // meshes not named keep their mode
    const std::vector<uint8_t> current = {1, 0, 1};
    rpt_mesh_light one = {0u, RPT_MESH_LIGHT_OFF};
    REQUIRE(check_mesh_lights(plan, true, MAXD, 0u, &one, 1, current, mode, err) == RPT_OK && mode == std::vector<uint8_t>({0, 0, 1}));
    LightPlan lp;
    lp.mode = mode;
    REQUIRE(lp.any() && lp.on(2) && !lp.on(0) && !lp.on(9) && lp.ordinal(2) == kLightNone);       // (no plan built yet: no ordinals)
    lp.mode.clear();
    REQUIRE(!lp.any());
    // the pieces of the table at their ends: exponents of the smallest and largest area, quanta, the total's overflow
    REQUIRE(light_exponent(0.0f) == 0 && light_exponent(1.0f) == 1 && light_exponent(0.75f) == 0 && light_exponent(0.5f) == 0);
    REQUIRE(light_exponent(3.40282347e+38f) == 128 && light_exponent(0x1p-76f) == -75);
    REQUIRE(light_quantum(0.75f, 0) == 3ull << 34 && light_quantum(0x1p-76f, -75) == 1ull << 35 && light_quantum(3.40282347e+38f, 128) == 0xFFFFFFull << 12);
    REQUIRE(light_quantum(0x1p-40f, 0) == 0 && light_quantum(0x1p-36f, 0) == 1);
    REQUIRE(light_total_area(1ull << 35, 0) == 0.5f && light_total_area(0, 5) == 0.0f);
    REQUIRE(light_total_area((1ull << 35) + 1, 0) == 0.5f);         // (rounds to nearest even)
    REQUIRE(light_total_area(3ull << 35, 128) > 3.40282347e+38f);    // +inf
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "tables")) return tables(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: light_harness tables IN OUT | checks\n");
    return 2;
}
