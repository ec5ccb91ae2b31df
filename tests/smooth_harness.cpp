// smooth_harness.cpp — csrc/host_smooth.h on the host, under the address and undefined-behaviour sanitizers
// (tests/test_mesh_smooth_host.py).
//
//   smooth_harness normals IN OUT   IN:  u32 n_meshes, then per mesh u32 n_vertices, u32 n_triangles, u32 mode, 3 n_vertices f32
//                                        positions, 3 n_triangles u32 indices (the mesh's own)
//                                   OUT: u32 n_faces, u32 n_adj, u32 n_vertices (of the scene), face_vertex [3][n_faces], adj_first
//                                        [n_vertices + 1], adj [n_adj], the bits' words, then 4 f32 per vertex = smooth_normals_reference.
//                                   The flattened corners reach build_smooth_plan through smooth_flat_indices, from rows and a
//                                   slot_vertex table in a scrambled slot order, as rpt_set_mesh_shading reads them from a device.
//   smooth_harness hits IN OUT      IN:  u32 n, then n x 24 f32 {o, d, a, e1, e2, na, nb, nc}
//                                   OUT: n x 3 f32 = smooth_hit_normal_reference
//   smooth_harness checks           every host check of rpt_set_mesh_shading, in its order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_smooth.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int normals(const char* in_path, const char* out_path)
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
        uint32_t head[3];
        REQUIRE(fread(head, 4, 3, f) == 3);
        const uint32_t first = plan.mesh_first.back();
        const size_t v0 = vertices.size(), t0 = flat.size();
        vertices.resize(v0 + 3 * (size_t)head[0]);
        flat.resize(t0 + 3 * (size_t)head[1]);
        REQUIRE(head[0] == 0 || fread(&vertices[v0], 4, 3 * (size_t)head[0], f) == 3 * (size_t)head[0]);
        REQUIRE(head[1] == 0 || fread(&flat[t0], 4, 3 * (size_t)head[1], f) == 3 * (size_t)head[1]);
        for (size_t i = t0; i < flat.size(); ++i) { REQUIRE(flat[i] < head[0]); flat[i] += first; }
        plan.mesh_first.push_back(first + head[0]);
        plan.tri_first.push_back(plan.tri_first.back() + head[1]);
        mode.push_back((uint8_t)head[2]);
    }
    fclose(f);
    const size_t n = flat.size() / 3;
    plan.n_slots = (uint32_t)n;
    // a scrambled slot order (slot s holds triangle (s * 7919 + 3) mod n when that is a permutation, else the reversed order)
    std::vector<unsigned char> rows(48 * n, 0xAB);
    std::vector<uint32_t> slot_vertex(3 * n);
    for (size_t s = 0; s < n; ++s) {
        const uint32_t index = (uint32_t)(n % 7919 ? (s * 7919 + 3) % n : n - 1 - s);
        memcpy(&rows[48 * s + 12], &index, 4);
        for (size_t c = 0; c < 3; ++c) slot_vertex[c * n + s] = flat[3 * (size_t)index + c];
    }
    std::vector<uint32_t> back;
    REQUIRE(smooth_flat_indices(rows.data(), slot_vertex.data(), n, back));
    REQUIRE(back == flat);
    if (n >= 2) {                                                   // a table that names a triangle twice is refused
        std::vector<unsigned char> twice = rows;
        memcpy(&twice[48 + 12], &twice[12], 4);
        REQUIRE(!smooth_flat_indices(twice.data(), slot_vertex.data(), n, back));
    }
    SmoothPlan sp;
    build_smooth_plan(plan, flat.data(), mode, sp);
    const SmoothLayout sl(sp.n_vertices, sp.n_tris, sp.n_faces, sp.n_adj);
    REQUIRE(sl.total % 16 == 0 && sl.off_bits + 4 * sp.bits.size() <= sl.total);
    std::vector<float> face(4 * (size_t)sp.n_faces), out(4 * (size_t)sp.n_vertices, 1.0f);
    smooth_normals_reference(vertices.data(), sp, face.data(), out.data());
    f = fopen(out_path, "wb");
    REQUIRE(f);
    const uint32_t head[3] = {sp.n_faces, sp.n_adj, sp.n_vertices};
    const auto put = [&](const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; };
    REQUIRE(put(head, 12) && put(sp.face_vertex.data(), 4 * sp.face_vertex.size()) && put(sp.adj_first.data(), 4 * sp.adj_first.size()) &&
            put(sp.adj.data(), 4 * sp.adj.size()) && put(sp.bits.data(), 4 * sp.bits.size()) && put(out.data(), 4 * out.size()));
    fclose(f);
    printf("normals OK\n");
    return 0;
}

static int hits(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t n = 0;
    REQUIRE(fread(&n, 4, 1, f) == 1);
    std::vector<float> in(24 * (size_t)n), out(3 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[24 * i];
        smooth_hit_normal_reference(r, r + 3, r + 6, r + 9, r + 12, r + 15, r + 18, r + 21, &out[3 * i]);
    }
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE(n == 0 || fwrite(out.data(), 4, out.size(), f) == out.size());
    fclose(f);
    printf("hits OK\n");
    return 0;
}

static int checks()
{
    // three meshes of 4, 0 and 2 vertices; the second has no triangle
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first = {0u, 4u, 4u, 6u};
    plan.tri_first = {0u, 2u, 2u, 3u};
    plan.n_slots = 3;
    const std::vector<uint8_t> none;
    std::vector<uint8_t> mode;
    std::string err;
    rpt_mesh_shading it[3] = {{0u, RPT_MESH_SHADING_SMOOTH}, {1u, RPT_MESH_SHADING_SMOOTH}, {2u, RPT_MESH_SHADING_FLAT}};
    // no scene comes before everything else, then 2^32 vertices, then NULL items
    REQUIRE(check_mesh_shading(plan, false, nullptr, 1, none, mode, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_shading: ") == 0);
    REQUIRE(check_mesh_shading(plan, false, nullptr, 0, none, mode, err) == RPT_ERR_NO_SCENE);
    RefitPlan huge = plan;
    huge.ok = false;
    REQUIRE(check_mesh_shading(huge, true, nullptr, 1, none, mode, err) == RPT_ERR_UNSUPPORTED && err.find("2^32") != std::string::npos);
    REQUIRE(check_mesh_shading(plan, true, nullptr, 1, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("items is NULL") != std::string::npos);
    REQUIRE(check_mesh_shading(plan, true, nullptr, 0, none, mode, err) == RPT_OK && mode == std::vector<uint8_t>({0, 0, 0}));
    // per item: out of range, then named twice, then the mode; the first fault of the first faulty item answers
    REQUIRE(check_mesh_shading(plan, true, it, 3, none, mode, err) == RPT_OK && mode == std::vector<uint8_t>({1, 1, 0}));
    rpt_mesh_shading bad[3] = {{0u, RPT_MESH_SHADING_SMOOTH}, {3u, 7u}, {0u, 7u}};
    REQUIRE(check_mesh_shading(plan, true, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mesh 3 out of range") != std::string::npos);
    bad[1].mesh = 0u;
    REQUIRE(check_mesh_shading(plan, true, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mesh 0 is named twice") != std::string::npos);
    bad[1].mesh = 2u;
    REQUIRE(check_mesh_shading(plan, true, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 1: mode 7") != std::string::npos);
    bad[1].mode = RPT_MESH_SHADING_FLAT;
    REQUIRE(check_mesh_shading(plan, true, bad, 3, none, mode, err) == RPT_ERR_INVALID_ARG && err.find("item 2: mesh 0 is named twice") != std::string::npos);
    // meshes not named keep their mode
    const std::vector<uint8_t> current = {1, 0, 1};
    rpt_mesh_shading one = {0u, RPT_MESH_SHADING_FLAT};
    REQUIRE(check_mesh_shading(plan, true, &one, 1, current, mode, err) == RPT_OK && mode == std::vector<uint8_t>({0, 0, 1}));
    SmoothPlan sp;
    sp.mode = mode;
    REQUIRE(sp.any() && sp.smooth(2) && !sp.smooth(0) && !sp.smooth(9));
    sp.mode.clear();
    REQUIRE(!sp.any());
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "normals")) return normals(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "hits")) return hits(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: smooth_harness normals IN OUT | hits IN OUT | checks\n");
    return 2;
}
