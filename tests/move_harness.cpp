// move_harness.cpp — csrc/host_move.h on the host, under the address and undefined-behaviour sanitizers (tests/test_mesh_move_host.py).
//
//   move_harness run IN OUT    IN:  u32 n, u32 has_transform, 12 f32 transform, 3n f32 positions, n bytes `referenced`
//                              OUT: 3n f32 = move_apply_reference, then the two words of move_check_reference
//   move_harness checks        every host check of a device-source call, in its order, against a pretend device-memory query
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_move.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int run(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[2];
    MoveTransform xf = {};
    REQUIRE(fread(head, 4, 2, f) == 2 && fread(xf.t, 4, 12, f) == 12);
    const uint32_t n = head[0];
    xf.on = head[1];
    std::vector<float> src(3 * (size_t)n), dst(3 * (size_t)n);
    std::vector<uint8_t> referenced(n);
    REQUIRE(n == 0 || (fread(src.data(), 4, src.size(), f) == src.size() && fread(referenced.data(), 1, n, f) == n));
    fclose(f);
    uint32_t words[kMoveWords] = {0u, 0u};
    move_check_reference(src.data(), n, xf, referenced.data(), words);
    move_apply_reference(src.data(), n, xf, dst.data());
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE((n == 0 || fwrite(dst.data(), 4, dst.size(), f) == dst.size()) && fwrite(words, 4, kMoveWords, f) == kMoveWords);
    fclose(f);
    printf("run OK\n");
    return 0;
}

// the pretend query: `g_device` is one allocation of device 3, everything else is not device memory
static float g_device[64];
static int pretend_query(const void* p, size_t bytes, int* device)
{
    const char* c = static_cast<const char*>(p);
    const char* lo = reinterpret_cast<const char*>(g_device);
    if (c < lo || c >= lo + sizeof(g_device)) return kMoveSourceNotDevice;
    if ((size_t)(lo + sizeof(g_device) - c) < bytes) return kMoveSourceShort;
    *device = 3;
    return kMoveSourceOk;
}

static int checks()
{
    // two meshes of 4 and 2 vertices
    RefitPlan plan;
    plan.ok = true;
    plan.mesh_first = {0u, 4u, 6u};
    plan.referenced.assign(6, 1);
    plan.mesh_max_abs = {1.0f, 2.0f};
    static float host[64];
    const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float bad_t[12];
    memcpy(bad_t, ident, sizeof(ident));
    bad_t[7] = __builtin_nanf("");
    float inf_t[12];
    memcpy(inf_t, ident, sizeof(ident));
    inf_t[11] = -__builtin_huge_valf();
    std::vector<int> devices;
    std::string err;
    const char* call = "rpt_update_meshes_device";
    auto check = [&](const std::vector<rpt_mesh_source>& s, bool mesh_scene, const RefitPlan& p) {
        err.clear();
        return check_mesh_sources(p, mesh_scene, s.empty() ? nullptr : s.data(), (uint32_t)(s.empty() ? 1 : s.size()), pretend_query, call, devices, err);
    };
    const rpt_mesh_source good0 = {0u, 4u, g_device, nullptr}, good1 = {1u, 2u, g_device + 12, ident};
    REQUIRE(check({}, true, plan) == RPT_ERR_INVALID_ARG && err == "rpt_update_meshes_device: sources is NULL");
    REQUIRE(check({good0}, false, plan) == RPT_ERR_NO_SCENE && err.find("needs an uploaded scene with meshes") != std::string::npos);
    RefitPlan huge = plan;
    huge.ok = false;
    REQUIRE(check({good0}, true, huge) == RPT_ERR_UNSUPPORTED && err.find("2^32") != std::string::npos);
    REQUIRE(check({{2u, 4u, g_device, nullptr}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 2 out of range") != std::string::npos);
    REQUIRE(check({good1, good1}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 1 is named twice") != std::string::npos);
    REQUIRE(check({{0u, 3u, g_device, nullptr}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 0: n_vertices 3") != std::string::npos);
    REQUIRE(check({{1u, 2u, nullptr, nullptr}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 1: vertices_dev is NULL") != std::string::npos);
    REQUIRE(check({{1u, 2u, host, nullptr}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 1: vertices_dev is not device memory") != std::string::npos);
    REQUIRE(check({{0u, 4u, g_device + 64 - 11, nullptr}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 0: vertices_dev's allocation ends before 4 vertices (48 bytes)") != std::string::npos);
    REQUIRE(check({{0u, 4u, g_device + 64 - 12, nullptr}}, true, plan) == RPT_OK);
    REQUIRE(check({{0u, 4u, g_device + 64 - 11, bad_t}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("allocation ends") != std::string::npos);
    REQUIRE(check({{0u, 4u, g_device, bad_t}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 0: transform entry 7 is not finite") != std::string::npos);
    REQUIRE(check({good0, {1u, 2u, g_device, inf_t}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("mesh 1: transform entry 11 is not finite") != std::string::npos);
    // the order: several faults answer the first; the device-memory question comes before the transform's
    REQUIRE(check({{0u, 3u, host, bad_t}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("n_vertices") != std::string::npos);
    REQUIRE(check({{0u, 4u, host, bad_t}}, true, plan) == RPT_ERR_INVALID_ARG && err.find("not device memory") != std::string::npos);
    REQUIRE(check({good0, {5u, 0u, nullptr, nullptr}}, false, plan) == RPT_ERR_NO_SCENE);
    // accepted: the devices are reported, a mesh without vertices needs no pointer
    REQUIRE(check({good1, good0}, true, plan) == RPT_OK && devices.size() == 2 && devices[0] == 3 && devices[1] == 3);
    RefitPlan empty = plan;
    empty.mesh_first = {0u, 4u, 4u};
    REQUIRE(check({{1u, 0u, nullptr, nullptr}}, true, empty) == RPT_OK && devices[0] == -1);
    // the read-back's meaning
    uint32_t words[kMoveWords] = {move_bits(2.5f), 0u};
    float big = 0.0f;
    REQUIRE(move_check_result(good0, words, call, big, err) == RPT_OK && big == 2.5f);
    words[kMoveWordBad] = 0xFFFFFFFFu - 3u;
    REQUIRE(move_check_result(good0, words, call, big, err) == RPT_ERR_INVALID_ARG && err == "rpt_update_meshes_device: mesh 0 vertex 3 is not finite");
    // the layout keeps the table of bytes behind the words
    const MoveLayout ml(3u, 1000u);
    REQUIRE(ml.off_words == 0 && ml.off_referenced >= 24 && ml.off_referenced % 16 == 0 && ml.total >= ml.off_referenced + 1000);
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: move_harness run IN OUT | checks\n");
    return 2;
}
