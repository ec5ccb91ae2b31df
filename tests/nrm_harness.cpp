// nrm_harness.cpp — csrc/host_nrm.h on the host (tests/test_mesh_normal_map_host.py); a stand-alone program, so it may be built
// with -fsanitize=address,undefined and run as it is.
//
//   nrm_harness decode IN OUT   IN:  u32 n_texels, flags, then f32 strength, then n_texels x 4 bytes RGBA
//                               OUT: n_texels x 4 f32 (nrm_decode_reference)
//   nrm_harness bend IN OUT     IN:  u32 n, then n x 18 f32 {N, e1, e2, sa, ta, sb, tb, sc, tc, x, y, z}
//                               OUT: n x 3 f32 (nrm_bend)
//   nrm_harness shade IN OUT    IN:  u32 width, height, wrap, filter, n, then width*height x 4 f32 decoded texels, then n x 17 f32
//                                    {N, e1, e2, u, v, sa, ta, sb, tb, sc, tc}
//                               OUT: n x 3 f32 (nrm_shade: tex_interp, tex_lookup, nrm_bend)
//   nrm_harness checks          every host check of rpt_set_mesh_normal_maps, in its order; the plan, the layout and the descriptors
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_nrm.h"

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
    uint32_t head[2];
    float strength;
    REQUIRE(fread(head, 4, 2, f) == 2 && fread(&strength, 4, 1, f) == 1);
    const size_t n = head[0];
    std::vector<uint8_t> bytes(4 * n);                               // exactly the map's bytes: anything outside is the sanitizer's to find
    REQUIRE(n == 0 || fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
    std::vector<TexTexel> texels(n);
    nrm_decode_reference(bytes.data(), n, strength, head[1], texels.data());
    std::vector<float> out(4 * n);
    if (n) memcpy(out.data(), texels.data(), 16 * n);
    REQUIRE(write_floats(out_path, out) == 0);
    printf("decode OK\n");
    return 0;
}

static int bend(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t n;
    REQUIRE(fread(&n, 4, 1, f) == 1);
    std::vector<float> in(18 * (size_t)n), out(3 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[18 * i];
        nrm_bend(r, r + 3, r + 6, r[9], r[10], r[11], r[12], r[13], r[14], r[15], r[16], r[17], &out[3 * i]);
    }
    REQUIRE(write_floats(out_path, out) == 0);
    printf("bend OK\n");
    return 0;
}

static int shade(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[5];
    REQUIRE(fread(head, 4, 5, f) == 5);
    const uint32_t w = head[0], h = head[1], n = head[4];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    std::vector<TexTexel> texels((size_t)w * h);
    REQUIRE(fread(texels.data(), 16, texels.size(), f) == texels.size());
    std::vector<float> in(17 * (size_t)n), out(3 * (size_t)n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &in[17 * i];
        nrm_shade(r, r + 3, r + 6, r[9], r[10], r[11], r[12], r[13], r[14], r[15], r[16], texels.data(), w, h, head[2], head[3], &out[3 * i]);
    }
    REQUIRE(write_floats(out_path, out) == 0);
    printf("shade OK\n");
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
    const std::vector<NrmMap> none;
    std::vector<NrmMap> map;
    std::string err;
    const uint8_t px[4] = {1, 2, 3, 4};                              // (never read by the checks: any non-NULL pointer says "set")
    const auto on = [&](uint32_t mesh, uint32_t w, uint32_t h, float strength = 1.0f, uint32_t filter = RPT_TEX_FILTER_BILINEAR, uint32_t flags = 0u) {
        rpt_mesh_normal_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_NORMAL_MAP_ON; it.width = w; it.height = h; it.texels = px; it.filter = filter; it.flags = flags;
        it.strength = strength;
        return it;
    };
    const auto off = [&](uint32_t mesh) {
        rpt_mesh_normal_map it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_NORMAL_MAP_OFF;
        return it;
    };
    const auto run = [&](const rpt_mesh_normal_map* items, uint32_t n, const std::vector<NrmMap>& cur = std::vector<NrmMap>()) {
        return check_mesh_normal_maps(plan, true, tex, items, n, cur, map, err);
    };
    const auto says = [&](const char* what) { return err.find(what) != std::string::npos; };
    const int INVALID = RPT_ERR_INVALID_ARG;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    // no scene comes before everything else, then NULL items
    REQUIRE(check_mesh_normal_maps(plan, false, tex, nullptr, 1, none, map, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_normal_maps: ") == 0);
    REQUIRE(run(nullptr, 1) == INVALID && says("items is NULL") && err.find("rpt_set_mesh_normal_maps: ") == 0);
    REQUIRE(run(nullptr, 0) == RPT_OK && map.size() == 3 && !map[0].width && !map[2].width);
    rpt_mesh_normal_map good[2] = {on(0, 5, 3, 0.0f, RPT_TEX_FILTER_NEAREST), on(2, 33, 7, 16.0f, RPT_TEX_FILTER_BILINEAR, RPT_NORMAL_MAP_FLIP_GREEN)};
    REQUIRE(run(good, 2) == RPT_OK && map[0].width == 5 && map[0].height == 3 && map[0].strength == 0.0f && map[0].filter == RPT_TEX_FILTER_NEAREST &&
            !map[1].width && map[2].width == 33 && map[2].strength == 16.0f && map[2].flags == RPT_NORMAL_MAP_FLIP_GREEN);
    const std::vector<NrmMap> held = map;
    // per item, in order: the first fault of the first faulty item answers.  Each case carries the NEXT check's fault as well.
    rpt_mesh_normal_map it[2];
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
    it[0] = on(0, 2, 2, 1.0f, 2u); it[0].texels = nullptr;           // the pointer before the filter
    REQUIRE(run(it, 1) == INVALID && says("texels is NULL"));
    it[0] = on(0, 2, 2, 1.0f, 2u, 2u);                               // the filter before the flags
    REQUIRE(run(it, 1) == INVALID && says("filter 2"));
    it[0] = on(0, 2, 2, -1.0f, RPT_TEX_FILTER_NEAREST, 6u);          // the flags before the strength
    REQUIRE(run(it, 1) == INVALID && says("unknown flag bits 0x6"));
    it[0] = on(1, 2, 2, -1.0f);                                      // the strength before "untextured" (mesh 1 is)
    REQUIRE(run(it, 1) == INVALID && says("strength"));
    it[0] = on(1, 2, 2, 16.5f);
    REQUIRE(run(it, 1) == INVALID && says("strength"));
    it[0] = on(1, 2, 2, inf);
    REQUIRE(run(it, 1) == INVALID && says("strength"));
    it[0] = on(1, 2, 2, nan);
    REQUIRE(run(it, 1) == INVALID && says("strength"));
    it[0] = off(0); it[0].width = 1; it[0].strength = nan;           // an OFF item's strength is checked before its size
    REQUIRE(run(it, 1) == INVALID && says("strength"));
    it[0] = off(0); it[0].width = 1;
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_NORMAL_MAP_OFF takes"));
    it[0] = off(0); it[0].texels = px;
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_NORMAL_MAP_OFF takes"));
    it[0] = on(1, 16384, 16384);                                     // "untextured" before the total
    REQUIRE(run(it, 1) == INVALID && says("mesh 1 is untextured") && says("1 x 1 white texture"));
    it[0] = on(0, 8192, 8192); it[1] = on(2, 1, 1);                   // 2^26 + 1
    REQUIRE(run(it, 2) == RPT_ERR_UNSUPPORTED && says("2^26"));
    it[0] = on(0, 8192, 8192);
    REQUIRE(run(it, 1) == RPT_OK);                                   // exactly 2^26
    REQUIRE(run(it, 1, held) == RPT_ERR_UNSUPPORTED && says("2^26"));     // mesh 2 keeps its 33 x 7
    // a rejected call leaves `map` alone; OFF removes; a mesh not named keeps its map
    map = held;
    it[0] = on(1, 2, 2);
    REQUIRE(run(it, 1, held) == INVALID && map.size() == 3 && map[0].width == 5 && map[2].width == 33);
    it[0] = off(0);
    REQUIRE(run(it, 1, held) == RPT_OK && !map[0].width && map[2].width == 33 && map[2].height == 7 && map[2].strength == 16.0f);
    it[0] = off(1);                                                  // removing what is not there (even from an untextured mesh) is no error
    REQUIRE(run(it, 1, held) == RPT_OK && map[0].width == 5);
    // the plan, the layout, the descriptors
    NrmPlan np;
    build_nrm_plan(plan, held, np);
    REQUIRE(np.any() && np.on(0) && !np.on(1) && np.on(2) && !np.on(3) && np.n_meshes == 3 && np.n_tris == 3);
    REQUIRE(np.map[0].first == 0 && np.map[2].first == 15 && np.n_texels == 15 + 231);
    const NrmLayout nl(np.n_meshes, np.n_tris, np.n_texels);
    REQUIRE(nl.off_desc == 0 && nl.off_none == 48 && nl.off_texels == 64 && nl.total == 64 + 16 * 246 && sizeof(NrmDesc) == 16 && sizeof(TexTexel) == 16);
    const std::vector<uint32_t> d = nrm_desc_table(np, tex);
    const std::vector<uint32_t> want = {0u, 5u, 3u, 1u, 15u, 33u, 7u, 7u, 0u, 0u, 0u, 0u};      // by texture ordinal; mesh 2 is CLAMP and BILINEAR
    REQUIRE(d == want);
    {                                                                // mesh 1 textured as well, all CLAMP: ordinals move, texels do not
        std::vector<TexImage> image(3);
        for (TexImage& im : image) { im.width = 2; im.height = 2; im.wrap = RPT_TEX_WRAP_CLAMP; }
        TexPlan t3;
        build_tex_plan(plan, image, std::vector<float>(), t3);
        const std::vector<uint32_t> d3 = nrm_desc_table(np, t3);
        const std::vector<uint32_t> want3 = {0u, 5u, 3u, 3u, 0u, 0u, 0u, 0u, 15u, 33u, 7u, 7u};
        REQUIRE(d3 == want3);
    }
    NrmPlan empty;
    build_nrm_plan(plan, none, empty);
    REQUIRE(!empty.any() && empty.n_texels == 0 && empty.map.size() == 3);
    // the decode's stated exact values
    REQUIRE(nrm_decode_value(128) == 0.0f && nrm_decode_value(255) == 1.0f && nrm_decode_value(0) == -1.0f && nrm_decode_value(1) == -1.0f);
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "bend")) return bend(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "shade")) return shade(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    fprintf(stderr, "usage: nrm_harness decode IN OUT | bend IN OUT | shade IN OUT | checks\n");
    return 2;
}
