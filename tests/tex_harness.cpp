// tex_harness.cpp — csrc/host_tex.h on the host, under the address and undefined-behaviour sanitizers
// (tests/test_mesh_texture_host.py).
//
//   tex_harness decode IN OUT   IN:  u32 n_gammas, f32 gamma [n_gammas], u32 n_texels, u8 RGBA [4 n_texels]
//                               OUT: per gamma 256 f32 L[k] (tex_decode_value), then 4 n_texels f32 (tex_decode_reference)
//   tex_harness lookup IN OUT   IN:  u32 width, height, wrap, filter, n, then 4 width height f32 decoded texels, then n x {s, t} f32
//                               OUT: n x 3 f32 tex (tex_lookup)
//   tex_harness checks          every host check of rpt_set_mesh_textures, in its order; the plan and the layout
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_tex.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int decode(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t n_gammas = 0, n_texels = 0;
    REQUIRE(fread(&n_gammas, 4, 1, f) == 1 && n_gammas > 0 && n_gammas < 64);
    std::vector<float> gammas(n_gammas);
    REQUIRE(fread(gammas.data(), 4, n_gammas, f) == n_gammas);
    REQUIRE(fread(&n_texels, 4, 1, f) == 1 && n_texels > 0);
    std::vector<uint8_t> bytes(4 * (size_t)n_texels);
    REQUIRE(fread(bytes.data(), 1, bytes.size(), f) == bytes.size());
    fclose(f);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    for (float g : gammas) {
        float L[256];
        for (uint32_t k = 0; k < 256u; ++k) L[k] = tex_decode_value(k, g);
        std::vector<TexTexel> out(n_texels, TexTexel{-1.0f, -1.0f, -1.0f, -1.0f});
        tex_decode_reference(bytes.data(), n_texels, g, out.data());
        REQUIRE(fwrite(L, 4, 256, f) == 256 && fwrite(out.data(), 16, n_texels, f) == n_texels);
    }
    fclose(f);
    printf("decode OK\n");
    return 0;
}

static int lookup(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[5];
    REQUIRE(fread(head, 4, 5, f) == 5);
    const uint32_t w = head[0], h = head[1], n = head[4];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    // exactly as many texels as the image has: a tap outside it is the address sanitizer's to find
    std::vector<TexTexel> texels((size_t)w * h);
    REQUIRE(fread(texels.data(), 16, texels.size(), f) == texels.size());
    std::vector<float> st(2 * (size_t)n), out(3 * (size_t)n);
    REQUIRE(n == 0 || fread(st.data(), 4, st.size(), f) == st.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) tex_lookup(texels.data(), w, h, head[2], head[3], st[2 * i], st[2 * i + 1], &out[3 * i]);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE(n == 0 || fwrite(out.data(), 4, out.size(), f) == out.size());
    fclose(f);
    printf("lookup OK\n");
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
    const std::vector<TexImage> none;
    std::vector<TexImage> image;
    std::string err;
    const float uv4[8] = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f, -1.5f, 2.5f};
    const float uv2[4] = {0.25f, 0.5f, 1048576.0f, -1048576.0f};
    const uint8_t px[4] = {1, 2, 3, 4};                              // (never read by the checks: any non-NULL pointer says "set")
    const auto item = [&](uint32_t mesh, uint32_t nv, const float* uvs, uint32_t w, uint32_t h) {
        rpt_mesh_texture it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.n_vertices = nv; it.uvs = uvs; it.width = w; it.height = h; it.texels = px;
        it.wrap = RPT_TEX_WRAP_CLAMP; it.filter = RPT_TEX_FILTER_BILINEAR; it.gamma = 2.2f;
        return it;
    };
    const auto run = [&](const rpt_mesh_texture* items, uint32_t n, const std::vector<TexImage>& cur = std::vector<TexImage>()) {
        return check_mesh_textures(plan, true, items, n, cur, image, err);
    };
    const auto says = [&](const char* what) { return err.find(what) != std::string::npos; };
    // no scene comes before everything else, then 2^32 vertices, then NULL items
    REQUIRE(check_mesh_textures(plan, false, nullptr, 1, none, image, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_textures: ") == 0);
    RefitPlan huge = plan;
    huge.ok = false;
    REQUIRE(check_mesh_textures(huge, true, nullptr, 1, none, image, err) == RPT_ERR_UNSUPPORTED && says("2^32"));
    REQUIRE(run(nullptr, 1) == RPT_ERR_INVALID_ARG && says("items is NULL"));
    REQUIRE(run(nullptr, 0) == RPT_OK && image.size() == 3 && !image[0].width && !image[2].width);
    // per item, in order; the first fault of the first faulty item answers
    rpt_mesh_texture good[2] = {item(0, 4, uv4, 3, 5), item(2, 2, uv2, 1, 1)};
    REQUIRE(run(good, 2) == RPT_OK && image[0].width == 3 && image[0].height == 5 && image[0].wrap == RPT_TEX_WRAP_CLAMP &&
            image[0].filter == RPT_TEX_FILTER_BILINEAR && image[0].gamma == 2.2f && !image[1].width && image[2].width == 1);
    rpt_mesh_texture bad[2] = {item(0, 4, uv4, 3, 5), item(3, 9, nullptr, 0, 99999)};
    bad[1].wrap = 7; bad[1].filter = 7; bad[1].gamma = -1.0f;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("item 1: mesh 3 out of range"));
    bad[1].mesh = 0;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("item 1: mesh 0 is named twice"));
    bad[1].mesh = 2;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("item 1: mesh 2: n_vertices 9"));
    bad[1].n_vertices = 2;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("mesh 2: uvs is NULL"));
    bad[1].uvs = uv2;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("a texture of 0 x 99999"));
    bad[1].width = 16385; bad[1].height = 1;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("a texture of 16385 x 1"));
    bad[1].width = 1; bad[1].height = 0;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("a texture of 1 x 0"));
    bad[1].height = 16384; bad[1].texels = nullptr;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("texels is NULL"));
    bad[1].texels = px;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("wrap 7"));
    bad[1].wrap = RPT_TEX_WRAP_REPEAT;
    REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("filter 7"));
    bad[1].filter = RPT_TEX_FILTER_NEAREST;
    const float gammas[6] = {-1.0f, 0.0f, 16.5f, INFINITY, -INFINITY, NAN};
    for (float g : gammas) {
        bad[1].gamma = g;
        REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("gamma"));
    }
    bad[1].gamma = 16.0f;
    REQUIRE(run(bad, 2) == RPT_OK && image[2].height == 16384 && image[2].gamma == 16.0f);
    const float bad_uvs[4][4] = {{0.0f, NAN, 0.0f, 0.0f}, {0.0f, 0.0f, INFINITY, 0.0f}, {0.0f, 0.0f, 0.0f, 1048577.0f}, {-1048580.0f, 0.0f, 0.0f, 0.0f}};
    const char* names[4] = {"vertex 0", "vertex 1", "vertex 1", "vertex 0"};
    for (int k = 0; k < 4; ++k) {
        bad[1].uvs = bad_uvs[k];
        REQUIRE(run(bad, 2) == RPT_ERR_INVALID_ARG && says("item 1: mesh 2") && says(names[k]) && says("2^20"));
    }
    // a mesh without vertices may be textured, with no uvs at all
    rpt_mesh_texture empty = item(1, 0, nullptr, 2, 2);
    REQUIRE(run(&empty, 1) == RPT_OK && image[1].width == 2);
    // removal: width == height == 0 and texels NULL; nothing else of the item is read
    rpt_mesh_texture rm = item(0, 77, nullptr, 0, 0);
    rm.texels = nullptr; rm.wrap = 9; rm.filter = 9; rm.gamma = NAN;
    std::vector<TexImage> current(3);
    current[0].width = 4; current[0].height = 4; current[2].width = 8; current[2].height = 2;
    REQUIRE(run(&rm, 1, current) == RPT_OK && !image[0].width && image[2].width == 8 && image[2].height == 2);      // meshes not named keep theirs
    // the 2^26 rule, with sizes only: after the items' own checks, over what the call would leave
    rpt_mesh_texture big[2] = {item(0, 4, uv4, 8192, 8192), item(2, 2, uv2, 1, 1)};
    REQUIRE(run(big, 1) == RPT_OK);                                  // exactly 2^26
    REQUIRE(run(big, 2) == RPT_ERR_UNSUPPORTED && says("2^26"));
    current[0] = TexImage(); current[2].width = 1; current[2].height = 1;
    REQUIRE(run(big, 1, current) == RPT_ERR_UNSUPPORTED && says("2^26"));    // (a texture kept from before counts)
    rpt_mesh_texture swap[2] = {item(0, 4, uv4, 8192, 8192), item(2, 0, nullptr, 0, 0)};
    swap[1].texels = nullptr;
    REQUIRE(run(swap, 2, current) == RPT_OK);                        // (one the call removes does not)
    big[1].gamma = NAN;
    REQUIRE(run(big, 2) == RPT_ERR_INVALID_ARG && says("gamma"));    // (an item's own fault comes first)
    REQUIRE(run(nullptr, 0, current) == RPT_OK && image[2].width == 1);
    // the plan and the layout
    REQUIRE(run(good, 2) == RPT_OK);
    std::vector<float> uvs;
    tex_merge_uvs(plan, good, 2, uvs);
    REQUIRE(uvs.size() == 12 && uvs[6] == -1.5f && uvs[7] == 2.5f && uvs[8] == 0.25f && uvs[11] == -1048576.0f);
    TexPlan tp;
    build_tex_plan(plan, image, uvs, tp);
    REQUIRE(tp.any() && tp.n_tex() == 2 && tp.tex_mesh[0] == 0 && tp.tex_mesh[1] == 2 && tp.n_texels == 16 && tp.image[2].first == 15);
    REQUIRE(tp.textured(0) && !tp.textured(1) && tp.textured(2) && !tp.textured(9) && tp.ordinal(2) == 1 && tp.ordinal(1) == kTexNone);
    REQUIRE(tp.tri_tex == std::vector<uint32_t>({0u, 0u, 1u}));
    REQUIRE(tp.desc.size() == 16 && tp.desc[0] == 0 && tp.desc[1] == 3 && tp.desc[2] == 5 && tp.desc[8] == 15 && tp.desc[9] == 1);
    REQUIRE(sizeof(TexDesc) == 4 * kTexDescWords && sizeof(TexTexel) == 16 && alignof(TexTexel) == 16);
    const TexLayout tl(tp.n_tex(), tp.n_tris, tp.n_vertices, tp.n_texels);
    REQUIRE(tl.off_desc == 0 && tl.off_tri_tex == 64 && tl.off_uvs == 80 && tl.off_flat_bits == 128 && tl.off_texels == 144 && tl.total == 144 + 256);
    rpt_mesh_texture rm2 = item(2, 0, nullptr, 0, 0);
    rm2.texels = nullptr;
    tex_merge_uvs(plan, &rm2, 1, uvs);
    REQUIRE(uvs[8] == 0.0f && uvs[11] == 0.0f && uvs[7] == 2.5f);
    REQUIRE(!TexPlan().any());
    // the pieces of the lookup at their ends
    REQUIRE(tex_wrap(-0x1p-30f, RPT_TEX_WRAP_REPEAT) == 1.0f && tex_wrap(-0x1p-30f, RPT_TEX_WRAP_CLAMP) == 0.0f && tex_wrap(1.0f, RPT_TEX_WRAP_REPEAT) == 0.0f);
    REQUIRE(tex_wrap(1048576.0f, RPT_TEX_WRAP_REPEAT) == 0.0f && tex_wrap(1048576.0f, RPT_TEX_WRAP_CLAMP) == 1.0f && tex_wrap(-2.25f, RPT_TEX_WRAP_REPEAT) == 0.75f);
    REQUIRE(tex_nearest_index(1.0f, 3, RPT_TEX_WRAP_REPEAT) == 0 && tex_nearest_index(1.0f, 3, RPT_TEX_WRAP_CLAMP) == 2 && tex_nearest_index(0.5f, 3, RPT_TEX_WRAP_CLAMP) == 1);
    uint32_t i0, i1;
    float fx;
    tex_bilinear_taps(0.0f, 4, RPT_TEX_WRAP_REPEAT, i0, i1, fx);
    REQUIRE(i0 == 3 && i1 == 0 && fx == 0.5f);
    tex_bilinear_taps(0.0f, 4, RPT_TEX_WRAP_CLAMP, i0, i1, fx);
    REQUIRE(i0 == 0 && i1 == 0 && fx == 0.5f);
    tex_bilinear_taps(1.0f, 4, RPT_TEX_WRAP_REPEAT, i0, i1, fx);
    REQUIRE(i0 == 3 && i1 == 0 && fx == 0.5f);
    tex_bilinear_taps(1.0f, 4, RPT_TEX_WRAP_CLAMP, i0, i1, fx);
    REQUIRE(i0 == 3 && i1 == 3);
    tex_bilinear_taps(0.5f, 1, RPT_TEX_WRAP_REPEAT, i0, i1, fx);
    REQUIRE(i0 == 0 && i1 == 0 && fx == 0.0f);
    REQUIRE(tex_decode_value(0, 2.2f) == 0.0f && tex_decode_value(255, 0.4545f) == 1.0f && tex_decode_value(51, 1.0f) == 0.2f);
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "decode")) return decode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "lookup")) return lookup(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: tex_harness decode IN OUT | lookup IN OUT | checks\n");
    return 2;
}
