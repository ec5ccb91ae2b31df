// cut_harness.cpp — csrc/host_cut.h on the host, under the address and undefined-behaviour sanitizers
// (tests/test_mesh_cutout_host.py).
//
//   cut_harness mask IN OUT     IN:  u32 width, height, threshold, then width height bytes of alpha
//                               OUT: cut_mask_words(width, height) u32 (cut_mask_reference)
//   cut_harness lookup IN OUT   IN:  u32 width, height, wrap, n, then 6 f32 {sa, ta, sb, tb, sc, tc}, then n x {u, v} f32
//                               OUT: n u32 (cut_texel)
//   cut_harness checks          every host check of rpt_set_mesh_cutouts, in its order; the plan, the layout and the descriptors
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_cut.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int mask(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[3];
    REQUIRE(fread(head, 4, 3, f) == 3);
    const uint32_t w = head[0], h = head[1];
    REQUIRE(w > 0 && h > 0 && w <= kTexMaxSide && h <= kTexMaxSide);
    // exactly as many bytes and words as the mask has: anything outside is the address sanitizer's to find
    std::vector<uint8_t> alpha((size_t)w * h);
    REQUIRE(fread(alpha.data(), 1, alpha.size(), f) == alpha.size());
    fclose(f);
    std::vector<uint32_t> words(cut_mask_words(w, h), 0xA5A5A5A5u);
    cut_mask_reference(alpha.data(), w, h, head[2], words.data());
    for (size_t k = 0; k < alpha.size(); ++k) REQUIRE(cut_bit(words.data(), (uint32_t)k) == (alpha[k] >= head[2]));
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE(fwrite(words.data(), 4, words.size(), f) == words.size());
    fclose(f);
    printf("mask OK\n");
    return 0;
}

static int lookup(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[4];
    float uv[6];
    REQUIRE(fread(head, 4, 4, f) == 4 && fread(uv, 4, 6, f) == 6);
    const uint32_t w = head[0], h = head[1], n = head[3];
    REQUIRE(w > 0 && h > 0);
    std::vector<float> in(2 * (size_t)n);
    std::vector<uint32_t> out(n);
    REQUIRE(n == 0 || fread(in.data(), 4, in.size(), f) == in.size());
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        out[i] = cut_texel(in[2 * i], in[2 * i + 1], uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], w, h, head[2]);
        REQUIRE(out[i] < w * h);
    }
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE(n == 0 || fwrite(out.data(), 4, out.size(), f) == out.size());
    fclose(f);
    printf("lookup OK\n");
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
    LightPlan dark, lit;
    lit.mode = {(uint8_t)RPT_MESH_LIGHT_ON, (uint8_t)RPT_MESH_LIGHT_OFF, (uint8_t)RPT_MESH_LIGHT_OFF};
    const std::vector<CutMask> none;
    std::vector<CutMask> mask;
    std::string err;
    const uint8_t px[4] = {1, 2, 3, 4};                              // (never read by the checks: any non-NULL pointer says "set")
    const auto on = [&](uint32_t mesh, uint32_t w, uint32_t h, uint32_t threshold = 128u) {
        rpt_mesh_cutout it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_CUTOUT_ON; it.width = w; it.height = h; it.alpha = px; it.threshold = threshold;
        return it;
    };
    const auto off = [&](uint32_t mesh) {
        rpt_mesh_cutout it;
        memset(&it, 0, sizeof(it));
        it.mesh = mesh; it.mode = RPT_MESH_CUTOUT_OFF;
        return it;
    };
    const auto run = [&](const rpt_mesh_cutout* items, uint32_t n, const std::vector<CutMask>& cur = std::vector<CutMask>(), const LightPlan* lp = nullptr) {
        return check_mesh_cutouts(plan, true, tex, lp ? *lp : dark, items, n, cur, mask, err);
    };
    const auto says = [&](const char* what) { return err.find(what) != std::string::npos; };
    const int INVALID = RPT_ERR_INVALID_ARG;
    // 2, 3: no scene comes before everything else, then NULL items
    REQUIRE(check_mesh_cutouts(plan, false, tex, dark, nullptr, 1, none, mask, err) == RPT_ERR_NO_SCENE && err.find("rpt_set_mesh_cutouts: ") == 0);
    REQUIRE(run(nullptr, 1) == INVALID && says("items is NULL") && err.find("rpt_set_mesh_cutouts: ") == 0);
    REQUIRE(run(nullptr, 0) == RPT_OK && mask.size() == 3 && !mask[0].width && !mask[2].width);
    rpt_mesh_cutout good[2] = {on(0, 5, 3, 1), on(2, 33, 7, 255)};
    REQUIRE(run(good, 2) == RPT_OK && mask[0].width == 5 && mask[0].height == 3 && mask[0].threshold == 1 && !mask[1].width && mask[2].width == 33 &&
            mask[2].threshold == 255);
    const std::vector<CutMask> held = mask;
    // per item, in order: the first fault of the first faulty item answers.  Each case carries the NEXT check's fault as well.
    rpt_mesh_cutout it[2];
    it[0] = on(3, 0, 0, 0); it[0].mode = 7;                          // 4 before 5
    REQUIRE(run(it, 1) == INVALID && says("mesh 3 out of range"));
    it[0] = on(0, 2, 2); it[1] = on(0, 0, 0, 0); it[1].mode = 7;      // 4 (twice) before 5
    REQUIRE(run(it, 2) == INVALID && says("item 1: mesh 0 is named twice"));
    it[0] = on(0, 0, 2); it[0].mode = 2;                             // 5 before 6
    REQUIRE(run(it, 1) == INVALID && says("mode 2"));
    it[0] = on(0, 0, 2); it[0].alpha = nullptr;                      // 6 before 7
    REQUIRE(run(it, 1) == INVALID && says("a mask of 0 x 2"));
    it[0] = on(0, 2, 16385); it[0].alpha = nullptr;
    REQUIRE(run(it, 1) == INVALID && says("a mask of 2 x 16385"));
    it[0] = on(0, 2, 2, 0); it[0].alpha = nullptr;                   // 7 before 8
    REQUIRE(run(it, 1) == INVALID && says("alpha is NULL"));
    it[0] = on(1, 2, 2, 0);                                          // 8 before 10 (mesh 1 is untextured)
    REQUIRE(run(it, 1) == INVALID && says("threshold 0"));
    it[0] = on(1, 2, 2, 256);
    REQUIRE(run(it, 1) == INVALID && says("threshold 256"));
    it[0] = off(0); it[0].width = 1;                                 // 9
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_CUTOUT_OFF takes"));
    it[0] = off(0); it[0].alpha = px;
    REQUIRE(run(it, 1) == INVALID && says("RPT_MESH_CUTOUT_OFF takes"));
    it[0] = on(1, 2, 2);                                             // 10
    REQUIRE(run(it, 1) == INVALID && says("mesh 1 is untextured") && says("1 x 1 white texture"));
    {                                                                // 10 before 11: an untextured mesh light
        LightPlan both;
        both.mode = {(uint8_t)RPT_MESH_LIGHT_OFF, (uint8_t)RPT_MESH_LIGHT_ON, (uint8_t)RPT_MESH_LIGHT_OFF};
        REQUIRE(run(it, 1, none, &both) == INVALID && says("untextured"));
    }
    it[0] = on(0, 16384, 16384);                                     // 11 before 12
    REQUIRE(run(it, 1, none, &lit) == RPT_ERR_UNSUPPORTED && says("mesh 0 is a mesh light"));
    it[0] = on(2, 2, 2);
    REQUIRE(run(it, 1, none, &lit) == RPT_OK);                       // (another mesh of that scene may have one)
    it[0] = on(0, 8192, 8192); it[1] = on(2, 1, 1);                   // 12: 2^26 + 1
    REQUIRE(run(it, 2) == RPT_ERR_UNSUPPORTED && says("2^26"));
    it[0] = on(0, 8192, 8192);
    REQUIRE(run(it, 1) == RPT_OK);                                   // exactly 2^26
    REQUIRE(run(it, 1, held) == RPT_ERR_UNSUPPORTED && says("2^26"));     // mesh 2 keeps its 33 x 7
    // a rejected call leaves `mask` alone; OFF removes; a mesh not named keeps its mask
    mask = held;
    it[0] = on(1, 2, 2);
    REQUIRE(run(it, 1, held) == INVALID && mask.size() == 3 && mask[0].width == 5 && mask[2].width == 33);
    it[0] = off(0);
    REQUIRE(run(it, 1, held) == RPT_OK && !mask[0].width && mask[2].width == 33 && mask[2].height == 7 && mask[2].threshold == 255);
    it[0] = off(1);                                                  // removing what is not there (even from an untextured mesh) is no error
    REQUIRE(run(it, 1, held) == RPT_OK && mask[0].width == 5);
    // the plan, the layout, the descriptors
    REQUIRE(cut_mask_words(1, 1) == 4 && cut_mask_words(5, 3) == 4 && cut_mask_words(33, 7) == 8 && cut_mask_words(64, 64) == 128 &&
            cut_mask_words(16, 8) == 4 && cut_mask_words(129, 1) == 8 && cut_mask_words(16384, 4096) == (1u << 21));
    CutPlan cp;
    build_cut_plan(plan, held, cp);
    REQUIRE(cp.any() && cp.on(0) && !cp.on(1) && cp.on(2) && !cp.on(3) && cp.n_meshes == 3 && cp.n_tris == 3);
    REQUIRE(cp.mask[0].first == 0 && cp.mask[2].first == 4 && cp.n_words == 12);
    const CutLayout cl(cp.n_meshes, cp.n_tris, cp.n_words);
    REQUIRE(cl.off_desc == 0 && cl.off_none == 48 && cl.off_bits == 64 && cl.total == 64 + 48 && sizeof(CutDesc) == 16);
    REQUIRE((4 * cp.mask[2].first) % 16 == 0);
    const std::vector<uint32_t> d = cut_desc_table(cp, tex);
    const std::vector<uint32_t> want = {0u, 5u, 3u, 1u, 4u, 33u, 7u, 3u, 0u, 0u, 0u, 0u};     // by texture ordinal; mesh 2 is CLAMP
    REQUIRE(d == want);
    {                                                                // the texture of mesh 0 replaced by a CLAMP one and mesh 1 textured: ordinals move, masks do not
        std::vector<TexImage> image(3);
        for (TexImage& im : image) { im.width = 2; im.height = 2; im.wrap = RPT_TEX_WRAP_CLAMP; }
        TexPlan t3;
        build_tex_plan(plan, image, std::vector<float>(), t3);
        const std::vector<uint32_t> d3 = cut_desc_table(cp, t3);
        const std::vector<uint32_t> want3 = {0u, 5u, 3u, 3u, 0u, 0u, 0u, 0u, 4u, 33u, 7u, 3u};
        REQUIRE(d3 == want3);
    }
    CutPlan empty;
    build_cut_plan(plan, none, empty);
    REQUIRE(!empty.any() && empty.n_words == 0 && empty.mask.size() == 3);
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "mask")) return mask(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "lookup")) return lookup(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    fprintf(stderr, "usage: cut_harness mask IN OUT | lookup IN OUT | checks\n");
    return 2;
}
