// env_harness.cpp — csrc/host_env.h on the host, under the address and undefined-behaviour sanitizers
// (tests/test_mesh_env_host.py).
//
//   env_harness table IN OUT    IN:  u32 size, sampled, then 3 size^2 f32 texels
//                               OUT: 4 size^2 f32 {r, g, b, (float)q_k}, size^2 u64 C_k (zeros: BACKGROUND_ONLY), i32 E
//                                    (env_table_reference)
//   env_harness lookup IN OUT   IN:  u32 size, sampled, n, f32 scale, 3 size^2 f32 texels, then n x 3 f32 directions
//                               OUT: n x {u32 k, f32 p[3] (env_texel_of), f32 radiance[3], f32 lp (env_lookup)}
//   env_harness sample IN OUT   IN:  u32 size, n, f32 scale, n_f, 3 size^2 f32 texels, then n x {r0a, r0b, r1, r2} f32
//                               OUT: n x {u32 k, f32 direction[3], f32 pdf, f32 emission[3]} (env_sample over the SAMPLED table)
//   env_harness checks          every host check of rpt_set_environment, in its order; the exponent; the layout
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_env.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// exactly as many entries as the image has: an index outside it is the address sanitizer's to find
struct Table {
    uint32_t size = 0;
    std::vector<EnvTexel> texels;
    std::vector<uint64_t> cdf;
    int32_t exponent = 0;
    uint64_t q() const { return cdf.empty() ? 0ull : cdf.back(); }
};

static bool read_table(FILE* f, uint32_t size, bool sampled, Table& t)
{
    if (size == 0 || size > kEnvMaxSize) return false;
    const size_t n = (size_t)size * size;
    std::vector<float> raw(3 * n);
    if (fread(raw.data(), 4, raw.size(), f) != raw.size()) return false;
    t.size = size;
    t.texels.assign(n, EnvTexel{-1.0f, -1.0f, -1.0f, -1.0f});
    t.cdf.assign(sampled ? n : 0, ~0ull);
    env_table_reference(raw.data(), size, sampled, t.texels.data(), sampled ? t.cdf.data() : nullptr, &t.exponent);
    return true;
}

static int table(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[2];
    REQUIRE(fread(head, 4, 2, f) == 2);
    Table t;
    REQUIRE(read_table(f, head[0], head[1] != 0, t));
    fclose(f);
    const size_t n = t.texels.size();
    std::vector<uint64_t> cdf(t.cdf);
    cdf.resize(n, 0ull);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    REQUIRE(fwrite(t.texels.data(), 16, n, f) == n && fwrite(cdf.data(), 8, n, f) == n && fwrite(&t.exponent, 4, 1, f) == 1);
    fclose(f);
    printf("table OK\n");
    return 0;
}

static int lookup(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[3];
    float scale;
    REQUIRE(fread(head, 4, 3, f) == 3 && fread(&scale, 4, 1, f) == 1);
    Table t;
    REQUIRE(read_table(f, head[0], head[1] != 0, t));
    const uint32_t n = head[2];
    std::vector<float> dirs(3 * (size_t)n);
    REQUIRE(fread(dirs.data(), 4, dirs.size(), f) == dirs.size());
    fclose(f);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    for (uint32_t i = 0; i < n; ++i) {
        float p[3], rad[3], lp;
        const uint32_t k = env_texel_of(&dirs[3 * (size_t)i], t.size, p);
        const uint32_t k2 = env_lookup(t.texels.data(), t.size, t.q(), (float)t.q(), scale, &dirs[3 * (size_t)i], rad, &lp);
        REQUIRE(k == k2);
        REQUIRE(fwrite(&k, 4, 1, f) == 1 && fwrite(p, 4, 3, f) == 3 && fwrite(rad, 4, 3, f) == 3 && fwrite(&lp, 4, 1, f) == 1);
    }
    fclose(f);
    printf("lookup OK\n");
    return 0;
}

static int sample(const char* in_path, const char* out_path)
{
    FILE* f = fopen(in_path, "rb");
    REQUIRE(f);
    uint32_t head[2];
    float par[2];
    REQUIRE(fread(head, 4, 2, f) == 2 && fread(par, 4, 2, f) == 2);
    Table t;
    REQUIRE(read_table(f, head[0], true, t));
    const uint32_t n = head[1];
    std::vector<float> draws(4 * (size_t)n);
    REQUIRE(fread(draws.data(), 4, draws.size(), f) == draws.size());
    fclose(f);
    f = fopen(out_path, "wb");
    REQUIRE(f);
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = &draws[4 * (size_t)i];
        float dir[3], em[3], pdf;
        const uint32_t k = env_sample(t.texels.data(), t.cdf.data(), t.size, t.q(), (float)t.q(), par[0], par[1], r[0], r[1], r[2], r[3], dir, &pdf, em);
        REQUIRE(fwrite(&k, 4, 1, f) == 1 && fwrite(dir, 4, 3, f) == 3 && fwrite(&pdf, 4, 1, f) == 1 && fwrite(em, 4, 3, f) == 3);
    }
    fclose(f);
    printf("sample OK\n");
    return 0;
}

static int checks()
{
    std::string err;
    std::vector<float> img(3 * 4, 0.25f);
    rpt_environment env{2u, img.data(), 1.0f, RPT_ENV_SAMPLED};
    const auto run = [&](bool mesh, uint64_t other, const rpt_environment* e) { err.clear(); return check_environment(mesh, other, e, err); };
    // the order: the scene first, then the fields in the order of the struct's statement, then the 2^24 rule
    REQUIRE(run(true, 0, &env) == RPT_OK && err.empty());
    REQUIRE(run(true, 0, nullptr) == RPT_OK);
    REQUIRE(run(false, 0, nullptr) == RPT_ERR_NO_SCENE);
    rpt_environment bad = env;
    bad.size = 0; bad.texels = nullptr; bad.mode = 7u; bad.scale = -1.0f;
    REQUIRE(run(false, kEnvMaxPick, &bad) == RPT_ERR_NO_SCENE && err.find("rpt_set_environment: ") == 0);
    REQUIRE(run(true, kEnvMaxPick, &bad) == RPT_ERR_INVALID_ARG && err.find("size 0") != std::string::npos);
    bad.size = 4097;
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("size 4097") != std::string::npos);
    bad.size = 2;
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("texels is NULL") != std::string::npos);
    bad.texels = img.data();
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("mode 7") != std::string::npos);
    bad.mode = RPT_ENV_BACKGROUND_ONLY;
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("scale") != std::string::npos);
    bad.scale = std::numeric_limits<float>::infinity();
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("scale") != std::string::npos);
    bad.scale = std::nanf("");
    REQUIRE(run(true, 0, &bad) == RPT_ERR_INVALID_ARG && err.find("scale") != std::string::npos);
    bad.scale = 0.0f;
    REQUIRE(run(true, 0, &bad) == RPT_OK);
    const float wrong[4] = {-1e-30f, std::nanf(""), std::numeric_limits<float>::infinity(), 1.3e30f};
    for (float w : wrong) {
        img[3 * 2 + 1] = w;
        REQUIRE(run(true, kEnvMaxPick, &env) == RPT_ERR_INVALID_ARG && err.find("texel 2 (column 0, row 1): component 1") != std::string::npos);
        img[3 * 2 + 1] = 0.25f;
    }
    img[5] = 1.2676506e+30f;                                        // 2^100 itself is legal
    REQUIRE(run(true, 0, &env) == RPT_OK);
    img[5] = 0.25f;
    // the 2^24 rule: SAMPLED only, and after everything else
    REQUIRE(run(true, kEnvMaxPick - 2, &env) == RPT_OK);
    REQUIRE(run(true, kEnvMaxPick - 1, &env) == RPT_ERR_UNSUPPORTED && err.find("2^24") != std::string::npos);
    env.mode = RPT_ENV_BACKGROUND_ONLY;
    REQUIRE(run(true, kEnvMaxPick - 1, &env) == RPT_OK);
    // the exponent: W_max = f * 2^E with f in [0.5, 1), subnormal values included
    REQUIRE(env_exponent(0.0f) == 0 && env_exponent(1.0f) == 1 && env_exponent(0.75f) == 0 && env_exponent(0.5f) == 0 && env_exponent(3.0f) == 2);
    const float tiny[3] = {1.4e-45f, 2.8e-45f, 1.1754942e-38f};     // 2^-149, 2^-148, the largest subnormal
    REQUIRE(env_exponent(tiny[0]) == -148 && env_exponent(tiny[1]) == -147 && env_exponent(tiny[2]) == -126);
    REQUIRE(env_exponent(1.17549435e-38f) == -125);
    for (float w : {1.4e-45f, 3.0e-40f, 1.0f, 3.8e30f}) {
        const uint64_t q = env_quantum(w, env_exponent(w));
        REQUIRE(q >= (1ull << 35) && q < (1ull << 36));
    }
    REQUIRE(env_mulhi(~0ull, ~0ull) == ~0ull - 1 && env_mulhi(1ull << 63, 6) == 3 && env_mulhi(0x123456789ABCDEFull, 0) == 0);
    // the layout: nothing overlaps, BACKGROUND_ONLY holds no CDF
    const EnvLayout a(17, true, 100), b(17, false, 100);
    REQUIRE(a.off_cdf >= 16u * 289u && a.off_block >= a.off_cdf + 8u * 289u && a.n_blocks == 2 && a.off_head >= a.off_block + 16u);
    REQUIRE(a.off_none == a.off_head + 16u && a.off_flat_bits >= a.off_none + 400u && a.total >= a.off_flat_bits + 16u);
    REQUIRE(b.off_block == b.off_cdf && b.n_blocks == 0 && b.total < a.total);
    printf("checks OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "table")) return table(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "lookup")) return lookup(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "sample")) return sample(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
    printf("usage: env_harness table|lookup|sample IN OUT | checks\n");
    return 2;
}
