// host_env.h — the host half of environment lighting (include/rpt.h, "environment lighting"): the statement of the lookup of a
// direction, of the table (weights, exponent, quanta, CDF) and of the sampler as plain functions, the checks of rpt_set_environment,
// the layout of every device's tables, and a host reference of the table.  Plain C++ with no HIP type in it, like host_light.h and
// host_tex.h: capi.hip includes it, k_env.hip compiles the RPT_ENV_FN functions for the device (dev_mesh_env.h calls them at the miss
// and in direct_light), and tests/env_harness.cpp runs this file under the address and undefined-behaviour sanitizers
// (tests/test_mesh_env_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off: each a*b + c below is one product and one add.
// The divide and the square root are the correctly rounded ones.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_map.h"

#ifndef RPT_ENV_FN
#define RPT_ENV_FN inline
#endif

namespace rpthost {

constexpr uint32_t kEnvNone = 0xFFFFFFFFu;
constexpr uint32_t kEnvMaxSize = 4096;
constexpr uint32_t kEnvScanBlock = 256;         // texels per workgroup of the scan (k_env.hip)
constexpr uint64_t kEnvMaxPick = 1ull << 24;    // the pickable lights stay below it: the index draw has 24 bits
constexpr float kEnvFMax = 3.40282347e+38f;
constexpr float kEnvMaxTexel = 1.2676506e+30f;  // 2^100

// A texel as the device holds it, 16 B: one gather at a miss.  q is (float)q_k (0 for a BACKGROUND_ONLY environment and for a dark
// table): what the miss weight needs of the CDF.
struct alignas(16) EnvTexel { float r, g, b, q; };

RPT_ENV_FN float env_sgn(float x) { return x >= 0.0f ? 1.0f : -1.0f; }

// w_k = (r + g) + b
RPT_ENV_FN float env_weight(float r, float g, float b) { return (r + g) + b; }

// E with w_max = f * 2^E, f in [0.5, 1), for every finite w_max > 0, subnormal ones included; w_max == 0 (a dark table): 0.
RPT_ENV_FN int32_t env_exponent(float w_max)
{
    uint32_t u;
    __builtin_memcpy(&u, &w_max, 4);
    if (u == 0u) return 0;
    const uint32_t field = (u >> 23) & 255u;
    if (field != 0u) return (int32_t)field - 126;
    return (31 - __builtin_clz(u & 0x7FFFFFu)) - 148;                // w_max = m * 2^-149, 2^b <= m < 2^(b+1): E = b - 148
}

// q_k = floor(w_k * 2^(36 - E)) — the product is exact in float64 (a 24-bit significand times a power of two within the range: E lies
// in [-148, 103]), and the conversion truncates a non-negative value below 2^36.
RPT_ENV_FN uint64_t env_quantum(float w, int32_t e)
{
    const uint64_t bits = (uint64_t)(1023 + 36 - e) << 52;
    double scale;
    __builtin_memcpy(&scale, &bits, 8);
    return (uint64_t)((double)w * scale);
}

// Lookup of a direction: the texel k of `d` in an S x S image, or kEnvNone; p = (px, d.y / l1, pz) BEFORE the fold (what the miss
// weight's pdf is evaluated for).
RPT_ENV_FN uint32_t env_texel_of(const float d[3], uint32_t size, float p[3])
{
    p[0] = 0.0f; p[1] = 0.0f; p[2] = 0.0f;
    const float l1 = (__builtin_fabsf(d[0]) + __builtin_fabsf(d[1])) + __builtin_fabsf(d[2]);
    if (!(l1 > 0.0f && l1 <= kEnvFMax)) return kEnvNone;
    float px = d[0] / l1, pz = d[2] / l1;
    p[0] = px; p[1] = d[1] / l1; p[2] = pz;
    if (d[1] < 0.0f) {
        const float fx = (1.0f - __builtin_fabsf(pz)) * env_sgn(px);
        const float fz = (1.0f - __builtin_fabsf(px)) * env_sgn(pz);
        px = fx; pz = fz;
    }
    const float s = px * 0.5f + 0.5f, t = pz * 0.5f + 0.5f;
    const float size_f = (float)size;
    int32_t i = (int32_t)__builtin_floorf(s * size_f), j = (int32_t)__builtin_floorf(t * size_f);
    if (i > (int32_t)size - 1) i = (int32_t)size - 1;
    if (j > (int32_t)size - 1) j = (int32_t)size - 1;
    if (i < 0) i = 0;                                               // (no part of the statement: s and t lie in [0, 1])
    if (j < 0) j = 0;
    return (uint32_t)j * size + (uint32_t)i;
}

// The point of the octahedron the sampler takes in texel k with the draws r1, r2 (after the fold; py as it was before it), and the
// direction towards it.
RPT_ENV_FN void env_sample_point(uint32_t k, uint32_t size, float r1, float r2, float p[3])
{
    const float size_f = (float)size;
    const uint32_t i = k % size, j = k / size;
    const float s = ((float)i + r1) / size_f, t = ((float)j + r2) / size_f;
    float px = s * 2.0f - 1.0f, pz = t * 2.0f - 1.0f;
    const float py = (1.0f - __builtin_fabsf(px)) - __builtin_fabsf(pz);
    if (py < 0.0f) {
        const float fx = (1.0f - __builtin_fabsf(pz)) * env_sgn(px);
        const float fz = (1.0f - __builtin_fabsf(px)) * env_sgn(pz);
        px = fx; pz = fz;
    }
    p[0] = px; p[1] = py; p[2] = pz;
}

// pdf = (sel * ((S_f * S_f) * 0.25f)) * (l2 * len), sel = q_f / Q_f: the sampler's and the miss weight's one function.  `len` (may
// be NULL) gets sqrt(l2).
RPT_ENV_FN float env_pdf(float q_f, float q_total_f, uint32_t size, const float p[3], float* len_out)
{
    const float size_f = (float)size;
    const float l2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const float len = __builtin_sqrtf(l2);
    if (len_out) *len_out = len;
    const float sel = q_f / q_total_f;
    return (sel * ((size_f * size_f) * 0.25f)) * (l2 * len);
}

// The high 64 bits of a * b, from 32-bit halves (the same on the host and on the device).
RPT_ENV_FN uint64_t env_mulhi(uint64_t a, uint64_t b)
{
    const uint64_t al = a & 0xFFFFFFFFull, ah = a >> 32, bl = b & 0xFFFFFFFFull, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xFFFFFFFFull) + (hl & 0xFFFFFFFFull);
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// The pick: J has 48 bits, T = (J * Q) >> 48 < Q, k = the first index with C_k > T.  Needs Q = cdf[n - 1] > 0.
RPT_ENV_FN uint32_t env_pick(const uint64_t* cdf, uint32_t n, float r0a, float r0b)
{
    const uint64_t j = ((uint64_t)(uint32_t)(r0a * 16777216.0f) << 24) | (uint64_t)(uint32_t)(r0b * 16777216.0f);
    const uint64_t t = env_mulhi(j << 16, cdf[n - 1u]);
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// The lookup of direction d as the miss exit makes it: the texel's index (kEnvNone: none), its radiance, and lp, the pdf the sampler
// has for this direction (0 where next-event estimation cannot produce it: q_total == 0 — BACKGROUND_ONLY or a dark table —, q_k == 0,
// no texel).
RPT_ENV_FN uint32_t env_lookup(const EnvTexel* texels, uint32_t size, uint64_t q_total, float q_total_f, float scale, const float d[3],
                               float radiance[3], float* lp)
{
    radiance[0] = 0.0f; radiance[1] = 0.0f; radiance[2] = 0.0f;
    *lp = 0.0f;
    float p[3];
    const uint32_t k = env_texel_of(d, size, p);
    if (k == kEnvNone) return k;
    const EnvTexel c = texels[k];                                   // one 16 B gather
    radiance[0] = c.r * scale; radiance[1] = c.g * scale; radiance[2] = c.b * scale;
    if (q_total != 0ull && c.q != 0.0f) *lp = env_pdf(c.q, q_total_f, size, p, nullptr);
    return k;
}

// The sampler with the draws r0a, r0b, r1, r2: the picked texel (kEnvNone: q_total == 0, and everything stays zero), the direction,
// the pdf and the emission N_f * (texel_k * scale) of the PICKED texel.
RPT_ENV_FN uint32_t env_sample(const EnvTexel* texels, const uint64_t* cdf, uint32_t size, uint64_t q_total, float q_total_f, float scale,
                               float n_f, float r0a, float r0b, float r1, float r2, float direction[3], float* pdf, float emission[3])
{
    direction[0] = 0.0f; direction[1] = 0.0f; direction[2] = 0.0f;
    emission[0] = 0.0f; emission[1] = 0.0f; emission[2] = 0.0f;
    *pdf = 0.0f;
    if (q_total == 0ull) return kEnvNone;
    const uint32_t k = env_pick(cdf, size * size, r0a, r0b);
    float p[3], len;
    env_sample_point(k, size, r1, r2, p);
    const EnvTexel c = texels[k];
    *pdf = env_pdf(c.q, q_total_f, size, p, &len);
    direction[0] = p[0] / len; direction[1] = p[1] / len; direction[2] = p[2] / len;
    emission[0] = n_f * (c.r * scale); emission[1] = n_f * (c.g * scale); emission[2] = n_f * (c.b * scale);
    return k;
}

// The device's environment tables (DevState::env), one allocation.  Per texel 16 B and, SAMPLED, 8 B (its CDF entry, the scan's
// partial sum before the last pass) plus 8 B per 256 texels (the scan's block sums); 16 B of scratch (the bits of W_max); per triangle
// of the SCENE 4 B (0xFFFFFFFF: the tri_light and tri_tex the render kernel reads while no mesh is ON or textured) and one bit (the
// all-FLAT smooth bits it reads while no mesh is SMOOTH).
struct EnvLayout {
    size_t off_texels = 0, off_cdf = 0, off_block = 0, off_head = 0, off_none = 0, off_flat_bits = 0, total = 0;
    uint32_t n_blocks = 0;
    EnvLayout(uint32_t size, bool sampled, uint32_t n_tris)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t n = (size_t)size * size;
        n_blocks = sampled ? (uint32_t)((n + kEnvScanBlock - 1) / kEnvScanBlock) : 0u;
        off_cdf = round16(16 * n);
        off_block = off_cdf + (sampled ? round16(8 * n) : 0);
        off_head = off_block + round16(8 * (size_t)n_blocks);
        off_none = off_head + 16;
        off_flat_bits = off_none + round16(4 * (size_t)n_tris);
        total = off_flat_bits + round16(4 * (((size_t)n_tris + 31) / 32));
    }
};

// What the context remembers of its environment (size == 0: none is set).
struct EnvPlan {
    uint32_t size = 0;
    uint32_t mode = RPT_ENV_BACKGROUND_ONLY;
    float scale = 0.0f;
    uint32_t n_tris = 0;                       // of the scene: the sizes of the empty tables of the absent features
    uint64_t q_total = 0;                      // Q as the devices computed it (0: BACKGROUND_ONLY, or the table is dark)
    int32_t exponent = 0;                      // E (0 then as well)

    bool any() const { return size != 0u; }
    bool sampled() const { return size != 0u && mode == RPT_ENV_SAMPLED; }
    uint32_t n_texels() const { return size * size; }
    EnvLayout layout() const { return EnvLayout(size, sampled(), n_tris); }     // of every device's tables
};

// `err` = "rpt_set_environment: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int env_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_environment", code, fmt, a...); }

// Every check of rpt_set_environment but the NULL context (include/rpt.h), in one fixed order.  `n_other`: the pickable lights
// without the environment (n_lights + ON meshes).  env == NULL (remove) passes once a mesh scene is uploaded.
inline int check_environment(bool mesh_scene, uint64_t n_other, const rpt_environment* env, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return env_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!env) return RPT_OK;
    if (env->size == 0u || env->size > kEnvMaxSize) return env_error(err, INVALID, "size %u is not in 1 .. %u", env->size, kEnvMaxSize);
    if (!env->texels) return env_error(err, INVALID, "texels is NULL");
    if (env->mode != RPT_ENV_BACKGROUND_ONLY && env->mode != RPT_ENV_SAMPLED)
        return env_error(err, INVALID, "mode %u is neither RPT_ENV_BACKGROUND_ONLY nor RPT_ENV_SAMPLED", env->mode);
    if (!(env->scale >= 0.0f && env->scale <= kEnvFMax)) return env_error(err, INVALID, "scale %g is not finite and >= 0", (double)env->scale);
    const size_t n = (size_t)env->size * env->size;
    for (size_t k = 0; k < n; ++k)
        for (size_t c = 0; c < 3; ++c) {
            const float v = env->texels[3 * k + c];
            if (!(v >= 0.0f && v <= kEnvMaxTexel))
                return env_error(err, INVALID, "texel %zu (column %zu, row %zu): component %zu is %g: not finite, negative or above 2^100", k,
                                 k % env->size, k / env->size, c, (double)v);
        }
    if (env->mode == RPT_ENV_SAMPLED && n_other + 1u >= kEnvMaxPick)
        return env_error(err, RPT_ERR_UNSUPPORTED, "%llu lights and ON meshes and the environment: the pickable lights must stay below 2^24",
                         (unsigned long long)n_other);
    return RPT_OK;
}

// ---- the host reference: what k_env.hip's table kernels compute, statement for statement -------------------------------------------
// `texels`: size*size*3 f32; `out`: size*size texels; `cdf` (NULL for BACKGROUND_ONLY): size*size entries.
inline void env_table_reference(const float* texels, uint32_t size, bool sampled, EnvTexel* out, uint64_t* cdf, int32_t* exponent)
{
    const size_t n = (size_t)size * size;
    float w_max = 0.0f;
    for (size_t k = 0; k < n; ++k) {
        const float w = env_weight(texels[3 * k], texels[3 * k + 1], texels[3 * k + 2]);
        out[k] = EnvTexel{texels[3 * k], texels[3 * k + 1], texels[3 * k + 2], 0.0f};
        if (w > w_max) w_max = w;
    }
    *exponent = 0;
    if (!sampled) return;
    const int32_t e = env_exponent(w_max);
    uint64_t sum = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t q = w_max > 0.0f ? env_quantum(env_weight(out[k].r, out[k].g, out[k].b), e) : 0ull;
        out[k].q = (float)q;
        sum += q;
        cdf[k] = sum;
    }
    *exponent = w_max > 0.0f ? e : 0;
}

}  // namespace rpthost
