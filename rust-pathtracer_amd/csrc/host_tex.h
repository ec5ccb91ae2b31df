// host_tex.h — the host half of mesh textures (include/rpt.h, "mesh textures"): the statement of the decode and of the lookup as plain
// functions, the plan rpt_set_mesh_textures makes (the textured meshes in ascending mesh order, where each one's texels lie, what
// every device gets), its checks, and a host reference of decode and lookup.  Plain C++ with no HIP type in it, like host_light.h:
// capi.hip includes it, k_tex.hip compiles the RPT_TEX_FN functions for the device (dev_mesh_tex.h calls them at the hit), and
// tests/tex_harness.cpp runs this file under the address and undefined-behaviour sanitizers (tests/test_mesh_texture_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off: each a*b + c*d below is two products and one add.
// The divide is the correctly rounded one (RPT_TEX_DIV: the host's `/`, the device's fdiv), the power is rpt_powf of
// include/rpt_strict_math.h.
//
// Numbering.  The textured meshes in ascending mesh index are ORDINALS 0 .. n_tex - 1; their decoded images lie one after the other
// in one texel table.  Nothing here knows a slot: a rebuild leaves every table bit for bit.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "../../include/rpt_strict_math.h"
#include "host_map.h"
#include "host_refit.h"

#ifndef RPT_TEX_FN
#define RPT_TEX_FN inline
#endif
#ifndef RPT_TEX_DIV
#define RPT_TEX_DIV(n, d) ((n) / (d))
#endif

namespace rpthost {

constexpr uint32_t kTexNone = 0xFFFFFFFFu;
constexpr uint32_t kTexDescWords = 8;           // TexDesc below, as words
constexpr uint32_t kTexMaxSide = kMapMaxSide;
constexpr uint64_t kTexMaxTexels = 1ull << 26;  // of all textures of a scene
constexpr float kTexMaxUv = 1048576.0f;         // 2^20: floorf and the casts of the lookup stay exact

// A decoded texel, 16 B: one gather per filter tap.  (a is 0: alpha is ignored.)
struct alignas(16) TexTexel { float r, g, b, a; };

// One textured mesh, 32 B.
struct TexDesc {
    uint32_t first;                   // its first texel in the texel table
    uint32_t width, height;
    uint32_t wrap, filter;            // RPT_TEX_WRAP_*, RPT_TEX_FILTER_*
    uint32_t pad[3];
};

// L[k] of include/rpt.h, "decode": the linear value of byte k.  The end points are by definition.
RPT_TEX_FN float tex_decode_value(uint32_t k, float gamma)
{
    const float x = RPT_TEX_DIV((float)k, 255.0f);
    if (gamma == 1.0f) return x;
    if (k == 0u) return 0.0f;
    if (k == 255u) return 1.0f;
    return rpt_powf(x, gamma);
}

// s (or t) at the hit: w = (1 - u) - v is the caller's; (w*sa + u*sb) + v*sc.
RPT_TEX_FN float tex_interp(float w, float u, float v, float sa, float sb, float sc) { return (w * sa + u * sb) + v * sc; }

// One axis' wrap: x in [0, 1] (1.0 is reached by rounding for a tiny negative s, and is legal).
RPT_TEX_FN float tex_wrap(float s, uint32_t wrap)
{
    if (wrap == RPT_TEX_WRAP_CLAMP) return s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    return s - __builtin_floorf(s);
}

// One axis of NEAREST: the texel index.  The last line is no part of the statement: it holds for every finite s within the UV
// bound, and keeps an index that a NaN produced inside the table.
RPT_TEX_FN uint32_t tex_nearest_index(float x, uint32_t n, uint32_t wrap)
{
    int32_t i = (int32_t)__builtin_floorf(x * (float)n);
    if (wrap == RPT_TEX_WRAP_CLAMP) { if (i > (int32_t)n - 1) i = (int32_t)n - 1; }
    else if (i == (int32_t)n) i = 0;
    return (uint32_t)i < n ? (uint32_t)i : 0u;
}

// One axis of BILINEAR: the two texel indices and the weight of the second.
RPT_TEX_FN void tex_bilinear_taps(float x, uint32_t n, uint32_t wrap, uint32_t& i0, uint32_t& i1, float& f)
{
    const float p = x * (float)n - 0.5f;
    const float f0 = __builtin_floorf(p);
    f = p - f0;
    int32_t a = (int32_t)f0;
    int32_t b = a + 1;
    if (wrap == RPT_TEX_WRAP_CLAMP) {
        if (a < 0) a = 0;
        if (b > (int32_t)n - 1) b = (int32_t)n - 1;
    } else {
        if (a < 0) a += (int32_t)n;
        if (b >= (int32_t)n) b -= (int32_t)n;
    }
    i0 = (uint32_t)a < n ? (uint32_t)a : 0u;                        // (as tex_nearest_index: never taken within the UV bound)
    i1 = (uint32_t)b < n ? (uint32_t)b : 0u;
}

// tex of include/rpt.h, "lookup at the hit": `texels` is the image's first texel, row 0 first.
RPT_TEX_FN void tex_lookup(const TexTexel* texels, uint32_t width, uint32_t height, uint32_t wrap, uint32_t filter, float s, float t, float out[3])
{
    const float x = tex_wrap(s, wrap), y = tex_wrap(t, wrap);
    if (filter == RPT_TEX_FILTER_NEAREST) {
        const uint32_t i = tex_nearest_index(x, width, wrap), j = tex_nearest_index(y, height, wrap);
        const TexTexel c = texels[(size_t)j * width + i];
        out[0] = c.r; out[1] = c.g; out[2] = c.b;
        return;
    }
    uint32_t i0, i1, j0, j1;
    float fx, fy;
    tex_bilinear_taps(x, width, wrap, i0, i1, fx);
    tex_bilinear_taps(y, height, wrap, j0, j1, fy);
    const TexTexel c00 = texels[(size_t)j0 * width + i0], c10 = texels[(size_t)j0 * width + i1];
    const TexTexel c01 = texels[(size_t)j1 * width + i0], c11 = texels[(size_t)j1 * width + i1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float top_r = gx * c00.r + fx * c10.r, top_g = gx * c00.g + fx * c10.g, top_b = gx * c00.b + fx * c10.b;
    const float bot_r = gx * c01.r + fx * c11.r, bot_g = gx * c01.g + fx * c11.g, bot_b = gx * c01.b + fx * c11.b;
    out[0] = gy * top_r + fy * bot_r;
    out[1] = gy * top_g + fy * bot_g;
    out[2] = gy * top_b + fy * bot_b;
}

// The host reference of the decode kernel: `texels` (RGBA8, width*height*4 bytes) -> `out` (width*height texels).
inline void tex_decode_reference(const uint8_t* texels, size_t n_texels, float gamma, TexTexel* out)
{
    float L[256];
    for (uint32_t k = 0; k < 256u; ++k) L[k] = tex_decode_value(k, gamma);
    for (size_t i = 0; i < n_texels; ++i) out[i] = TexTexel{L[texels[4 * i]], L[texels[4 * i + 1]], L[texels[4 * i + 2]], 0.0f};
}

// One mesh's texture as the context remembers it (width == 0: the mesh is untextured).
struct TexImage {
    uint32_t width = 0, height = 0, wrap = 0, filter = 0;
    float gamma = 1.0f;
    uint64_t first = 0;               // its first texel in the devices' texel table
};

// The device's texture tables (DevState::tex), one allocation.  Per textured mesh 32 B; per triangle of the SCENE 4 B (which
// texture) and one bit (the all-FLAT smooth bits the render kernel reads while no mesh is SMOOTH or ON); per vertex of the scene 8 B
// (its UV); per texel 16 B.
struct TexLayout {
    size_t off_desc = 0, off_tri_tex = 0, off_uvs = 0, off_flat_bits = 0, off_texels = 0, total = 0;
    TexLayout(uint32_t n_tex, uint32_t n_tris, uint32_t n_vertices, uint64_t n_texels)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_tri_tex = round16(4 * (size_t)kTexDescWords * n_tex);
        off_uvs = off_tri_tex + round16(4 * (size_t)n_tris);
        off_flat_bits = off_uvs + round16(8 * (size_t)n_vertices);
        off_texels = off_flat_bits + round16(4 * (((size_t)n_tris + 31) / 32));
        total = off_texels + 16 * (size_t)n_texels;
    }
};

// What rpt_set_mesh_textures leaves on the host for the life of the textures, and (the staging vectors) what every device gets.
struct TexPlan {
    std::vector<TexImage> image;               // mesh -> its texture; empty: no mesh is textured
    std::vector<float> uvs;                    // 2 per concatenated vertex of the scene (zeros for untextured meshes); kept: a later
                                               // call that names other meshes sends the whole table again
    uint32_t n_tris = 0, n_vertices = 0;
    uint64_t n_texels = 0;
    std::vector<uint32_t> tex_mesh;            // ordinal -> mesh, ascending
    // staging: released once every device holds it
    std::vector<uint32_t> desc;                // kTexDescWords per ordinal
    std::vector<uint32_t> tri_tex;             // flattened triangle -> its mesh's ordinal, or kTexNone

    uint32_t n_tex() const { return (uint32_t)tex_mesh.size(); }
    bool textured(uint32_t mesh) const { return mesh < image.size() && image[mesh].width != 0u; }
    bool any() const
    {
        for (const TexImage& im : image) if (im.width != 0u) return true;
        return false;
    }
    uint32_t ordinal(uint32_t mesh) const
    {
        for (uint32_t j = 0; j < n_tex(); ++j) if (tex_mesh[j] == mesh) return j;
        return kTexNone;
    }
    void release_staging()
    {
        std::vector<uint32_t>().swap(desc);
        std::vector<uint32_t>().swap(tri_tex);
    }
    TexLayout layout() const { return TexLayout(n_tex(), n_tris, n_vertices, n_texels); }     // of every device's tables
};

// The plan of `image` (one entry per mesh, `first` not yet set) and `uvs` over a scene: ordinals, texel offsets, descriptors and the
// triangles' lookup.
inline void build_tex_plan(const RefitPlan& plan, std::vector<TexImage> image, std::vector<float> uvs, TexPlan& tp)
{
    tp = TexPlan();
    tp.image = std::move(image);
    tp.uvs = std::move(uvs);
    tp.n_tris = plan.n_slots;
    tp.n_vertices = plan.n_vertices();
    tp.uvs.resize(2 * (size_t)tp.n_vertices, 0.0f);
    tp.tri_tex.assign(tp.n_tris, kTexNone);
    for (uint32_t m = 0; m < plan.n_meshes() && m < tp.image.size(); ++m) {
        TexImage& im = tp.image[m];
        if (im.width == 0u) continue;
        const uint32_t j = tp.n_tex();
        tp.tex_mesh.push_back(m);
        im.first = tp.n_texels;
        tp.n_texels += (uint64_t)im.width * im.height;
        const uint32_t d[kTexDescWords] = {(uint32_t)im.first, im.width, im.height, im.wrap, im.filter, 0u, 0u, 0u};
        tp.desc.insert(tp.desc.end(), d, d + kTexDescWords);
        for (uint32_t k = plan.tri_first[m]; k < plan.tri_first[m + 1u]; ++k) tp.tri_tex[k] = j;
    }
}

// `err` = "rpt_set_mesh_textures: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int tex_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_mesh_textures", code, fmt, a...); }

inline bool tex_finite(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

// Every check of rpt_set_mesh_textures but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `image` is `current`
// (empty: no mesh textured) with the named meshes' new textures (`first` unset), one entry per mesh.  Reads the items' uvs, never
// their texels.
inline int check_mesh_textures(const RefitPlan& plan, bool mesh_scene, const rpt_mesh_texture* items, uint32_t n_items,
                               const std::vector<TexImage>& current, std::vector<TexImage>& image, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return tex_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!plan.ok) return tex_error(err, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    if (!items && n_items) return tex_error(err, INVALID, "items is NULL");
    std::vector<TexImage> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_texture& it = items[i];
        if (it.mesh >= plan.n_meshes()) return tex_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return tex_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        if (it.width == 0u && it.height == 0u && !it.texels) { next[it.mesh] = TexImage(); continue; }       // remove
        const uint32_t count = plan.mesh_first[it.mesh + 1u] - plan.mesh_first[it.mesh];
        if (it.n_vertices != count) return tex_error(err, INVALID, "item %u: mesh %u: n_vertices %u != the uploaded mesh's %u", i, it.mesh, it.n_vertices, count);
        if (!it.uvs && count) return tex_error(err, INVALID, "item %u: mesh %u: uvs is NULL", i, it.mesh);
        if (it.width == 0u || it.height == 0u || it.width > kTexMaxSide || it.height > kTexMaxSide)
            return tex_error(err, INVALID, "item %u: mesh %u: a texture of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (!it.texels) return tex_error(err, INVALID, "item %u: mesh %u: texels is NULL", i, it.mesh);
        if (it.wrap != RPT_TEX_WRAP_REPEAT && it.wrap != RPT_TEX_WRAP_CLAMP)
            return tex_error(err, INVALID, "item %u: wrap %u of mesh %u is neither RPT_TEX_WRAP_REPEAT nor RPT_TEX_WRAP_CLAMP", i, it.wrap, it.mesh);
        if (it.filter != RPT_TEX_FILTER_NEAREST && it.filter != RPT_TEX_FILTER_BILINEAR)
            return tex_error(err, INVALID, "item %u: filter %u of mesh %u is neither RPT_TEX_FILTER_NEAREST nor RPT_TEX_FILTER_BILINEAR", i, it.filter, it.mesh);
        if (!tex_finite(it.gamma) || !(it.gamma > 0.0f) || it.gamma > 16.0f)
            return tex_error(err, INVALID, "item %u: mesh %u: gamma %g (it must be finite, above 0 and at most 16)", i, it.mesh, (double)it.gamma);
        for (uint32_t v = 0; v < count; ++v)
            for (uint32_t c = 0; c < 2u; ++c) {
                const float x = it.uvs[2 * (size_t)v + c];
                if (!tex_finite(x) || x > kTexMaxUv || x < -kTexMaxUv)
                    return tex_error(err, INVALID, "item %u: mesh %u: vertex %u has a UV that is not finite or beyond 2^20 in magnitude", i, it.mesh, v);
            }
        TexImage im;
        im.width = it.width; im.height = it.height; im.wrap = it.wrap; im.filter = it.filter; im.gamma = it.gamma;
        next[it.mesh] = im;
    }
    uint64_t total = 0;
    for (const TexImage& im : next) total += (uint64_t)im.width * im.height;
    if (total > kTexMaxTexels)
        return tex_error(err, RPT_ERR_UNSUPPORTED, "the scene's textures would hold %llu texels: more than 2^26 in all", (unsigned long long)total);
    image = std::move(next);
    return RPT_OK;
}

// The UV table after a call: `uvs` (2 per concatenated vertex) with the set items' copied in and the removed meshes' zeroed.
inline void tex_merge_uvs(const RefitPlan& plan, const rpt_mesh_texture* items, uint32_t n_items, std::vector<float>& uvs)
{
    uvs.resize(2 * (size_t)plan.n_vertices(), 0.0f);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_texture& it = items[i];
        const uint32_t first = plan.mesh_first[it.mesh], count = plan.mesh_first[it.mesh + 1u] - first;
        if (!count) continue;
        if (it.width == 0u) memset(&uvs[2 * (size_t)first], 0, 8 * (size_t)count);
        else memcpy(&uvs[2 * (size_t)first], it.uvs, 8 * (size_t)count);
    }
}

}  // namespace rpthost
