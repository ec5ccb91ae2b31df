// host_nrm.h — the host half of mesh normal maps (include/rpt.h, "mesh normal maps"): the statement of the decode and of the bend as
// plain functions, the plan rpt_set_mesh_normal_maps makes (which meshes are ON, where each one's decoded texels lie, what every
// device gets), its checks, and the plain-loop reference of the decode.  Plain C++ with no HIP type in it, like host_cut.h: capi.hip
// includes it, k_nrm.hip compiles the RPT_NRM_FN functions for the device (dev_mesh_nrm.h calls them at the hit), and
// tests/nrm_harness.cpp runs this file on the host (tests/test_mesh_normal_map_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off: each a*b + c*d below is two products and one add.
// `/` and __builtin_sqrtf are the correctly rounded divide and root on the host and on the device (as in host_env.h).  The
// interpolation, the wrap and the filter are host_tex.h's tex_interp, tex_wrap and tex_lookup: reused, not restated.
//
// Numbering.  The descriptors are indexed by the TEXTURE ordinal of host_tex.h (a normal-mapped mesh is textured), so the hit finds
// them through tri_tex; the table has one entry per mesh of the scene, so a texture call that changes the ordinals rewrites entries
// and moves no texel.  Nothing here knows a slot, and there is no per-vertex tangent: a move or a rebuild leaves every table bit for bit.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_refit.h"
#include "host_tex.h"

#ifndef RPT_NRM_FN
#define RPT_NRM_FN inline
#endif

namespace rpthost {

constexpr uint32_t kNrmDescWords = 4;           // NrmDesc below, as words
constexpr uint64_t kNrmMaxTexels = 1ull << 26;  // of all maps of a scene
constexpr float kNrmMaxStrength = 16.0f;

// One textured mesh, 16 B: one gather per hit on a textured mesh.  flags == 0: the mesh has no map (the rest is not read).
struct alignas(16) NrmDesc {
    uint32_t first;                   // its first texel in the map table
    uint32_t width, height;           // of the map
    uint32_t flags;                   // bit 0: ON; bit 1: the texture's wrap is RPT_TEX_WRAP_CLAMP; bit 2: the map's filter is BILINEAR
};

// c(k) of include/rpt.h, "decode": c(128) = 0, c(255) = 1, c(0) = c(1) = -1.
RPT_NRM_FN float nrm_decode_value(uint32_t k)
{
    const float c = ((float)k - 128.0f) / 127.0f;
    return c < -1.0f ? -1.0f : c;
}

// One decoded texel from its RGBA8 word (R in the low byte): {sx * c(R), sy * c(G), c(B), 0}.
RPT_NRM_FN TexTexel nrm_decode_texel(uint32_t rgba, float sx, float sy)
{
    return TexTexel{sx * nrm_decode_value(rgba & 255u), sy * nrm_decode_value((rgba >> 8) & 255u), nrm_decode_value((rgba >> 16) & 255u), 0.0f};
}

// sx and sy of a map: strength, and -strength for y with RPT_NORMAL_MAP_FLIP_GREEN.
RPT_NRM_FN float nrm_scale_y(float strength, uint32_t flags) { return (flags & RPT_NORMAL_MAP_FLIP_GREEN) ? -strength : strength; }

RPT_NRM_FN float nrm_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The bend of include/rpt.h: N the normal the hit would have had, e1 and e2 the triangle row's, (sa, ta), (sb, tb), (sc, tc) the
// corners' UVs, (x, y, z) the looked-up texel.  Every fall-back stores N's very words.
RPT_NRM_FN void nrm_bend(const float* N, const float* e1, const float* e2, float sa, float ta, float sb, float tb, float sc, float tc, float x, float y,
                         float z, float* out)
{
    out[0] = N[0]; out[1] = N[1]; out[2] = N[2];
    if (x == 0.0f && y == 0.0f) return;
    const float du1 = sb - sa, dv1 = tb - ta, du2 = sc - sa, dv2 = tc - ta;
    const float D = du1 * dv2 - du2 * dv1;
    if (!(D < 0.0f || D > 0.0f)) return;
    const float g = D > 0.0f ? 1.0f : -1.0f;
    float T0[3], B0[3], T1[3], T[3];
    for (int i = 0; i < 3; ++i) {
        T0[i] = g * (e1[i] * dv2 - e2[i] * dv1);
        B0[i] = g * (e2[i] * du1 - e1[i] * du2);
    }
    const float k = nrm_dot(N, T0);
    for (int i = 0; i < 3; ++i) T1[i] = T0[i] - N[i] * k;
    const float t2 = nrm_dot(T1, T1);
    if (!(t2 > 0.0f && t2 <= 3.40282347e+38f)) return;
    const float tl = __builtin_sqrtf(t2);
    for (int i = 0; i < 3; ++i) T[i] = T1[i] / tl;
    float B[3] = {N[1] * T[2] - N[2] * T[1], N[2] * T[0] - N[0] * T[2], N[0] * T[1] - N[1] * T[0]};
    if (nrm_dot(B, B0) < 0.0f) { B[0] = -B[0]; B[1] = -B[1]; B[2] = -B[2]; }
    const float m[3] = {(x * T[0] + y * B[0]) + z * N[0], (x * T[1] + y * B[1]) + z * N[1], (x * T[2] + y * B[2]) + z * N[2]};
    const float m2 = nrm_dot(m, m);
    if (!(m2 > 0.0f && m2 <= 3.40282347e+38f)) return;
    const float ml = __builtin_sqrtf(m2);
    out[0] = m[0] / ml; out[1] = m[1] / ml; out[2] = m[2] / ml;
}

// The whole of "lookup at the hit" and "bend": u and v are the triangle test's own, `texels` the map's first decoded texel.
RPT_NRM_FN void nrm_shade(const float* N, const float* e1, const float* e2, float u, float v, float sa, float ta, float sb, float tb, float sc, float tc,
                          const TexTexel* texels, uint32_t width, uint32_t height, uint32_t wrap, uint32_t filter, float* out)
{
    const float w = (1.0f - u) - v;
    const float s = tex_interp(w, u, v, sa, sb, sc);
    const float t = tex_interp(w, u, v, ta, tb, tc);
    float xyz[3];
    tex_lookup(texels, width, height, wrap, filter, s, t, xyz);
    nrm_bend(N, e1, e2, sa, ta, sb, tb, sc, tc, xyz[0], xyz[1], xyz[2], out);
}

// The plain-loop reference of the decode kernel: `texels` (RGBA8, width*height*4 bytes) -> `out` (width*height texels).
inline void nrm_decode_reference(const uint8_t* texels, size_t n_texels, float strength, uint32_t flags, TexTexel* out)
{
    const float sx = strength, sy = nrm_scale_y(strength, flags);
    for (size_t i = 0; i < n_texels; ++i) {
        const uint32_t w = (uint32_t)texels[4 * i] | ((uint32_t)texels[4 * i + 1] << 8) | ((uint32_t)texels[4 * i + 2] << 16);
        out[i] = nrm_decode_texel(w, sx, sy);
    }
}

// One mesh's map as the context remembers it (width == 0: OFF).
struct NrmMap {
    uint32_t width = 0, height = 0, filter = 0, flags = 0;
    float strength = 0.0f;
    uint64_t first = 0;               // its first texel in the devices' map table
};

// The device's map tables (DevState::nrm), one allocation: per mesh of the SCENE 16 B (the descriptors, by texture ordinal); per
// triangle of the scene 4 B (the all-0xFFFFFFFF tri_light the render kernel reads while no mesh is ON and no cutout or environment
// supplies one); per map texel 16 B.
struct NrmLayout {
    size_t off_desc = 0, off_none = 0, off_texels = 0, total = 0;
    NrmLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_texels)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_none = round16(4 * (size_t)kNrmDescWords * n_meshes);
        off_texels = off_none + round16(4 * (size_t)n_tris);
        total = off_texels + 16 * (size_t)n_texels;
    }
};

// What rpt_set_mesh_normal_maps leaves on the host for the life of the maps.
struct NrmPlan {
    std::vector<NrmMap> map;          // mesh -> its map; empty: every mesh OFF
    uint32_t n_meshes = 0, n_tris = 0;
    uint64_t n_texels = 0;            // of all maps

    bool on(uint32_t mesh) const { return mesh < map.size() && map[mesh].width != 0u; }
    bool any() const
    {
        for (const NrmMap& m : map) if (m.width != 0u) return true;
        return false;
    }
    NrmLayout layout() const { return NrmLayout(n_meshes, n_tris, n_texels); }     // of every device's tables
};

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_nrm_plan(const RefitPlan& plan, std::vector<NrmMap> map, NrmPlan& np)
{
    np = NrmPlan();
    np.map = std::move(map);
    np.n_meshes = plan.n_meshes();
    np.n_tris = plan.n_slots;
    np.map.resize(np.n_meshes);
    for (NrmMap& m : np.map) {
        if (m.width == 0u) continue;
        m.first = np.n_texels;
        np.n_texels += (uint64_t)m.width * m.height;
    }
}

// The descriptor table of `np` under the textures of `tp`: kNrmDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> nrm_desc_table(const NrmPlan& np, const TexPlan& tp)
{
    std::vector<uint32_t> d((size_t)kNrmDescWords * np.n_meshes, 0u);
    for (uint32_t j = 0; j < tp.n_tex() && j < np.n_meshes; ++j) {
        const uint32_t m = tp.tex_mesh[j];
        if (!np.on(m)) continue;
        const NrmMap& c = np.map[m];
        d[4u * j] = (uint32_t)c.first;
        d[4u * j + 1u] = c.width;
        d[4u * j + 2u] = c.height;
        d[4u * j + 3u] = 1u | (tp.image[m].wrap == RPT_TEX_WRAP_CLAMP ? 2u : 0u) | (c.filter == RPT_TEX_FILTER_BILINEAR ? 4u : 0u);
    }
    return d;
}

// `err` = "rpt_set_mesh_normal_maps: " + the message; returns `code`.
inline int nrm_error(std::string& err, int code, const char* fmt, ...)
{
    char buf[512];
    const int head = snprintf(buf, sizeof(buf), "rpt_set_mesh_normal_maps: ");
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + head, sizeof(buf) - (size_t)head, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// Every check of rpt_set_mesh_normal_maps but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `map` is `current`
// (empty: every mesh OFF) with the named meshes' new maps (`first` unset), one entry per mesh.  Never reads the items' texels.
inline int check_mesh_normal_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_normal_map* items, uint32_t n_items,
                                  const std::vector<NrmMap>& current, std::vector<NrmMap>& map, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return nrm_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!items && n_items) return nrm_error(err, INVALID, "items is NULL");
    std::vector<NrmMap> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_normal_map& it = items[i];
        if (it.mesh >= plan.n_meshes()) return nrm_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return nrm_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        const bool on = it.mode == RPT_MESH_NORMAL_MAP_ON;
        if (!on && it.mode != RPT_MESH_NORMAL_MAP_OFF)
            return nrm_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_NORMAL_MAP_OFF nor RPT_MESH_NORMAL_MAP_ON", i, it.mode, it.mesh);
        if (on && (it.width == 0u || it.height == 0u || it.width > kTexMaxSide || it.height > kTexMaxSide))
            return nrm_error(err, INVALID, "item %u: mesh %u: a map of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (on && !it.texels) return nrm_error(err, INVALID, "item %u: mesh %u: texels is NULL", i, it.mesh);
        if (it.filter != RPT_TEX_FILTER_NEAREST && it.filter != RPT_TEX_FILTER_BILINEAR)
            return nrm_error(err, INVALID, "item %u: filter %u of mesh %u is neither RPT_TEX_FILTER_NEAREST nor RPT_TEX_FILTER_BILINEAR", i, it.filter, it.mesh);
        if (it.flags & ~(uint32_t)RPT_NORMAL_MAP_FLIP_GREEN)
            return nrm_error(err, INVALID, "item %u: mesh %u: unknown flag bits 0x%x", i, it.mesh, it.flags & ~(uint32_t)RPT_NORMAL_MAP_FLIP_GREEN);
        if (!tex_finite(it.strength) || !(it.strength >= 0.0f) || it.strength > kNrmMaxStrength)
            return nrm_error(err, INVALID, "item %u: mesh %u: strength %g (it must be finite and lie in 0 .. 16)", i, it.mesh, (double)it.strength);
        if (!on) {
            if (it.width != 0u || it.height != 0u || it.texels)
                return nrm_error(err, INVALID, "item %u: mesh %u: RPT_MESH_NORMAL_MAP_OFF takes width == height == 0 and texels == NULL", i, it.mesh);
            next[it.mesh] = NrmMap();
            continue;
        }
        if (!tex.textured(it.mesh))
            return nrm_error(err, INVALID, "item %u: mesh %u is untextured: a normal map takes its UVs and wrap from the mesh's texture (a 1 x 1 white texture is enough: rpt_set_mesh_textures)", i, it.mesh);
        NrmMap c;
        c.width = it.width; c.height = it.height; c.filter = it.filter; c.flags = it.flags; c.strength = it.strength;
        next[it.mesh] = c;
    }
    uint64_t total = 0;
    for (const NrmMap& c : next) total += (uint64_t)c.width * c.height;
    if (total > kNrmMaxTexels)
        return nrm_error(err, RPT_ERR_UNSUPPORTED, "the scene's normal maps would hold %llu texels: more than 2^26 in all", (unsigned long long)total);
    map = std::move(next);
    return RPT_OK;
}

}  // namespace rpthost
