// host_emap.h — the host half of mesh emission maps (include/rpt.h, "mesh emission maps"): the statement of the lookup and of the
// apply as plain functions, the plan rpt_set_mesh_emission_maps makes (which meshes are ON, where each one's decoded texels lie, what
// every device gets), its checks, and the plain-loop reference of decode + lookup + apply.  Plain C++ with no HIP type in it, like
// host_mmap.h: capi.hip includes it, k_emap.hip compiles the RPT_EMAP_FN functions for the device (dev_mesh_emap.h calls them at the
// hit, at the emitter exit and in the mesh-light sampler), and tests/emap_harness.cpp runs this file on the host
// (tests/test_mesh_emission_map_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off.  The decode, the interpolation, the wrap and the
// filter are host_tex.h's tex_decode_value, tex_interp, tex_wrap and tex_lookup: reused, not restated.
//
// Numbering.  Two descriptor tables, one entry per mesh of the scene each, so that a texture call or a light call that changes
// ordinals rewrites entries and moves no texel: the HIT table is indexed by the TEXTURE ordinal of host_tex.h (the hit finds it
// through tri_tex, as host_mmap.h's), the SAMPLER table by the LIGHT ordinal of host_light.h (the sampler is handed that ordinal).
// Nothing here knows a slot: a move or a rebuild leaves every table bit for bit.
//
// The zero block.  The emission-mapped render forms sit over the material-mapped ones (launch_emap.h).  A scene with an emission map
// and no material map takes them through a table of all-zero MmapDesc (flags == 0: "no map on this mesh") and the all-0xFFFFFFFF
// tri_light of MmapLayout::off_none, both carried here: the block at off_zero is laid out as MmapLayout(n_meshes, n_tris, 0), and
// EmapPlan::zero is the MmapPlan that describes it, so mesh_args_mmap.h binds it as it binds a real one.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_light.h"
#include "host_mmap.h"
#include "host_refit.h"
#include "host_tex.h"

#ifndef RPT_EMAP_FN
#define RPT_EMAP_FN inline
#endif

namespace rpthost {

constexpr uint32_t kEmapDescWords = 4;           // EmapDesc below, as words
constexpr uint64_t kEmapMaxTexels = 1ull << 26;  // of all maps of a scene

// One mesh, 16 B: one gather per hit on a textured mesh, one per sample of an ON mesh.  flags == 0: the mesh has no map (the rest
// is not read).
struct alignas(16) EmapDesc {
    uint32_t first;                   // its first texel in the map table
    uint32_t width, height;           // of the map
    uint32_t flags;                   // bit 0: ON; bit 1: the texture's wrap is RPT_TEX_WRAP_CLAMP; bit 2: the map's filter is BILINEAR
};

// The whole of "lookup": u and v are the triangle test's own (hit side) or the sampled point's bu and bv (sampler side), a, b, c the
// triangle's corners in its own order, `texels` the map's first decoded texel; E = the looked-up {r, g, b}.
RPT_EMAP_FN void emap_lookup(float u, float v, float sa, float ta, float sb, float tb, float sc, float tc, const TexTexel* texels, uint32_t width,
                             uint32_t height, uint32_t wrap, uint32_t filter, float E[3])
{
    const float w = (1.0f - u) - v;
    const float s = tex_interp(w, u, v, sa, sb, sc);
    const float t = tex_interp(w, u, v, ta, tb, tc);
    tex_lookup(texels, width, height, wrap, filter, s, t, E);
}

// The lookup through a descriptor (flags != 0).
RPT_EMAP_FN void emap_lookup_desc(const EmapDesc& d, const TexTexel* map_texels, float u, float v, const float* uva, const float* uvb, const float* uvc, float E[3])
{
    emap_lookup(u, v, uva[0], uva[1], uvb[0], uvb[1], uvc[0], uvc[1], map_texels + d.first, d.width, d.height,
                (d.flags & 2u) ? (uint32_t)RPT_TEX_WRAP_CLAMP : (uint32_t)RPT_TEX_WRAP_REPEAT,
                (d.flags & 4u) ? (uint32_t)RPT_TEX_FILTER_BILINEAR : (uint32_t)RPT_TEX_FILTER_NEAREST, E);
}

// "Apply": e.c = e.c * E.c, one multiplication each.
RPT_EMAP_FN void emap_apply(float e[3], const float E[3])
{
    e[0] = e[0] * E[0];
    e[1] = e[1] * E[1];
    e[2] = e[2] * E[2];
}

// The sampler's emission line: e.c = m.emission[c] * E.c, then emission.c = N_f * e.c — the products in this order.
RPT_EMAP_FN void emap_sample_emission(const float m_emission[3], const float E[3], float n_f, float out[3])
{
    float e[3] = {m_emission[0], m_emission[1], m_emission[2]};
    emap_apply(e, E);
    out[0] = n_f * e[0];
    out[1] = n_f * e[1];
    out[2] = n_f * e[2];
}

// The sampled point's barycentrics from the draws r1 and r2: the sampler's own three operations ("mesh lights"), with the correctly
// rounded root, so the bits are the sampler's.
RPT_EMAP_FN void emap_sample_uv(float r1, float r2, float& bu, float& bv)
{
    const float su = __builtin_sqrtf(r1);
    bu = 1.0f - su;
    bv = r2 * su;
}

// The plain-loop reference of decode + lookup + apply: the map's bytes (RGBA8, width * height * 4) decoded with `gamma` as "mesh
// textures" decodes, looked up at (u, v) over the corner UVs, applied to e.
inline void emap_reference(const uint8_t* bytes, uint32_t width, uint32_t height, float gamma, uint32_t wrap, uint32_t filter, float u, float v,
                           const float uva[2], const float uvb[2], const float uvc[2], float e[3])
{
    std::vector<TexTexel> texels((size_t)width * height);
    tex_decode_reference(bytes, texels.size(), gamma, texels.data());
    float E[3];
    emap_lookup(u, v, uva[0], uva[1], uvb[0], uvb[1], uvc[0], uvc[1], texels.data(), width, height, wrap, filter, E);
    emap_apply(e, E);
}

// One mesh's map as the context remembers it (width == 0: OFF).
struct EmapMap {
    uint32_t width = 0, height = 0, filter = 0;
    float gamma = 1.0f;
    uint64_t first = 0;               // its first texel in the devices' map table
};

// The device's map tables (DevState::emap), one allocation: per mesh of the SCENE 16 B twice (the hit table by texture ordinal, the
// sampler table by light ordinal); the zero block (the top of this file: per mesh 16 B, per triangle of the scene 4 B); per map texel
// 16 B.
struct EmapLayout {
    size_t off_desc = 0, off_light_desc = 0, off_zero = 0, off_texels = 0, total = 0;
    MmapLayout zero;
    EmapLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_texels) : zero(n_meshes, n_tris, 0)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_light_desc = round16(4 * (size_t)kEmapDescWords * n_meshes);
        off_zero = 2 * off_light_desc;
        off_texels = off_zero + round16(zero.total);
        total = off_texels + 16 * (size_t)n_texels;
    }
};

// What rpt_set_mesh_emission_maps leaves on the host for the life of the maps.
struct EmapPlan {
    std::vector<EmapMap> map;         // mesh -> its map; empty: every mesh OFF
    uint32_t n_meshes = 0, n_tris = 0;
    uint64_t n_texels = 0;            // of all maps
    MmapPlan zero;                    // the plan of the zero block: no map ON, the scene's sizes

    bool on(uint32_t mesh) const { return mesh < map.size() && map[mesh].width != 0u; }
    bool any() const
    {
        for (const EmapMap& m : map) if (m.width != 0u) return true;
        return false;
    }
    EmapLayout layout() const { return EmapLayout(n_meshes, n_tris, n_texels); }   // of every device's tables
};

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_emap_plan(const RefitPlan& plan, std::vector<EmapMap> map, EmapPlan& ep)
{
    ep = EmapPlan();
    ep.map = std::move(map);
    ep.n_meshes = plan.n_meshes();
    ep.n_tris = plan.n_slots;
    ep.map.resize(ep.n_meshes);
    for (EmapMap& m : ep.map) {
        if (m.width == 0u) continue;
        m.first = ep.n_texels;
        ep.n_texels += (uint64_t)m.width * m.height;
    }
    ep.zero.n_meshes = ep.n_meshes;
    ep.zero.n_tris = ep.n_tris;
}

inline void emap_desc_put(std::vector<uint32_t>& d, uint32_t j, const EmapMap& c, uint32_t wrap)
{
    d[4u * j] = (uint32_t)c.first;
    d[4u * j + 1u] = c.width;
    d[4u * j + 2u] = c.height;
    d[4u * j + 3u] = 1u | (wrap == RPT_TEX_WRAP_CLAMP ? 2u : 0u) | (c.filter == RPT_TEX_FILTER_BILINEAR ? 4u : 0u);
}

// The hit table of `ep` under the textures of `tp`: kEmapDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> emap_desc_table(const EmapPlan& ep, const TexPlan& tp)
{
    std::vector<uint32_t> d((size_t)kEmapDescWords * ep.n_meshes, 0u);
    for (uint32_t j = 0; j < tp.n_tex() && j < ep.n_meshes; ++j) {
        const uint32_t m = tp.tex_mesh[j];
        if (ep.on(m)) emap_desc_put(d, j, ep.map[m], tp.image[m].wrap);
    }
    return d;
}

// The sampler table of `ep` under the textures of `tp` and the lights of `lp`: entry j the map of light ordinal j.
inline std::vector<uint32_t> emap_light_desc_table(const EmapPlan& ep, const TexPlan& tp, const LightPlan& lp)
{
    std::vector<uint32_t> d((size_t)kEmapDescWords * ep.n_meshes, 0u);
    for (uint32_t j = 0; j < lp.n_on() && j < ep.n_meshes; ++j) {
        const uint32_t m = lp.on_mesh[j];
        if (ep.on(m) && tp.textured(m)) emap_desc_put(d, j, ep.map[m], tp.image[m].wrap);
    }
    return d;
}

// `err` = "rpt_set_mesh_emission_maps: " + the message; returns `code`.
inline int emap_error(std::string& err, int code, const char* fmt, ...)
{
    char buf[512];
    const int head = snprintf(buf, sizeof(buf), "rpt_set_mesh_emission_maps: ");
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + head, sizeof(buf) - (size_t)head, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// Every check of rpt_set_mesh_emission_maps but the NULL context (include/rpt.h), in one fixed order: rpt_set_mesh_material_maps'
// list with the gamma rule of rpt_set_mesh_textures in the place of the channels'.  RPT_OK: `map` is `current` (empty: every mesh
// OFF) with the named meshes' new maps (`first` unset), one entry per mesh.  Never reads the items' texels.
inline int check_mesh_emission_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_emission_map* items, uint32_t n_items,
                                    const std::vector<EmapMap>& current, std::vector<EmapMap>& map, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return emap_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!items && n_items) return emap_error(err, INVALID, "items is NULL");
    std::vector<EmapMap> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_emission_map& it = items[i];
        if (it.mesh >= plan.n_meshes()) return emap_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return emap_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        const bool on = it.mode == RPT_MESH_EMISSION_MAP_ON;
        if (!on && it.mode != RPT_MESH_EMISSION_MAP_OFF)
            return emap_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_EMISSION_MAP_OFF nor RPT_MESH_EMISSION_MAP_ON", i, it.mode, it.mesh);
        if (on && (it.width == 0u || it.height == 0u || it.width > kTexMaxSide || it.height > kTexMaxSide))
            return emap_error(err, INVALID, "item %u: mesh %u: a map of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (on && !it.texels) return emap_error(err, INVALID, "item %u: mesh %u: texels is NULL", i, it.mesh);
        if (it.filter != RPT_TEX_FILTER_NEAREST && it.filter != RPT_TEX_FILTER_BILINEAR)
            return emap_error(err, INVALID, "item %u: filter %u of mesh %u is neither RPT_TEX_FILTER_NEAREST nor RPT_TEX_FILTER_BILINEAR", i, it.filter, it.mesh);
        if (on && (!tex_finite(it.gamma) || !(it.gamma > 0.0f) || it.gamma > 16.0f))
            return emap_error(err, INVALID, "item %u: mesh %u: gamma %g (it must be finite, above 0 and at most 16)", i, it.mesh, (double)it.gamma);
        if (!on) {
            if (it.width != 0u || it.height != 0u || it.texels)
                return emap_error(err, INVALID, "item %u: mesh %u: RPT_MESH_EMISSION_MAP_OFF takes width == height == 0 and texels == NULL", i, it.mesh);
            next[it.mesh] = EmapMap();
            continue;
        }
        if (!tex.textured(it.mesh))
            return emap_error(err, INVALID, "item %u: mesh %u is untextured: an emission map takes its UVs and wrap from the mesh's texture (a 1 x 1 white texture is enough: rpt_set_mesh_textures)", i, it.mesh);
        EmapMap c;
        c.width = it.width; c.height = it.height; c.filter = it.filter; c.gamma = it.gamma;
        next[it.mesh] = c;
    }
    uint64_t total = 0;
    for (const EmapMap& c : next) total += (uint64_t)c.width * c.height;
    if (total > kEmapMaxTexels)
        return emap_error(err, RPT_ERR_UNSUPPORTED, "the scene's emission maps would hold %llu texels: more than 2^26 in all", (unsigned long long)total);
    map = std::move(next);
    return RPT_OK;
}

}  // namespace rpthost
