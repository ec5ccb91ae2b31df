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
//
// The plan's members, the hit table, the descriptor words and the order of the checks are host_map.h's (MapPlan, map_desc_table,
// map_desc_put, check_mesh_maps), shared with the normal and the material maps; here are the names, the second table, the zero
// block, the map's own field and its own check.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_light.h"
#include "host_map.h"
#include "host_mmap.h"
#include "host_refit.h"
#include "host_tex.h"

#ifndef RPT_EMAP_FN
#define RPT_EMAP_FN inline
#endif

namespace rpthost {

constexpr uint32_t kEmapDescWords = kMapDescWords;  // EmapDesc below, as words
constexpr uint64_t kEmapMaxTexels = kMapMaxTexels;  // of all maps of a scene
static_assert(RPT_MESH_EMISSION_MAP_OFF == kMapOff && RPT_MESH_EMISSION_MAP_ON == kMapOn, "host_map.h");

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
    MapLayout zero;
    EmapLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_texels) : zero(n_meshes, n_tris, 0)
    {
        off_light_desc = map_round16(4 * (size_t)kEmapDescWords * n_meshes);
        off_zero = 2 * off_light_desc;
        off_texels = off_zero + map_round16(zero.total);
        total = off_texels + 16 * (size_t)n_texels;
    }
    size_t off_elems() const { return off_texels; }
    // both descriptor tables and the zero block's descriptors; the zero block's empty light table
    std::vector<MapFill> fills() const { return {{0, off_texels, 0}, {off_zero + zero.off_none, zero.off_texels - zero.off_none, 0xFF}}; }
};

// What rpt_set_mesh_emission_maps leaves on the host for the life of the maps.
struct EmapPlan : MapPlan<EmapMap> {
    MmapPlan zero;                    // the plan of the zero block: no map ON, the scene's sizes
    EmapLayout layout() const { return EmapLayout(n_meshes, n_tris, n_texels); }   // of every device's tables
};

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_emap_plan(const RefitPlan& plan, std::vector<EmapMap> map, EmapPlan& ep)
{
    build_map_plan(plan.n_meshes(), plan.n_slots, std::move(map), ep);
    ep.zero.n_meshes = ep.n_meshes;
    ep.zero.n_tris = ep.n_tris;
}

// The hit table of `ep` under the textures of `tp`: kEmapDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> emap_desc_table(const EmapPlan& ep, const TexPlan& tp) { return map_desc_table(ep, tp); }

// The sampler table of `ep` under the textures of `tp` and the lights of `lp`: entry j the map of light ordinal j.
inline std::vector<uint32_t> emap_light_desc_table(const EmapPlan& ep, const TexPlan& tp, const LightPlan& lp)
{
    std::vector<uint32_t> d((size_t)kEmapDescWords * ep.n_meshes, 0u);
    for (uint32_t j = 0; j < lp.n_on() && j < ep.n_meshes; ++j) {
        const uint32_t m = lp.on_mesh[j];
        if (ep.on(m) && tp.textured(m)) map_desc_put(d, j, ep.map[m], map_desc_flags(tp.image[m].wrap, ep.map[m].filter));
    }
    return d;
}

constexpr MapNames kEmapNames = {"rpt_set_mesh_emission_maps", "RPT_MESH_EMISSION_MAP", "an emission map", "emission maps"};

// Every check of rpt_set_mesh_emission_maps but the NULL context (include/rpt.h), in check_mesh_maps' order with the gamma rule of
// rpt_set_mesh_textures in the feature's place.  RPT_OK: `map` is `current` (empty: every mesh OFF) with the named meshes' new maps
// (`first` unset), one entry per mesh.  Never reads the items' texels.
inline int check_mesh_emission_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_emission_map* items, uint32_t n_items,
                                    const std::vector<EmapMap>& current, std::vector<EmapMap>& map, std::string& err)
{
    const auto own = [](uint32_t i, const rpt_mesh_emission_map& it, bool on, EmapMap& c, std::string& err) {
        if (on && (!tex_finite(it.gamma) || !(it.gamma > 0.0f) || it.gamma > 16.0f))
            return call_error(err, kEmapNames.call, RPT_ERR_INVALID_ARG, "item %u: mesh %u: gamma %g (it must be finite, above 0 and at most 16)", i, it.mesh, (double)it.gamma);
        c.gamma = it.gamma;
        return (int)RPT_OK;
    };
    return check_mesh_maps(kEmapNames, plan, mesh_scene, tex, items, n_items, current, map, err, own);
}

}  // namespace rpthost
