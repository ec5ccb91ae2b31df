// host_mmap.h — the host half of mesh material maps (include/rpt.h, "mesh material maps"): the statement of the decode and of the
// apply as plain functions, the plan rpt_set_mesh_material_maps makes (which meshes are ON, where each one's decoded texels lie, what
// every device gets), its checks, and the plain-loop reference of the decode.  Plain C++ with no HIP type in it, like host_nrm.h:
// capi.hip includes it, k_mmap.hip compiles the RPT_MMAP_FN functions for the device (dev_mesh_mmap.h calls them at the hit), and
// tests/mmap_harness.cpp runs this file on the host (tests/test_mesh_material_map_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off.  `/` is the correctly rounded divide on the host
// and on the device (as in host_nrm.h).  The interpolation, the wrap and the filter are host_tex.h's tex_interp, tex_wrap and
// tex_lookup: reused, not restated.
//
// Numbering.  As host_nrm.h: the descriptors are indexed by the TEXTURE ordinal of host_tex.h (a mapped mesh is textured), so the
// hit finds them through tri_tex; the table has one entry per mesh of the scene, so a texture call that changes the ordinals
// rewrites entries and moves no texel.  Nothing here knows a slot: a move or a rebuild leaves every table bit for bit.
//
// The layout, the plan, the descriptor table and the order of the checks are host_map.h's (MapLayout, MapPlan, map_desc_table,
// check_mesh_maps), shared with the normal and the emission maps; here are the names, the map's own fields and its own checks.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_map.h"
#include "host_refit.h"
#include "host_tex.h"

#ifndef RPT_MMAP_FN
#define RPT_MMAP_FN inline
#endif

namespace rpthost {

constexpr uint32_t kMmapDescWords = kMapDescWords;  // MmapDesc below, as words
constexpr uint64_t kMmapMaxTexels = kMapMaxTexels;  // of all maps of a scene
static_assert(RPT_MESH_MATERIAL_MAP_OFF == kMapOff && RPT_MESH_MATERIAL_MAP_ON == kMapOn, "host_map.h");

// One textured mesh, 16 B: one gather per hit on a textured mesh.  flags == 0: the mesh has no map (the rest is not read).
struct alignas(16) MmapDesc {
    uint32_t first;                   // its first texel in the map table
    uint32_t width, height;           // of the map
    uint32_t flags;                   // bit 0: ON; bit 1: the texture's wrap is RPT_TEX_WRAP_CLAMP; bit 2: the map's filter is BILINEAR
};

// c(k) of include/rpt.h, "decode": c(0) = 0, c(255) = 1, both exactly.
RPT_MMAP_FN float mmap_decode_value(uint32_t k) { return (float)k / 255.0f; }

// One channel's factor from the RGBA8 word (R in the low byte): c(its byte), or exactly 1 for RPT_MATERIAL_MAP_CHANNEL_NONE.
RPT_MMAP_FN float mmap_decode_channel(uint32_t rgba, uint32_t channel)
{
    return channel == RPT_MATERIAL_MAP_CHANNEL_NONE ? 1.0f : mmap_decode_value((rgba >> (8u * (channel & 3u))) & 255u);
}

// One decoded texel: {fr, fm, 0, 0}.  The channel choice is resolved here: the render kernels never see it.
RPT_MMAP_FN TexTexel mmap_decode_texel(uint32_t rgba, uint32_t roughness_channel, uint32_t metallic_channel)
{
    return TexTexel{mmap_decode_channel(rgba, roughness_channel), mmap_decode_channel(rgba, metallic_channel), 0.0f, 0.0f};
}

// The whole of "lookup at the hit": u and v are the triangle test's own, `texels` the map's first decoded texel; f[0] = fr, f[1] = fm.
// BILINEAR over texels in [0, 1] stays in [0, 1] (include/rpt.h says why), so there is no clamp.
RPT_MMAP_FN void mmap_factors(float u, float v, float sa, float ta, float sb, float tb, float sc, float tc, const TexTexel* texels, uint32_t width,
                              uint32_t height, uint32_t wrap, uint32_t filter, float f[2])
{
    const float w = (1.0f - u) - v;
    const float s = tex_interp(w, u, v, sa, sb, sc);
    const float t = tex_interp(w, u, v, ta, tb, tc);
    float rm[3];
    tex_lookup(texels, width, height, wrap, filter, s, t, rm);
    f[0] = rm[0]; f[1] = rm[1];
}

// "Apply": one multiplication each.
RPT_MMAP_FN void mmap_apply(float& roughness, float& metallic, const float f[2])
{
    roughness = roughness * f[0];
    metallic = metallic * f[1];
}

// The plain-loop reference of the decode kernel: `texels` (RGBA8, width*height*4 bytes) -> `out` (width*height texels).
inline void mmap_decode_reference(const uint8_t* texels, size_t n_texels, uint32_t roughness_channel, uint32_t metallic_channel, TexTexel* out)
{
    for (size_t i = 0; i < n_texels; ++i) {
        const uint32_t w = (uint32_t)texels[4 * i] | ((uint32_t)texels[4 * i + 1] << 8) | ((uint32_t)texels[4 * i + 2] << 16) | ((uint32_t)texels[4 * i + 3] << 24);
        out[i] = mmap_decode_texel(w, roughness_channel, metallic_channel);
    }
}

// One mesh's map as the context remembers it (width == 0: OFF).
struct MmapMap {
    uint32_t width = 0, height = 0, filter = 0;
    uint32_t roughness_channel = RPT_MATERIAL_MAP_CHANNEL_NONE, metallic_channel = RPT_MATERIAL_MAP_CHANNEL_NONE;
    uint64_t first = 0;               // its first texel in the devices' map table
};

// The device's map tables (DevState::mmap): host_map.h's, whose all-0xFFFFFFFF tri_light the form over the textured mesh-light tables
// reads while no mesh is ON (that base has no part of its own to lend one).
using MmapLayout = MapLayout;

// What rpt_set_mesh_material_maps leaves on the host for the life of the maps.
using MmapPlan = MapPlan<MmapMap>;

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_mmap_plan(const RefitPlan& plan, std::vector<MmapMap> map, MmapPlan& mp) { build_map_plan(plan.n_meshes(), plan.n_slots, std::move(map), mp); }

// The descriptor table of `mp` under the textures of `tp`: kMmapDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> mmap_desc_table(const MmapPlan& mp, const TexPlan& tp) { return map_desc_table(mp, tp); }

constexpr MapNames kMmapNames = {"rpt_set_mesh_material_maps", "RPT_MESH_MATERIAL_MAP", "a material map", "material maps"};

inline bool mmap_channel_ok(uint32_t c) { return c <= 3u || c == RPT_MATERIAL_MAP_CHANNEL_NONE; }

// Every check of rpt_set_mesh_material_maps but the NULL context (include/rpt.h), in check_mesh_maps' order with the channels in the
// feature's place.  RPT_OK: `map` is `current` (empty: every mesh OFF) with the named meshes' new maps (`first` unset), one entry per
// mesh.  Never reads the items' texels.
inline int check_mesh_material_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_material_map* items, uint32_t n_items,
                                    const std::vector<MmapMap>& current, std::vector<MmapMap>& map, std::string& err)
{
    const auto own = [](uint32_t i, const rpt_mesh_material_map& it, bool on, MmapMap& c, std::string& err) {
        const int INVALID = RPT_ERR_INVALID_ARG;
        const char* call = kMmapNames.call;
        if (!mmap_channel_ok(it.roughness_channel) || !mmap_channel_ok(it.metallic_channel))
            return call_error(err, call, INVALID, "item %u: mesh %u: channels %u and %u (each must be 0 .. 3 or RPT_MATERIAL_MAP_CHANNEL_NONE)", i, it.mesh,
                              it.roughness_channel, it.metallic_channel);
        if (on && it.roughness_channel == RPT_MATERIAL_MAP_CHANNEL_NONE && it.metallic_channel == RPT_MATERIAL_MAP_CHANNEL_NONE)
            return call_error(err, call, INVALID, "item %u: mesh %u: both channels are RPT_MATERIAL_MAP_CHANNEL_NONE: the map would change nothing", i, it.mesh);
        c.roughness_channel = it.roughness_channel; c.metallic_channel = it.metallic_channel;
        return (int)RPT_OK;
    };
    return check_mesh_maps(kMmapNames, plan, mesh_scene, tex, items, n_items, current, map, err, own);
}

}  // namespace rpthost
