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

#ifndef RPT_MMAP_FN
#define RPT_MMAP_FN inline
#endif

namespace rpthost {

constexpr uint32_t kMmapDescWords = 4;           // MmapDesc below, as words
constexpr uint64_t kMmapMaxTexels = 1ull << 26;  // of all maps of a scene

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

// The device's map tables (DevState::mmap), one allocation: per mesh of the SCENE 16 B (the descriptors, by texture ordinal); per
// triangle of the scene 4 B (the all-0xFFFFFFFF tri_light the form over the textured mesh-light tables reads while no mesh is ON:
// that base has no part of its own to lend one); per map texel 16 B.
struct MmapLayout {
    size_t off_desc = 0, off_none = 0, off_texels = 0, total = 0;
    MmapLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_texels)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_none = round16(4 * (size_t)kMmapDescWords * n_meshes);
        off_texels = off_none + round16(4 * (size_t)n_tris);
        total = off_texels + 16 * (size_t)n_texels;
    }
};

// What rpt_set_mesh_material_maps leaves on the host for the life of the maps.
struct MmapPlan {
    std::vector<MmapMap> map;         // mesh -> its map; empty: every mesh OFF
    uint32_t n_meshes = 0, n_tris = 0;
    uint64_t n_texels = 0;            // of all maps

    bool on(uint32_t mesh) const { return mesh < map.size() && map[mesh].width != 0u; }
    bool any() const
    {
        for (const MmapMap& m : map) if (m.width != 0u) return true;
        return false;
    }
    MmapLayout layout() const { return MmapLayout(n_meshes, n_tris, n_texels); }   // of every device's tables
};

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_mmap_plan(const RefitPlan& plan, std::vector<MmapMap> map, MmapPlan& mp)
{
    mp = MmapPlan();
    mp.map = std::move(map);
    mp.n_meshes = plan.n_meshes();
    mp.n_tris = plan.n_slots;
    mp.map.resize(mp.n_meshes);
    for (MmapMap& m : mp.map) {
        if (m.width == 0u) continue;
        m.first = mp.n_texels;
        mp.n_texels += (uint64_t)m.width * m.height;
    }
}

// The descriptor table of `mp` under the textures of `tp`: kMmapDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> mmap_desc_table(const MmapPlan& mp, const TexPlan& tp)
{
    std::vector<uint32_t> d((size_t)kMmapDescWords * mp.n_meshes, 0u);
    for (uint32_t j = 0; j < tp.n_tex() && j < mp.n_meshes; ++j) {
        const uint32_t m = tp.tex_mesh[j];
        if (!mp.on(m)) continue;
        const MmapMap& c = mp.map[m];
        d[4u * j] = (uint32_t)c.first;
        d[4u * j + 1u] = c.width;
        d[4u * j + 2u] = c.height;
        d[4u * j + 3u] = 1u | (tp.image[m].wrap == RPT_TEX_WRAP_CLAMP ? 2u : 0u) | (c.filter == RPT_TEX_FILTER_BILINEAR ? 4u : 0u);
    }
    return d;
}

// `err` = "rpt_set_mesh_material_maps: " + the message; returns `code`.
inline int mmap_error(std::string& err, int code, const char* fmt, ...)
{
    char buf[512];
    const int head = snprintf(buf, sizeof(buf), "rpt_set_mesh_material_maps: ");
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + head, sizeof(buf) - (size_t)head, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

inline bool mmap_channel_ok(uint32_t c) { return c <= 3u || c == RPT_MATERIAL_MAP_CHANNEL_NONE; }

// Every check of rpt_set_mesh_material_maps but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `map` is `current`
// (empty: every mesh OFF) with the named meshes' new maps (`first` unset), one entry per mesh.  Never reads the items' texels.
inline int check_mesh_material_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_material_map* items, uint32_t n_items,
                                    const std::vector<MmapMap>& current, std::vector<MmapMap>& map, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return mmap_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!items && n_items) return mmap_error(err, INVALID, "items is NULL");
    std::vector<MmapMap> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_material_map& it = items[i];
        if (it.mesh >= plan.n_meshes()) return mmap_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return mmap_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        const bool on = it.mode == RPT_MESH_MATERIAL_MAP_ON;
        if (!on && it.mode != RPT_MESH_MATERIAL_MAP_OFF)
            return mmap_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_MATERIAL_MAP_OFF nor RPT_MESH_MATERIAL_MAP_ON", i, it.mode, it.mesh);
        if (on && (it.width == 0u || it.height == 0u || it.width > kTexMaxSide || it.height > kTexMaxSide))
            return mmap_error(err, INVALID, "item %u: mesh %u: a map of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (on && !it.texels) return mmap_error(err, INVALID, "item %u: mesh %u: texels is NULL", i, it.mesh);
        if (it.filter != RPT_TEX_FILTER_NEAREST && it.filter != RPT_TEX_FILTER_BILINEAR)
            return mmap_error(err, INVALID, "item %u: filter %u of mesh %u is neither RPT_TEX_FILTER_NEAREST nor RPT_TEX_FILTER_BILINEAR", i, it.filter, it.mesh);
        if (!mmap_channel_ok(it.roughness_channel) || !mmap_channel_ok(it.metallic_channel))
            return mmap_error(err, INVALID, "item %u: mesh %u: channels %u and %u (each must be 0 .. 3 or RPT_MATERIAL_MAP_CHANNEL_NONE)", i, it.mesh,
                              it.roughness_channel, it.metallic_channel);
        if (on && it.roughness_channel == RPT_MATERIAL_MAP_CHANNEL_NONE && it.metallic_channel == RPT_MATERIAL_MAP_CHANNEL_NONE)
            return mmap_error(err, INVALID, "item %u: mesh %u: both channels are RPT_MATERIAL_MAP_CHANNEL_NONE: the map would change nothing", i, it.mesh);
        if (!on) {
            if (it.width != 0u || it.height != 0u || it.texels)
                return mmap_error(err, INVALID, "item %u: mesh %u: RPT_MESH_MATERIAL_MAP_OFF takes width == height == 0 and texels == NULL", i, it.mesh);
            next[it.mesh] = MmapMap();
            continue;
        }
        if (!tex.textured(it.mesh))
            return mmap_error(err, INVALID, "item %u: mesh %u is untextured: a material map takes its UVs and wrap from the mesh's texture (a 1 x 1 white texture is enough: rpt_set_mesh_textures)", i, it.mesh);
        MmapMap c;
        c.width = it.width; c.height = it.height; c.filter = it.filter;
        c.roughness_channel = it.roughness_channel; c.metallic_channel = it.metallic_channel;
        next[it.mesh] = c;
    }
    uint64_t total = 0;
    for (const MmapMap& c : next) total += (uint64_t)c.width * c.height;
    if (total > kMmapMaxTexels)
        return mmap_error(err, RPT_ERR_UNSUPPORTED, "the scene's material maps would hold %llu texels: more than 2^26 in all", (unsigned long long)total);
    map = std::move(next);
    return RPT_OK;
}

}  // namespace rpthost
