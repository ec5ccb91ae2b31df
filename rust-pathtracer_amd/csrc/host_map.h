// host_map.h — what the image-map features of a mesh scene share on the host: cutouts (host_cut.h), normal maps (host_nrm.h), material
// maps (host_mmap.h) and emission maps (host_emap.h).  Each keeps, per device, one allocation of descriptors, an empty tri_light and the
// meshes' decoded images one after the other, and each setter makes that allocation anew: the named meshes' images are staged and
// decoded, the others' are copied over on the device.  Here are the one error formatter every host_*.h uses, the layout, the plan and
// the descriptor words of such a table, the skeleton of the setters' checks, and the RECIPE: the offsets of one device's part of a
// call as plain numbers, which capi.hip's map_device walks with HIP calls and tests/map_harness.cpp with memset and memcpy
// (tests/test_mesh_map_host.py).  Plain C++ with no HIP type in it.
//
// host_refit.h and host_tex.h include this file for the formatter, so nothing here names their types: the scene's plan and the
// texture plan are template parameters where a function needs them.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"

namespace rpthost {

// `err` = `call` + ": " + the message (at most 511 characters, as capi.hip's set_err keeps); returns `code`.
inline int call_error(std::string& err, const char* call, int code, const char* fmt, ...)
{
    char buf[512];
    const int head = snprintf(buf, sizeof(buf), "%s: ", call);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + head, sizeof(buf) - (size_t)head, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

constexpr uint32_t kMapDescWords = 4;           // a descriptor, as words: first, width, height, flags
constexpr uint32_t kMapMaxSide = 16384;         // of an image
constexpr uint64_t kMapMaxTexels = 1ull << 26;  // of all images of one feature in a scene
constexpr uint32_t kMapOff = 0, kMapOn = 1;     // an item's mode, under every feature's own names (each header asserts it)

inline size_t map_round16(size_t b) { return (b + 15) & ~(size_t)15; }

// One byte pattern over a range of a fresh allocation.
struct MapFill {
    size_t off, bytes;
    int value;
};

// A device's map tables, one allocation: per mesh of the SCENE 16 B (the descriptors, by texture ordinal); per triangle of the scene
// 4 B (an all-0xFFFFFFFF tri_light for the render forms that have no other to read); per map texel 16 B.
struct MapLayout {
    size_t off_desc = 0, off_none = 0, off_texels = 0, total = 0;
    MapLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_texels)
    {
        off_none = map_round16(4 * (size_t)kMapDescWords * n_meshes);
        off_texels = off_none + map_round16(4 * (size_t)n_tris);
        total = off_texels + 16 * (size_t)n_texels;
    }
    size_t off_elems() const { return off_texels; }
    std::vector<MapFill> fills() const { return {{0, off_none, 0}, {off_none, off_texels - off_none, 0xFF}}; }
};

// One mesh's part of a table, in the table's elements (texels, or a mask's words); count == 0: the mesh is OFF.
struct MapSlot {
    uint64_t first = 0, count = 0;
};

// What a setter leaves on the host for the life of its maps.  Entry: width (0: OFF), height and first, and what the feature adds.
template <class Entry>
struct MapPlan {
    std::vector<Entry> map;           // mesh -> its map; empty: every mesh OFF
    uint32_t n_meshes = 0, n_tris = 0;
    uint64_t n_texels = 0;            // of all maps

    bool on(uint32_t mesh) const { return mesh < map.size() && map[mesh].width != 0u; }
    bool any() const
    {
        for (const Entry& m : map) if (m.width != 0u) return true;
        return false;
    }
    MapLayout layout() const { return MapLayout(n_meshes, n_tris, n_texels); }     // of every device's tables
    std::vector<MapSlot> slots() const
    {
        std::vector<MapSlot> s(map.size());
        for (size_t m = 0; m < map.size(); ++m) s[m] = MapSlot{map[m].first, (uint64_t)map[m].width * map[m].height};
        return s;
    }
};

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene of n_meshes meshes and n_tris triangles.
template <class Plan, class Entry>
inline void build_map_plan(uint32_t n_meshes, uint32_t n_tris, std::vector<Entry> map, Plan& p)
{
    p = Plan();
    p.map = std::move(map);
    p.n_meshes = n_meshes;
    p.n_tris = n_tris;
    p.map.resize(n_meshes);
    for (Entry& m : p.map) {
        if (m.width == 0u) continue;
        m.first = p.n_texels;
        p.n_texels += (uint64_t)m.width * m.height;
    }
}

// A descriptor's flags word.  bit 0: ON; bit 1: the texture's wrap is RPT_TEX_WRAP_CLAMP; bit 2: the map's filter is BILINEAR.
inline uint32_t map_desc_flags(uint32_t wrap, uint32_t filter)
{
    return 1u | (wrap == RPT_TEX_WRAP_CLAMP ? 2u : 0u) | (filter == RPT_TEX_FILTER_BILINEAR ? 4u : 0u);
}

// Descriptor j of table d: the ON entry c with `flags`.
template <class Entry>
inline void map_desc_put(std::vector<uint32_t>& d, uint32_t j, const Entry& c, uint32_t flags)
{
    d[4u * j] = (uint32_t)c.first;
    d[4u * j + 1u] = c.width;
    d[4u * j + 2u] = c.height;
    d[4u * j + 3u] = flags;
}

// The descriptor table of `p` under the textures of `tp` (host_tex.h, TexPlan): kMapDescWords per mesh of the scene, entry j the map
// of texture ordinal j.
template <class Plan, class Tex>
inline std::vector<uint32_t> map_desc_table(const Plan& p, const Tex& tp)
{
    std::vector<uint32_t> d((size_t)kMapDescWords * p.n_meshes, 0u);
    for (uint32_t j = 0; j < tp.n_tex() && j < p.n_meshes; ++j) {
        const uint32_t m = tp.tex_mesh[j];
        if (p.on(m)) map_desc_put(d, j, p.map[m], map_desc_flags(tp.image[m].wrap, p.map[m].filter));
    }
    return d;
}

// The words in which the three map setters' messages differ.
struct MapNames {
    const char* call;                 // "rpt_set_mesh_normal_maps"
    const char* mode;                 // "RPT_MESH_NORMAL_MAP": its modes are this + "_OFF" and + "_ON"
    const char* a_map;                // "a normal map"
    const char* maps;                 // "normal maps"
};

// Every check of a map setter but the NULL context (include/rpt.h), in one fixed order.
// own(i, item, on, entry, err) is the feature's own block: its checks, and on RPT_OK its fields of `entry`.  RPT_OK: `map` is
// `current` (empty: every mesh OFF) with the named meshes' new maps (`first` unset), one entry per mesh.  Never reads the items' texels.
template <class Refit, class Tex, class Item, class Entry, class Own>
inline int check_mesh_maps(const MapNames& nm, const Refit& plan, bool mesh_scene, const Tex& tex, const Item* items, uint32_t n_items,
                           const std::vector<Entry>& current, std::vector<Entry>& map, std::string& err, Own own)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return call_error(err, nm.call, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!items && n_items) return call_error(err, nm.call, INVALID, "items is NULL");
    std::vector<Entry> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const Item& it = items[i];
        if (it.mesh >= plan.n_meshes()) return call_error(err, nm.call, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return call_error(err, nm.call, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        const bool on = it.mode == kMapOn;
        if (!on && it.mode != kMapOff)
            return call_error(err, nm.call, INVALID, "item %u: mode %u of mesh %u is neither %s_OFF nor %s_ON", i, it.mode, it.mesh, nm.mode, nm.mode);
        if (on && (it.width == 0u || it.height == 0u || it.width > kMapMaxSide || it.height > kMapMaxSide))
            return call_error(err, nm.call, INVALID, "item %u: mesh %u: a map of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (on && !it.texels) return call_error(err, nm.call, INVALID, "item %u: mesh %u: texels is NULL", i, it.mesh);
        if (it.filter != RPT_TEX_FILTER_NEAREST && it.filter != RPT_TEX_FILTER_BILINEAR)
            return call_error(err, nm.call, INVALID, "item %u: filter %u of mesh %u is neither RPT_TEX_FILTER_NEAREST nor RPT_TEX_FILTER_BILINEAR", i, it.filter, it.mesh);
        Entry c;
        const int rc = own(i, it, on, c, err);
        if (rc != RPT_OK) return rc;
        if (!on) {
            if (it.width != 0u || it.height != 0u || it.texels)
                return call_error(err, nm.call, INVALID, "item %u: mesh %u: %s_OFF takes width == height == 0 and texels == NULL", i, it.mesh, nm.mode);
            next[it.mesh] = Entry();
            continue;
        }
        if (!tex.textured(it.mesh))
            return call_error(err, nm.call, INVALID, "item %u: mesh %u is untextured: %s takes its UVs and wrap from the mesh's texture (a 1 x 1 white texture is enough: rpt_set_mesh_textures)", i, it.mesh, nm.a_map);
        c.width = it.width; c.height = it.height; c.filter = it.filter;
        next[it.mesh] = c;
    }
    uint64_t total = 0;
    for (const Entry& c : next) total += (uint64_t)c.width * c.height;
    if (total > kMapMaxTexels)
        return call_error(err, nm.call, RPT_ERR_UNSUPPORTED, "the scene's %s would hold %llu texels: more than 2^26 in all", nm.maps, (unsigned long long)total);
    map = std::move(next);
    return RPT_OK;
}

// ---- the recipe of one device's part of a setter ------------------------------------------------------------------------------------
// One item of a call, whatever the feature: the mesh, ON or OFF, the image's sides and its bytes on the host.
struct MapNamed {
    uint32_t mesh;
    bool on;
    uint32_t width, height;
    const void* src;
};

template <class Item, class Src>
inline std::vector<MapNamed> map_named(const Item* items, uint32_t n_items, Src Item::*src)
{
    std::vector<MapNamed> named(n_items);
    for (uint32_t i = 0; i < n_items; ++i) named[i] = MapNamed{items[i].mesh, items[i].mode == kMapOn, items[i].width, items[i].height, items[i].*src};
    return named;
}

// A feature's constants: the bytes of a table element on the device (16: a texel; 4: a mask word), of a texel of the source image
// (4: RGBA8; 1: an alpha), and of what the decode wants in front of each staged image (1024: the L table of tex_decode; else 0).
struct MapConsts {
    uint32_t elem_bytes, src_bytes, prefix;
};

constexpr uint32_t kMapNoMesh = 0xFFFFFFFFu;

struct MapRecipe {
    struct Item {                     // a named ON item: staged, then decoded into the new table
        uint32_t index;               // in the call's items
        size_t stage;                 // its part of the stage allocation: the prefix, then (at stage + prefix) the image's bytes
        uint64_t dst, count;          // its first element in the new table; its texels
    };
    struct Keep {                     // a mesh that is ON and not named: copied from the old table to the new one on the device
        uint32_t mesh;
        uint64_t src, dst;            // its first element in the old table, in the new one
        size_t bytes;
    };
    size_t stage_bytes = 0;           // of the stage allocation: every part is a multiple of 16 B
    std::vector<Item> items;
    std::vector<Keep> keeps;
    uint32_t missing = kMapNoMesh;    // a mesh to keep that the device holds nothing for: an error, and no step
};

// now: the new plan's slots; old: those of the plan the device's tables were made by; held: the device has such tables.
inline MapRecipe map_recipe(const std::vector<MapSlot>& now, const std::vector<MapSlot>& old, bool held, const std::vector<MapNamed>& named, const MapConsts& k)
{
    MapRecipe r;
    std::vector<uint8_t> is_named(now.size(), 0);
    for (uint32_t i = 0; i < named.size(); ++i) {
        const MapNamed& it = named[i];
        is_named[it.mesh] = 1;
        if (!it.on) continue;
        const size_t n = (size_t)it.width * it.height;
        r.items.push_back(MapRecipe::Item{i, r.stage_bytes, now[it.mesh].first, n});
        r.stage_bytes += k.prefix + map_round16(k.src_bytes * n);
    }
    for (uint32_t m = 0; m < now.size(); ++m) {
        if (is_named[m] || !now[m].count) continue;
        if (!held || m >= old.size() || !old[m].count) {
            r = MapRecipe();
            r.missing = m;
            return r;
        }
        r.keeps.push_back(MapRecipe::Keep{m, old[m].first, now[m].first, k.elem_bytes * (size_t)now[m].count});
    }
    return r;
}

}  // namespace rpthost
