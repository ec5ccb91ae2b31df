// host_cut.h — the host half of mesh cutouts (include/rpt.h, "mesh cutouts"): the statement of the mask bits and of the cut test as
// plain functions, the plan rpt_set_mesh_cutouts makes (which meshes are ON, where each one's mask lies, what every device gets), its
// checks, and the plain-loop reference of the mask.  Plain C++ with no HIP type in it, like host_tex.h: capi.hip includes it,
// k_cut.hip compiles the RPT_CUT_FN functions for the device (dev_mesh_cut.h calls them inside the walks), and tests/cut_harness.cpp
// runs this file under the address and undefined-behaviour sanitizers (tests/test_mesh_cutout_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off.  The interpolation, the wrap and the NEAREST index
// are host_tex.h's tex_interp, tex_wrap and tex_nearest_index: reused, not restated.
//
// Numbering.  The cutout descriptors are indexed by the TEXTURE ordinal of host_tex.h (a cutout mesh is textured), so the walk finds
// them through tri_tex and needs no per-triangle table of its own; the table has one entry per mesh of the scene, so a texture call
// that changes the ordinals rewrites entries and moves no mask.  Nothing here knows a slot: a rebuild leaves every table bit for bit.
//
// The error formatter, the 16-byte rounding, the descriptor words and the recipe of a device's part (MapSlot, MapFill) are host_map.h's,
// shared with the three map features; the layout (bits, not texels), the plan (words) and the checks (their own order) stay here.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_light.h"
#include "host_map.h"
#include "host_refit.h"
#include "host_tex.h"

#ifndef RPT_CUT_FN
#define RPT_CUT_FN inline
#endif

namespace rpthost {

constexpr uint32_t kCutDescWords = kMapDescWords;  // CutDesc below, as words
constexpr uint64_t kCutMaxTexels = kMapMaxTexels;  // of all masks of a scene
static_assert(RPT_MESH_CUTOUT_OFF == kMapOff && RPT_MESH_CUTOUT_ON == kMapOn, "host_map.h");
constexpr uint32_t kCutPadTexels = 128;         // a mask starts at a 16 B boundary and holds whole 64-texel waves

// One textured mesh, 16 B: one gather per candidate of a cutout mesh.  flags == 0: the mesh has no cutout (the rest is not read).
struct alignas(16) CutDesc {
    uint32_t first;                   // its first word in the mask table
    uint32_t width, height;           // of the mask
    uint32_t flags;                   // bit 0: ON; bit 1: the texture's wrap is RPT_TEX_WRAP_CLAMP
};

// The words one mask takes in the table: its bits, padded to kCutPadTexels texels.
RPT_CUT_FN uint32_t cut_mask_words(uint32_t width, uint32_t height)
{
    const uint64_t n = (uint64_t)width * height;
    return (uint32_t)(((n + (kCutPadTexels - 1u)) / kCutPadTexels) * (kCutPadTexels / 32u));
}

// Bit k of a mask: alpha >= threshold, an integer compare.
RPT_CUT_FN bool cut_opaque_byte(uint32_t alpha, uint32_t threshold) { return alpha >= threshold; }

// Bit k of the mask whose first word is `words`.
RPT_CUT_FN bool cut_bit(const uint32_t* words, uint32_t k) { return ((words[k >> 5] >> (k & 31u)) & 1u) != 0u; }

// The texel of the cut test (include/rpt.h, "cut test"): u and v are the triangle test's own, (sa, ta), (sb, tb), (sc, tc) the corners'
// UVs, `wrap` the texture's.  NEAREST whatever the colour filter.
RPT_CUT_FN uint32_t cut_texel(float u, float v, float sa, float ta, float sb, float tb, float sc, float tc, uint32_t width, uint32_t height,
                              uint32_t wrap)
{
    const float w = (1.0f - u) - v;
    const float s = tex_interp(w, u, v, sa, sb, sc);
    const float t = tex_interp(w, u, v, ta, tb, tc);
    const float x = tex_wrap(s, wrap), y = tex_wrap(t, wrap);
    const uint32_t i = tex_nearest_index(x, width, wrap), j = tex_nearest_index(y, height, wrap);
    return j * width + i;
}

// The plain-loop reference of the mask kernel: `alpha` (one byte per texel, row 0 first) -> cut_mask_words(width, height) words,
// the padding zero.
inline void cut_mask_reference(const uint8_t* alpha, uint32_t width, uint32_t height, uint32_t threshold, uint32_t* words)
{
    const uint32_t n_words = cut_mask_words(width, height);
    for (uint32_t w = 0; w < n_words; ++w) words[w] = 0u;
    const size_t n = (size_t)width * height;
    for (size_t k = 0; k < n; ++k)
        if (cut_opaque_byte(alpha[k], threshold)) words[k >> 5] |= 1u << (k & 31u);
}

// One mesh's cutout as the context remembers it (width == 0: OFF).
struct CutMask {
    uint32_t width = 0, height = 0, threshold = 0;
    uint64_t first = 0;               // its first word in the devices' mask table
};

// The device's cutout tables (DevState::cut), one allocation: per mesh of the SCENE 16 B (the descriptors, by texture ordinal); per
// triangle of the scene 4 B (the all-0xFFFFFFFF tri_light the render kernel reads while no mesh is ON); one bit per mask texel.
struct CutLayout {
    size_t off_desc = 0, off_none = 0, off_bits = 0, total = 0;
    CutLayout(uint32_t n_meshes, uint32_t n_tris, uint64_t n_words)
    {
        off_none = map_round16(4 * (size_t)kCutDescWords * n_meshes);
        off_bits = off_none + map_round16(4 * (size_t)n_tris);
        total = off_bits + 4 * (size_t)n_words;
    }
    size_t off_elems() const { return off_bits; }
    // the descriptors; the empty light table; the masks, whose padding stays zero
    std::vector<MapFill> fills() const { return {{0, off_none, 0}, {off_none, off_bits - off_none, 0xFF}, {off_bits, total - off_bits, 0}}; }
};

// What rpt_set_mesh_cutouts leaves on the host for the life of the cutouts.
struct CutPlan {
    std::vector<CutMask> mask;        // mesh -> its cutout; empty: every mesh OFF
    uint32_t n_meshes = 0, n_tris = 0;
    uint64_t n_words = 0;             // of all masks

    bool on(uint32_t mesh) const { return mesh < mask.size() && mask[mesh].width != 0u; }
    bool any() const
    {
        for (const CutMask& m : mask) if (m.width != 0u) return true;
        return false;
    }
    CutLayout layout() const { return CutLayout(n_meshes, n_tris, n_words); }     // of every device's tables
    std::vector<MapSlot> slots() const
    {
        std::vector<MapSlot> s(mask.size());
        for (size_t m = 0; m < mask.size(); ++m) s[m] = MapSlot{mask[m].first, mask[m].width ? cut_mask_words(mask[m].width, mask[m].height) : 0u};
        return s;
    }
};

// The plan of `mask` (one entry per mesh, `first` not yet set) over a scene.
inline void build_cut_plan(const RefitPlan& plan, std::vector<CutMask> mask, CutPlan& cp)
{
    cp = CutPlan();
    cp.mask = std::move(mask);
    cp.n_meshes = plan.n_meshes();
    cp.n_tris = plan.n_slots;
    cp.mask.resize(cp.n_meshes);
    for (CutMask& m : cp.mask) {
        if (m.width == 0u) continue;
        m.first = cp.n_words;
        cp.n_words += cut_mask_words(m.width, m.height);
    }
}

// The descriptor table of `cp` under the textures of `tp`: kCutDescWords per mesh of the scene, entry j the cutout of texture ordinal j.
inline std::vector<uint32_t> cut_desc_table(const CutPlan& cp, const TexPlan& tp)
{
    std::vector<uint32_t> d((size_t)kCutDescWords * cp.n_meshes, 0u);
    for (uint32_t j = 0; j < tp.n_tex() && j < cp.n_meshes; ++j) {
        const uint32_t m = tp.tex_mesh[j];
        if (cp.on(m)) map_desc_put(d, j, cp.mask[m], map_desc_flags(tp.image[m].wrap, RPT_TEX_FILTER_NEAREST));      // (no filter bit: the cut test is NEAREST)
    }
    return d;
}

// `err` = "rpt_set_mesh_cutouts: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int cut_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_mesh_cutouts", code, fmt, a...); }

// Every check of rpt_set_mesh_cutouts but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `mask` is `current` (empty:
// every mesh OFF) with the named meshes' new cutouts (`first` unset), one entry per mesh.  Never reads the items' alpha.
inline int check_mesh_cutouts(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const LightPlan& light, const rpt_mesh_cutout* items,
                              uint32_t n_items, const std::vector<CutMask>& current, std::vector<CutMask>& mask, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return cut_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!items && n_items) return cut_error(err, INVALID, "items is NULL");
    std::vector<CutMask> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_cutout& it = items[i];
        if (it.mesh >= plan.n_meshes()) return cut_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return cut_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        if (it.mode != RPT_MESH_CUTOUT_OFF && it.mode != RPT_MESH_CUTOUT_ON)
            return cut_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_CUTOUT_OFF nor RPT_MESH_CUTOUT_ON", i, it.mode, it.mesh);
        if (it.mode == RPT_MESH_CUTOUT_OFF) {
            if (it.width != 0u || it.height != 0u || it.alpha)
                return cut_error(err, INVALID, "item %u: mesh %u: RPT_MESH_CUTOUT_OFF takes width == height == 0 and alpha == NULL", i, it.mesh);
            next[it.mesh] = CutMask();
            continue;
        }
        if (it.width == 0u || it.height == 0u || it.width > kTexMaxSide || it.height > kTexMaxSide)
            return cut_error(err, INVALID, "item %u: mesh %u: a mask of %u x %u (each side must lie in 1 .. 16384)", i, it.mesh, it.width, it.height);
        if (!it.alpha) return cut_error(err, INVALID, "item %u: mesh %u: alpha is NULL", i, it.mesh);
        if (it.threshold < 1u || it.threshold > 255u)
            return cut_error(err, INVALID, "item %u: mesh %u: threshold %u (it must lie in 1 .. 255)", i, it.mesh, it.threshold);
        if (!tex.textured(it.mesh))
            return cut_error(err, INVALID, "item %u: mesh %u is untextured: a cutout takes its UVs and wrap from the mesh's texture (a 1 x 1 white texture is enough: rpt_set_mesh_textures)", i, it.mesh);
        if (light.on(it.mesh))
            return cut_error(err, RPT_ERR_UNSUPPORTED, "item %u: mesh %u is a mesh light: next-event estimation would sample points inside holes", i, it.mesh);
        CutMask c;
        c.width = it.width; c.height = it.height; c.threshold = it.threshold;
        next[it.mesh] = c;
    }
    uint64_t total = 0;
    for (const CutMask& c : next) total += (uint64_t)c.width * c.height;
    if (total > kCutMaxTexels)
        return cut_error(err, RPT_ERR_UNSUPPORTED, "the scene's masks would hold %llu texels: more than 2^26 in all", (unsigned long long)total);
    mask = std::move(next);
    return RPT_OK;
}

}  // namespace rpthost
