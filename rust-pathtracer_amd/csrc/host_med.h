// host_med.h — the host half of mesh media (include/rpt.h, "mesh media"): the checks of rpt_set_mesh_media in their one order, the
// clamp, the plan the call makes (which meshes carry a medium, each one's ordinal, what every device gets) and the two tables: one
// row per medium-carrying mesh and one ordinal per triangle of the scene.  Plain C++ with no HIP type in it, like host_light.h:
// capi.hip includes it, k_med.hip compiles the RPT_MED_FN functions for the device, and tests/med_harness.cpp runs this file on the
// host (tests/test_mesh_media_host.py).
//
// Numbering.  The meshes that carry a medium other than NONE, in ascending mesh index, are ORDINALS 0 .. n_media - 1: the row of the
// medium table, and what a path remembers (dev_media.h, PathRegs.medium = 1 + ordinal).  tri_medium is indexed by the FLATTENED
// triangle index, never by a slot: a move or a rebuild leaves both tables bit for bit.
//
// The empty tables.  The eight media forms sit over the emission-mapped forms (launch_med.h), which sit over the material-mapped,
// textured, mesh-light forms.  A scene with a medium and none of those features takes them through tables this allocation carries:
// a block laid out as an emission-map allocation with no map ON (host_emap.h, EmapLayout(n_meshes, n_tris, 0): all-zero descriptors
// in both tables, the zero block of the material maps with its all-0xFFFFFFFF table) and all-zero smooth bits.  mesh_args_med.h
// lends each exactly while the feature it stands for is absent.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_emap.h"
#include "host_map.h"
#include "host_refit.h"

#ifndef RPT_MED_FN
#define RPT_MED_FN inline
#endif

namespace rpthost {

constexpr uint32_t kMedNone = 0xFFFFu;          // tri_medium of a triangle whose mesh carries no medium (dev_media.h, kNoMediumIdx)
constexpr uint32_t kMedMaxMedia = 0x7FFEu;      // meshes that may carry one: what a path can remember (dev_media.h, kMaxMediaMaterials)
constexpr uint32_t kMedRowWords = 8;            // MedRow below, as words

// One medium-carrying mesh, 32 B: two gathers per use.
struct alignas(16) MedRow {
    uint32_t type;                    // RPT_MEDIUM_ABSORB, _SCATTER or _EMISSIVE: never NONE
    float density;
    float color[3];
    float anisotropy;                 // already clamped
    uint32_t mesh;                    // whose medium this is (rpt_download_mesh_medium does not need it; a reader of the table does)
    uint32_t pad;
};
static_assert(sizeof(MedRow) == 4 * kMedRowWords, "MedRow is 8 words");

RPT_MED_FN bool med_finite(float x) { return x - x == 0.0f; }

// Material::finalize's clamp (material.rs:126): f32::clamp of a finite value.
RPT_MED_FN float med_clamp_anisotropy(float g) { return g < -0.9f ? -0.9f : (g > 0.9f ? 0.9f : g); }

// The medium ordinal of flattened triangle `index` (kMedNone: its mesh carries none).
RPT_MED_FN uint32_t med_ordinal_of(const uint32_t* tri_medium, uint32_t index) { return tri_medium[index]; }

// One mesh's medium as the context remembers it (type NONE: none).
struct MedEntry {
    uint32_t type = RPT_MEDIUM_NONE;
    float density = 0.0f;
    float color[3] = {0.0f, 0.0f, 0.0f};
    float anisotropy = 0.0f;          // clamped
};

// The device's media tables (DevState::med), one allocation: per medium 32 B; per triangle of the scene 4 B (its ordinal) and one
// bit (all-zero smooth bits); then the empty emission-map block (the top of this file).
struct MedLayout {
    size_t off_rows = 0, off_tri_medium = 0, off_flat_bits = 0, off_emap = 0, total = 0;
    EmapLayout emap;
    MedLayout(uint32_t n_media, uint32_t n_meshes, uint32_t n_tris) : emap(n_meshes, n_tris, 0)
    {
        off_tri_medium = map_round16(4 * (size_t)kMedRowWords * n_media);
        off_flat_bits = off_tri_medium + map_round16(4 * (size_t)n_tris);
        off_emap = off_flat_bits + map_round16(4 * (((size_t)n_tris + 31) / 32));
        total = off_emap + map_round16(emap.total);
    }
    size_t off_all_ones() const { return off_emap + emap.off_zero + emap.zero.off_none; }      // n_tris words of 0xFFFFFFFF
};

// What rpt_set_mesh_media leaves on the host for the life of the media.
struct MedPlan {
    std::vector<MedEntry> medium;     // mesh -> its medium; empty: no mesh carries one
    uint32_t n_meshes = 0, n_tris = 0;
    std::vector<uint32_t> on_mesh;    // ordinal -> mesh, ascending
    EmapPlan zero_emap;               // the plan of the empty emission-map block: no map ON, the scene's sizes
    // staging: released once every device holds it
    std::vector<uint32_t> rows;       // kMedRowWords per ordinal
    std::vector<uint32_t> tri_medium; // flattened triangle -> its mesh's ordinal, or kMedNone

    uint32_t n_media() const { return (uint32_t)on_mesh.size(); }
    bool on(uint32_t mesh) const { return mesh < medium.size() && medium[mesh].type != RPT_MEDIUM_NONE; }
    bool any() const
    {
        for (const MedEntry& m : medium) if (m.type != RPT_MEDIUM_NONE) return true;
        return false;
    }
    void release_staging()
    {
        std::vector<uint32_t>().swap(rows);
        std::vector<uint32_t>().swap(tri_medium);
    }
    MedLayout layout() const { return MedLayout(n_media(), n_meshes, n_tris); }     // of every device's tables
};

// The plan of `medium` (one entry per mesh) over a scene whose mesh m owns the flattened triangles tri_first[m] .. tri_first[m + 1).
inline void build_med_plan(const RefitPlan& plan, std::vector<MedEntry> medium, MedPlan& mp)
{
    mp = MedPlan();
    mp.medium = std::move(medium);
    mp.n_meshes = plan.n_meshes();
    mp.n_tris = plan.n_slots;
    mp.medium.resize(mp.n_meshes);
    build_emap_plan(plan, std::vector<EmapMap>(), mp.zero_emap);
    mp.tri_medium.assign(mp.n_tris, kMedNone);
    for (uint32_t m = 0; m < mp.n_meshes; ++m) {
        if (!mp.on(m)) continue;
        const uint32_t ord = mp.n_media();
        mp.on_mesh.push_back(m);
        const MedEntry& e = mp.medium[m];
        MedRow r;
        r.type = e.type; r.density = e.density;
        r.color[0] = e.color[0]; r.color[1] = e.color[1]; r.color[2] = e.color[2];
        r.anisotropy = e.anisotropy; r.mesh = m; r.pad = 0u;
        uint32_t w[kMedRowWords];
        memcpy(w, &r, sizeof(r));
        mp.rows.insert(mp.rows.end(), w, w + kMedRowWords);
        for (uint32_t k = plan.tri_first[m]; k < plan.tri_first[m + 1u]; ++k) mp.tri_medium[k] = ord;
    }
}

template <class... A>
inline int med_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_mesh_media", code, fmt, a...); }

// Every check of rpt_set_mesh_media but the NULL context (include/rpt.h, "mesh media"), in one fixed order: the scene, the NULL
// items, then item by item (mesh range, named twice, type, density, colour, anisotropy), and last — on what the call would leave —
// how many meshes a path can remember.  RPT_OK: `medium` is `current` (empty: no mesh carries one) with the named meshes' new media,
// anisotropy clamped, one entry per mesh.  Any other answer leaves `medium` untouched.
inline int check_mesh_media(const RefitPlan& plan, bool mesh_scene, const rpt_mesh_medium* items, uint32_t n_items, const std::vector<MedEntry>& current,
                            std::vector<MedEntry>& medium, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return med_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!plan.ok) return med_error(err, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    if (!items && n_items) return med_error(err, INVALID, "items is NULL");
    std::vector<MedEntry> next(current);
    next.resize(plan.n_meshes());
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_medium& it = items[i];
        if (it.mesh >= plan.n_meshes()) return med_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return med_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        if (it.medium_type > (uint32_t)RPT_MEDIUM_EMISSIVE) return med_error(err, INVALID, "item %u: medium_type %u of mesh %u is no RPT_MEDIUM_*", i, it.medium_type, it.mesh);
        if (!med_finite(it.density) || it.density < 0.0f) return med_error(err, INVALID, "item %u: mesh %u: density %g (it must be finite and not negative)", i, it.mesh, (double)it.density);
        if (!med_finite(it.color[0]) || !med_finite(it.color[1]) || !med_finite(it.color[2]))
            return med_error(err, INVALID, "item %u: mesh %u: the colour is not finite", i, it.mesh);
        if (!med_finite(it.anisotropy)) return med_error(err, INVALID, "item %u: mesh %u: the anisotropy is not finite", i, it.mesh);
        MedEntry& e = next[it.mesh];
        e = MedEntry();
        if (it.medium_type != RPT_MEDIUM_NONE) {
            e.type = it.medium_type;
            e.density = it.density;
            e.color[0] = it.color[0]; e.color[1] = it.color[1]; e.color[2] = it.color[2];
            e.anisotropy = med_clamp_anisotropy(it.anisotropy);
        }
    }
    uint64_t n_on = 0;
    for (const MedEntry& e : next) n_on += e.type != RPT_MEDIUM_NONE ? 1u : 0u;
    if (n_on > kMedMaxMedia) return med_error(err, RPT_ERR_UNSUPPORTED, "%llu meshes would carry a medium: a path can remember %u", (unsigned long long)n_on, kMedMaxMedia);
    medium = std::move(next);
    return RPT_OK;
}

// rpt_download_mesh_medium's answer for `mesh` (in range): what the context holds, NONE and zeros for a mesh without one.
inline void med_item_of(const MedPlan& mp, uint32_t mesh, rpt_mesh_medium& out)
{
    const MedEntry e = mesh < mp.medium.size() ? mp.medium[mesh] : MedEntry();
    out.mesh = mesh;
    out.medium_type = e.type;
    out.density = e.density;
    out.color[0] = e.color[0]; out.color[1] = e.color[1]; out.color[2] = e.color[2];
    out.anisotropy = e.anisotropy;
}

}  // namespace rpthost
