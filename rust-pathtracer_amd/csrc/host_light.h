// host_light.h — the host half of mesh lights (include/rpt.h, "mesh lights"): the statement of an ON mesh's table (areas, exponent,
// quanta, CDF, total area) as plain functions, the plan rpt_set_mesh_lights makes (the ON list in ascending mesh order, the table
// offsets, what every device gets), its checks, and a host reference of the table.  Plain C++ with no HIP type in it, like
// host_smooth.h: capi.hip includes it, k_light.hip compiles the RPT_LIGHT_FN functions for the device, and tests/light_harness.cpp
// runs this file under the address and undefined-behaviour sanitizers (tests/test_mesh_light_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off; the square root is the correctly rounded one.
//
// Numbering.  The triangles of the ON meshes, ON meshes in ascending mesh index and each mesh's triangles in its own order, are the
// FACES 0 .. n_faces - 1; the j-th ON mesh is ORDINAL j.  Nothing here knows a slot: a rebuild leaves every table bit for bit.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_map.h"
#include "host_refit.h"
#include "host_smooth.h"

#ifndef RPT_LIGHT_FN
#define RPT_LIGHT_FN inline
#endif

namespace rpthost {

constexpr uint32_t kLightNone = 0xFFFFFFFFu;
constexpr uint32_t kLightDescWords = 8;        // launch_light.h, LightMeshDesc: {first face, n, material, A_tot, E, A_max (scratch), -, -}
constexpr uint32_t kLightScanBlock = 256;      // faces per workgroup of the scan (k_light.hip)
constexpr uint64_t kLightMaxPick = 1ull << 24; // n_lights + ON meshes stays below it: the index draw has 24 bits

// A_k = !(l2 > 0 && l2 <= F::MAX) ? 0 : 0.5f * sqrt(l2), l2 = dot(g, g), g = cross(b - a, c - a)
RPT_LIGHT_FN float light_tri_area(const float* a, const float* b, const float* c)
{
    float g[3];
    smooth_face_vector(a, b, c, g);
    const float l2 = smooth_dot(g, g);
    if (!(l2 > 0.0f && l2 <= kSmoothFMax)) return 0.0f;
    return 0.5f * __builtin_sqrtf(l2);
}

// E with a_max = f * 2^E, f in [0.5, 1).  a_max > 0 is an area, at least 0.5 * sqrt(2^-149): never subnormal, so the exponent
// field says it.  a_max == 0 (a dark mesh): 0.
RPT_LIGHT_FN int32_t light_exponent(float a_max)
{
    uint32_t u;
    __builtin_memcpy(&u, &a_max, 4);
    return u == 0u ? 0 : (int32_t)((u >> 23) & 255u) - 126;
}

// q_k = floor(A_k * 2^(36 - E)) — the product is exact in float64 (a 24-bit significand times a power of two, far from the ends of
// the range: E lies in [-75, 128]), and the conversion truncates a non-negative value.
RPT_LIGHT_FN uint64_t light_quantum(float area, int32_t e)
{
    const uint64_t bits = (uint64_t)(1023 + 36 - e) << 52;
    double scale;
    __builtin_memcpy(&scale, &bits, 8);
    return (uint64_t)((double)area * scale);
}

// A_tot = f32(Q) * 2^(E - 36): the conversion rounds to nearest even, the product is exact or overflows to +inf.
RPT_LIGHT_FN float light_total_area(uint64_t q, int32_t e)
{
    const uint32_t bits = (uint32_t)(127 + e - 36) << 23;
    float scale;
    __builtin_memcpy(&scale, &bits, 4);
    return (float)q * scale;
}

// The device's mesh light tables (DevState::light), one allocation.  Per ON mesh 32 B; per face 36 B (its CDF entry and the scan's
// partial sum, 8 B each, its area, 4 B, its corners, 12 B, its ordinal, 4 B) and 8 B per 256 faces (the scan's block sums); per
// triangle of the SCENE 4 B (the hit side's lookup) and one bit (the all-FLAT smooth bits the render kernel reads while no mesh is
// SMOOTH).
struct LightLayout {
    size_t off_desc = 0, off_cdf = 0, off_part = 0, off_block = 0, off_area = 0, off_face_vertex = 0, off_face_mesh = 0, off_tri_light = 0,
           off_flat_bits = 0, total = 0;
    uint32_t n_blocks = 0;
    LightLayout(uint32_t n_on, uint32_t n_faces, uint32_t n_tris)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        n_blocks = (uint32_t)(((size_t)n_faces + kLightScanBlock - 1) / kLightScanBlock);
        off_cdf = round16(4 * (size_t)kLightDescWords * n_on);
        off_part = off_cdf + round16(8 * (size_t)n_faces);
        off_block = off_part + round16(8 * (size_t)n_faces);
        off_area = off_block + round16(8 * (size_t)n_blocks);
        off_face_vertex = off_area + round16(4 * (size_t)n_faces);
        off_face_mesh = off_face_vertex + round16(12 * (size_t)n_faces);
        off_tri_light = off_face_mesh + round16(4 * (size_t)n_faces);
        off_flat_bits = off_tri_light + round16(4 * (size_t)n_tris);
        total = off_flat_bits + round16(4 * (((size_t)n_tris + 31) / 32));
    }
};

// What rpt_set_mesh_lights leaves on the host for the life of the modes, and (the staging vectors) what every device gets.
struct LightPlan {
    std::vector<uint8_t> mode;                 // mesh -> RPT_MESH_LIGHT_*; empty: every mesh OFF
    uint32_t n_tris = 0;                       // of the scene
    uint32_t n_faces = 0;
    std::vector<uint32_t> on_mesh;             // ordinal -> mesh, ascending
    std::vector<uint32_t> on_first;            // ordinal -> its first face; n_on + 1 entries
    // staging: released once every device holds it
    std::vector<uint32_t> desc;                // kLightDescWords per ordinal: first face, n, material; the rest 0 (the device fills it)
    std::vector<uint32_t> face_vertex;         // [3][n_faces]: face -> its corners a, b, c in the concatenated vertex array
    std::vector<uint32_t> face_mesh;           // face -> its ordinal
    std::vector<uint32_t> tri_light;           // flattened triangle -> its mesh's ordinal, or kLightNone

    uint32_t n_on() const { return (uint32_t)on_mesh.size(); }
    bool any() const
    {
        for (uint8_t m : mode) if (m == RPT_MESH_LIGHT_ON) return true;
        return false;
    }
    bool on(uint32_t mesh) const { return mesh < mode.size() && mode[mesh] == RPT_MESH_LIGHT_ON; }
    // the ordinal of an ON mesh (kLightNone: it is OFF)
    uint32_t ordinal(uint32_t mesh) const
    {
        for (uint32_t j = 0; j < n_on(); ++j) if (on_mesh[j] == mesh) return j;
        return kLightNone;
    }
    void release_staging()
    {
        std::vector<uint32_t>().swap(desc);
        std::vector<uint32_t>().swap(face_vertex);
        std::vector<uint32_t>().swap(face_mesh);
        std::vector<uint32_t>().swap(tri_light);
    }
    LightLayout layout() const { return LightLayout(n_on(), n_faces, n_tris); }     // of every device's tables
};

// The plan of `mode` over a scene's flattened triangles (`flat`: 3 corners each, concatenated vertex indices).
inline void build_light_plan(const RefitPlan& plan, const uint32_t* flat, const std::vector<uint8_t>& mode, LightPlan& lp)
{
    lp = LightPlan();
    lp.mode = mode;
    lp.n_tris = plan.n_slots;
    lp.tri_light.assign(lp.n_tris, kLightNone);
    lp.on_first.push_back(0u);
    for (uint32_t m = 0; m < plan.n_meshes(); ++m) {
        if (!lp.on(m)) continue;
        lp.on_mesh.push_back(m);
        lp.n_faces += plan.tri_first[m + 1u] - plan.tri_first[m];
        lp.on_first.push_back(lp.n_faces);
    }
    const size_t nf = lp.n_faces;
    lp.desc.assign((size_t)kLightDescWords * lp.n_on(), 0u);
    lp.face_vertex.resize(3 * nf);
    lp.face_mesh.resize(nf);
    size_t f = 0;
    for (uint32_t j = 0; j < lp.n_on(); ++j) {
        const uint32_t m = lp.on_mesh[j];
        uint32_t* d = &lp.desc[(size_t)kLightDescWords * j];
        d[0] = lp.on_first[j];
        d[1] = plan.tri_first[m + 1u] - plan.tri_first[m];
        d[2] = plan.mesh_material[m];
        for (uint32_t k = plan.tri_first[m]; k < plan.tri_first[m + 1u]; ++k, ++f) {
            lp.tri_light[k] = j;
            lp.face_mesh[f] = j;
            for (size_t c = 0; c < 3; ++c) lp.face_vertex[c * nf + f] = flat[3 * (size_t)k + c];
        }
    }
}

// `err` = "rpt_set_mesh_lights: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int light_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_mesh_lights", code, fmt, a...); }

// Every check of rpt_set_mesh_lights but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `mode` is `current` (empty:
// every mesh OFF) with the named meshes' new modes, one entry per mesh.  The 2^24 rule comes before the items' own checks, so it
// counts what the well-formed items would leave ON (an item whose mesh or mode is out of range counts as absent, a mesh named
// twice with its last mode): exactly the new state whenever the call would otherwise be accepted.
inline int check_mesh_lights(const RefitPlan& plan, bool mesh_scene, uint32_t scene_flags, uint32_t n_lights, const rpt_mesh_light* items,
                             uint32_t n_items, const std::vector<uint8_t>& current, std::vector<uint8_t>& mode, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return light_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!(scene_flags & RPT_SCENE_ANYHIT_USES_MAX_DIST))
        return light_error(err, RPT_ERR_UNSUPPORTED, "the scene lacks RPT_SCENE_ANYHIT_USES_MAX_DIST: a mesh light's own triangles would occlude every shadow ray aimed at them");
    if (!plan.ok) return light_error(err, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    std::vector<uint8_t> would(current);
    would.resize(plan.n_meshes(), (uint8_t)RPT_MESH_LIGHT_OFF);
    for (uint32_t i = 0; items && i < n_items; ++i)
        if (items[i].mesh < plan.n_meshes() && (items[i].mode == RPT_MESH_LIGHT_OFF || items[i].mode == RPT_MESH_LIGHT_ON))
            would[items[i].mesh] = (uint8_t)items[i].mode;
    uint64_t n_on = 0;
    for (uint8_t m : would) n_on += m == RPT_MESH_LIGHT_ON ? 1u : 0u;
    if ((uint64_t)n_lights + n_on >= kLightMaxPick)
        return light_error(err, RPT_ERR_UNSUPPORTED, "%u lights and %llu ON meshes: the pickable lights must stay below 2^24", n_lights, (unsigned long long)n_on);
    if (!items && n_items) return light_error(err, INVALID, "items is NULL");
    mode = current;
    mode.resize(plan.n_meshes(), (uint8_t)RPT_MESH_LIGHT_OFF);
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_light& it = items[i];
        if (it.mesh >= plan.n_meshes()) return light_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return light_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        if (it.mode != RPT_MESH_LIGHT_OFF && it.mode != RPT_MESH_LIGHT_ON)
            return light_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_LIGHT_OFF nor RPT_MESH_LIGHT_ON", i, it.mode, it.mesh);
        mode[it.mesh] = (uint8_t)it.mode;
    }
    return RPT_OK;
}

// ---- the host reference: what k_light.hip's table kernels compute for ordinal j, statement for statement ---------------------------
// `vertices`: xyz per concatenated vertex; `cdf`: one entry per triangle of the mesh.  (Needs the plan's staging.)
inline void light_table_reference(const float* vertices, const LightPlan& lp, uint32_t j, uint64_t* cdf, int32_t* exponent, float* area)
{
    const size_t nf = lp.n_faces, first = lp.on_first[j], n = lp.on_first[j + 1u] - first;
    std::vector<float> a(n);
    float a_max = 0.0f;
    for (size_t k = 0; k < n; ++k) {
        const size_t f = first + k;
        a[k] = light_tri_area(vertices + 3 * (size_t)lp.face_vertex[f], vertices + 3 * (size_t)lp.face_vertex[nf + f],
                              vertices + 3 * (size_t)lp.face_vertex[2 * nf + f]);
        if (a[k] > a_max) a_max = a[k];
    }
    const int32_t e = light_exponent(a_max);
    uint64_t sum = 0;
    for (size_t k = 0; k < n; ++k) { sum += light_quantum(a[k], e); cdf[k] = sum; }
    const float a_tot = light_total_area(sum, e);
    const bool dark = !(a_max > 0.0f) || !(a_tot <= kSmoothFMax);
    if (dark) for (size_t k = 0; k < n; ++k) cdf[k] = 0;
    *exponent = dark ? 0 : e;
    *area = dark ? 0.0f : a_tot;
}

}  // namespace rpthost
