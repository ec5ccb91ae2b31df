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
//
// The layout, the plan, the descriptor table and the order of the checks are host_map.h's (MapLayout, MapPlan, map_desc_table,
// check_mesh_maps), shared with the material and the emission maps; here are the names, the map's own fields and its own checks.
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

#ifndef RPT_NRM_FN
#define RPT_NRM_FN inline
#endif

namespace rpthost {

constexpr uint32_t kNrmDescWords = kMapDescWords;  // NrmDesc below, as words
constexpr uint64_t kNrmMaxTexels = kMapMaxTexels;  // of all maps of a scene
static_assert(RPT_MESH_NORMAL_MAP_OFF == kMapOff && RPT_MESH_NORMAL_MAP_ON == kMapOn, "host_map.h");
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

// The device's map tables (DevState::nrm): host_map.h's, whose all-0xFFFFFFFF tri_light the render kernel reads while no mesh is ON and
// no cutout or environment supplies one.
using NrmLayout = MapLayout;

// What rpt_set_mesh_normal_maps leaves on the host for the life of the maps.
using NrmPlan = MapPlan<NrmMap>;

// The plan of `map` (one entry per mesh, `first` not yet set) over a scene.
inline void build_nrm_plan(const RefitPlan& plan, std::vector<NrmMap> map, NrmPlan& np) { build_map_plan(plan.n_meshes(), plan.n_slots, std::move(map), np); }

// The descriptor table of `np` under the textures of `tp`: kNrmDescWords per mesh of the scene, entry j the map of texture ordinal j.
inline std::vector<uint32_t> nrm_desc_table(const NrmPlan& np, const TexPlan& tp) { return map_desc_table(np, tp); }

constexpr MapNames kNrmNames = {"rpt_set_mesh_normal_maps", "RPT_MESH_NORMAL_MAP", "a normal map", "normal maps"};

// Every check of rpt_set_mesh_normal_maps but the NULL context (include/rpt.h), in check_mesh_maps' order with the flags and the
// strength in the feature's place.  RPT_OK: `map` is `current` (empty: every mesh OFF) with the named meshes' new maps (`first` unset),
// one entry per mesh.  Never reads the items' texels.
inline int check_mesh_normal_maps(const RefitPlan& plan, bool mesh_scene, const TexPlan& tex, const rpt_mesh_normal_map* items, uint32_t n_items,
                                  const std::vector<NrmMap>& current, std::vector<NrmMap>& map, std::string& err)
{
    const auto own = [](uint32_t i, const rpt_mesh_normal_map& it, bool, NrmMap& c, std::string& err) {
        const int INVALID = RPT_ERR_INVALID_ARG;
        const char* call = kNrmNames.call;
        if (it.flags & ~(uint32_t)RPT_NORMAL_MAP_FLIP_GREEN)
            return call_error(err, call, INVALID, "item %u: mesh %u: unknown flag bits 0x%x", i, it.mesh, it.flags & ~(uint32_t)RPT_NORMAL_MAP_FLIP_GREEN);
        if (!tex_finite(it.strength) || !(it.strength >= 0.0f) || it.strength > kNrmMaxStrength)
            return call_error(err, call, INVALID, "item %u: mesh %u: strength %g (it must be finite and lie in 0 .. 16)", i, it.mesh, (double)it.strength);
        c.flags = it.flags; c.strength = it.strength;
        return (int)RPT_OK;
    };
    return check_mesh_maps(kNrmNames, plan, mesh_scene, tex, items, n_items, current, map, err, own);
}

}  // namespace rpthost
