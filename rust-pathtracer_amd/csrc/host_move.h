// host_move.h — the host half of rpt_update_meshes_device / rpt_rebuild_meshes_device (include/rpt.h, "moving meshes from device
// memory"): the one statement of the per-mesh transform, the words the device check reduces, the host checks of a call, and a host
// reference of the two kernels.  Plain C++ with no HIP type in it, like host_refit.h: capi.hip includes it, k_move.hip compiles the
// RPT_MOVE_FN functions for the device (as k_build.hip compiles host_build.h's rules), and tests/move_harness.cpp runs this file
// under the address and undefined-behaviour sanitizers (tests/test_mesh_move_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off: the transform is three multiplies and three adds
// per component, each rounded to f32, in the order written.  The checks format their messages with host_map.h's call_error
// under the name of the call they were made for.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_map.h"
#include "host_refit.h"

#ifndef RPT_MOVE_FN
#define RPT_MOVE_FN inline
#endif

namespace rpthost {

// A source's transform as the kernels take it: the twelve floats (rows of a 3x4 matrix) and whether there is one at all.
struct MoveTransform {
    float t[12];
    uint32_t on;                               // 0: rpt_mesh_source.transform was NULL — the positions are taken as they are
};

RPT_MOVE_FN uint32_t move_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// THE statement (include/rpt.h): out[c] = ((t[4c]*x + t[4c+1]*y) + t[4c+2]*z) + t[4c+3].  `out` may not alias `p`.
RPT_MOVE_FN void move_point(const float* t, const float* p, float* out)
{
    const float x = p[0], y = p[1], z = p[2];
    for (int c = 0; c < 3; ++c) out[c] = ((t[4 * c] * x + t[4 * c + 1] * y) + t[4 * c + 2] * z) + t[4 * c + 3];
}

// One vertex of a source: the position the context will hold.  Without a transform the three words are copied (a -0 stays -0).
RPT_MOVE_FN void move_vertex(const MoveTransform& xf, const float* p, float* out)
{
    if (xf.on) move_point(xf.t, p, out);
    else { out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; }
}

// The two words the check reduces per named mesh, both by an unsigned max over words the host zeroed (max commutes: the result does
// not depend on the order):
//   kMoveWordBig   the largest |coordinate| over the mesh's REFERENCED vertices, as the bit pattern of a non-negative float (which
//                  orders like the float; 0: none)
//   kMoveWordBad   0xFFFFFFFF - v for the lowest vertex v with a coordinate that is not finite, referenced or not (0: none; a mesh
//                  has fewer than 2^32 - 1 vertices, so the word of a vertex is never 0)
constexpr uint32_t kMoveWordBig = 0u, kMoveWordBad = 1u, kMoveWords = 2u;

// what one vertex adds to the two words: `p` is its position AFTER the transform
RPT_MOVE_FN void move_vertex_words(const float* p, uint32_t vertex, bool referenced, uint32_t& big, uint32_t& bad)
{
    for (int c = 0; c < 3; ++c) {
        const uint32_t mag = move_bits(p[c]) & 0x7FFFFFFFu;
        if (mag >= 0x7F800000u) { const uint32_t w = 0xFFFFFFFFu - vertex; bad = w > bad ? w : bad; }
        if (referenced && mag > big) big = mag;
    }
}

inline float move_big_of(uint32_t word)
{
    float f;
    __builtin_memcpy(&f, &word, 4);
    return f;
}

// The device's tables of the device-source calls (DevState::move), one allocation on the context's first device, from its first
// device-source call to the next upload: two words per mesh, then RefitPlan::referenced (one byte per vertex).
struct MoveLayout {
    size_t off_words = 0, off_referenced = 0, total = 0;
    MoveLayout(uint32_t n_meshes, uint32_t n_vertices)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_referenced = round16(4 * (size_t)kMoveWords * n_meshes);
        total = off_referenced + round16((size_t)n_vertices);
        if (total == 0) total = 16;
    }
};

// Is `p` device memory with `bytes` bytes of its allocation from `p` on, and on which device?  capi.hip answers with
// hipPointerGetAttributes and hipMemGetAddressRange; the harness with a table.
constexpr int kMoveSourceOk = 0, kMoveSourceNotDevice = 1, kMoveSourceShort = 2;
typedef int (*MoveSourceQuery)(const void* p, size_t bytes, int* device);

// Every host check of a device-source call but the NULL context (include/rpt.h), in one fixed order, mirroring check_mesh_update:
// a call with several faults always answers the first.  RPT_OK: `devices[u]` is the device that holds source u (-1 for a source
// without vertices).  n_sources > 0.  No device memory is read.
inline int check_mesh_sources(const RefitPlan& plan, bool mesh_scene, const rpt_mesh_source* sources, uint32_t n_sources, MoveSourceQuery query,
                              const char* call, std::vector<int>& devices, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!sources) return call_error(err, call, INVALID, "sources is NULL");
    if (!mesh_scene) return call_error(err, call, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!plan.ok) return call_error(err, call, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    devices.assign(n_sources, -1);
    for (uint32_t u = 0; u < n_sources; ++u) {
        const rpt_mesh_source& so = sources[u];
        if (so.mesh >= plan.n_meshes()) return call_error(err, call, INVALID, "source %u: mesh %u out of range (the scene has %u)", u, so.mesh, plan.n_meshes());
        if (named[so.mesh]) return call_error(err, call, INVALID, "source %u: mesh %u is named twice", u, so.mesh);
        named[so.mesh] = 1;
        const uint32_t count = plan.mesh_first[so.mesh + 1u] - plan.mesh_first[so.mesh];
        if (so.n_vertices != count) return call_error(err, call, INVALID, "mesh %u: n_vertices %u != the uploaded mesh's %u", so.mesh, so.n_vertices, count);
        if (count && !so.vertices_dev) return call_error(err, call, INVALID, "mesh %u: vertices_dev is NULL", so.mesh);
        const int where = count ? query(so.vertices_dev, 12 * (size_t)count, &devices[u]) : kMoveSourceOk;
        if (where == kMoveSourceNotDevice) return call_error(err, call, INVALID, "mesh %u: vertices_dev is not device memory", so.mesh);
        if (where != kMoveSourceOk)
            return call_error(err, call, INVALID, "mesh %u: vertices_dev's allocation ends before %u vertices (%zu bytes)", so.mesh, count, 12 * (size_t)count);
        if (so.transform)
            for (int k = 0; k < 12; ++k)
                if ((move_bits(so.transform[k]) & 0x7FFFFFFFu) >= 0x7F800000u)
                    return call_error(err, call, INVALID, "mesh %u: transform entry %d is not finite", so.mesh, k);
    }
    return RPT_OK;
}

inline MoveTransform move_transform_of(const float* transform)
{
    MoveTransform xf = {};
    if (transform) { for (int k = 0; k < 12; ++k) xf.t[k] = transform[k]; xf.on = 1u; }
    return xf;
}

// What the device check's read-back says about source `so`: RPT_OK and the mesh's largest |coordinate|, or the error.
inline int move_check_result(const rpt_mesh_source& so, const uint32_t* words, const char* call, float& big, std::string& err)
{
    if (words[kMoveWordBad]) return call_error(err, call, RPT_ERR_INVALID_ARG, "mesh %u vertex %u is not finite", so.mesh, 0xFFFFFFFFu - words[kMoveWordBad]);
    big = move_big_of(words[kMoveWordBig]);
    return RPT_OK;
}

// ---- the two kernels on the host, statement for statement (k_move.hip) -------------------------------------------------------------
// meshmove_check_kernel over one source: `words` (kMoveWords of them) start as the host zeroed them.
inline void move_check_reference(const float* src, uint32_t n, const MoveTransform& xf, const uint8_t* referenced, uint32_t* words)
{
    for (uint32_t v = 0; v < n; ++v) {
        float p[3];
        move_vertex(xf, src + 3 * (size_t)v, p);
        move_vertex_words(p, v, referenced[v] != 0, words[kMoveWordBig], words[kMoveWordBad]);
    }
}

// meshmove_apply_kernel over one source
inline void move_apply_reference(const float* src, uint32_t n, const MoveTransform& xf, float* dst)
{
    for (uint32_t v = 0; v < n; ++v) move_vertex(xf, src + 3 * (size_t)v, dst + 3 * (size_t)v);
}

}  // namespace rpthost
