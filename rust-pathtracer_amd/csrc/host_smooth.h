// host_smooth.h — the host half of smooth mesh shading (include/rpt.h, "smooth mesh shading"): the statement of a vertex normal as
// plain functions, the adjacency the device's vertex pass walks, the checks of rpt_set_mesh_shading, and a host reference of both
// normal statements.  Plain C++ with no HIP type in it, like host_refit.h: capi.hip includes it, k_smooth.hip compiles the
// RPT_SMOOTH_FN functions for the device (as k_move.hip compiles host_move.h's), and tests/smooth_harness.cpp runs this file under
// the address and undefined-behaviour sanitizers (tests/test_mesh_smooth_host.py).
//
// Every translation unit that includes this file is built with -ffp-contract=off: a cross product is six multiplies and three
// subtractions, each rounded to f32, in the order written; the square root and the divides are the correctly rounded ones.
//
// Numbering.  The triangles of the SMOOTH meshes, in flattened order, are the FACES 0 .. n_faces - 1: a mesh's triangles stay in the
// mesh's own order, so "ascending triangle index" and "ascending face" are the same order.  Nothing here knows a slot: a rebuild
// reorders slots and leaves faces, adjacency and therefore every normal's bits where they were.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_map.h"
#include "host_refit.h"

#ifndef RPT_SMOOTH_FN
#define RPT_SMOOTH_FN inline
#endif

namespace rpthost {

constexpr float kSmoothFMax = 3.40282347e+38f;

// cross(a, b) and dot(a, b) of include/rpt.h ("triangle meshes")
RPT_SMOOTH_FN void smooth_cross(const float* a, const float* b, float* out)
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
RPT_SMOOTH_FN float smooth_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The face vector of a triangle (a, b, c): g = cross(b - a, c - a), not normalised.
RPT_SMOOTH_FN void smooth_face_vector(const float* a, const float* b, const float* c, float* g)
{
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    smooth_cross(e1, e2, g);
}

// The guarded normalize both statements end with: false (and n = 0) when !(l2 > 0 && l2 <= F::MAX), l2 = dot(s, s).
RPT_SMOOTH_FN bool smooth_normalize(const float* s, float* n)
{
    const float l2 = smooth_dot(s, s);
    if (!(l2 > 0.0f && l2 <= kSmoothFMax)) { n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f; return false; }
    const float len = __builtin_sqrtf(l2);
    n[0] = s[0] / len; n[1] = s[1] / len; n[2] = s[2] / len;
    return true;
}

// The vertex vector: the face vectors of faces[first .. last) (16 B each in `face`), summed per component left to right, starting
// with the first term; no face: (0, 0, 0).  Then the guarded normalize.
RPT_SMOOTH_FN void smooth_vertex_normal(const float* face, const uint32_t* faces, uint32_t first, uint32_t last, float* n)
{
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t k = first; k < last; ++k) {
        const float* g = face + 4 * (size_t)faces[k];
        if (k == first) { s[0] = g[0]; s[1] = g[1]; s[2] = g[2]; }
        else { s[0] = s[0] + g[0]; s[1] = s[1] + g[1]; s[2] = s[2] + g[2]; }
    }
    smooth_normalize(s, n);
}

// The device's smooth tables (DevState::smooth), one allocation.
struct SmoothLayout {
    size_t off_normals = 0, off_face = 0, off_face_vertex = 0, off_adj_first = 0, off_adj = 0, off_bits = 0, total = 0;
    SmoothLayout(uint32_t n_vertices, uint32_t n_tris, uint32_t n_faces, uint32_t n_adj)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_face = round16(16 * (size_t)n_vertices);                // the normals: 16 B per vertex of the scene
        off_face_vertex = off_face + round16(16 * (size_t)n_faces);
        off_adj_first = off_face_vertex + round16(12 * (size_t)n_faces);
        off_adj = off_adj_first + round16(4 * ((size_t)n_vertices + 1));
        off_bits = off_adj + round16(4 * (size_t)n_adj);
        total = off_bits + round16(4 * (((size_t)n_tris + 31) / 32));
    }
};

// What rpt_set_mesh_shading leaves on the host for the life of the modes, and (the vectors) what every device gets.
struct SmoothPlan {
    std::vector<uint8_t> mode;                 // mesh -> RPT_MESH_SHADING_*; empty: every mesh FLAT
    uint32_t n_vertices = 0, n_tris = 0;       // of the scene
    uint32_t n_faces = 0, n_adj = 0;
    // staging: released once every device holds it
    std::vector<uint32_t> face_vertex;         // [3][n_faces]: face -> its corners a, b, c in the concatenated vertex array
    std::vector<uint32_t> adj_first;           // vertex -> its range of `adj`; n_vertices + 1 entries
    std::vector<uint32_t> adj;                 // the faces that name the vertex at one or more corners, each once, ascending
    std::vector<uint32_t> bits;                // one bit per flattened triangle: its mesh is SMOOTH

    bool any() const
    {
        for (uint8_t m : mode) if (m == RPT_MESH_SHADING_SMOOTH) return true;
        return false;
    }
    bool smooth(uint32_t mesh) const { return mesh < mode.size() && mode[mesh] == RPT_MESH_SHADING_SMOOTH; }
    void release_staging()
    {
        std::vector<uint32_t>().swap(face_vertex);
        std::vector<uint32_t>().swap(adj_first);
        std::vector<uint32_t>().swap(adj);
        std::vector<uint32_t>().swap(bits);
    }
    SmoothLayout layout() const { return SmoothLayout(n_vertices, n_tris, n_faces, n_adj); }     // of every device's tables
};

// The flattened triangles' corners, 3 per triangle, from tables in slot order: `rows` (48 B per slot, word 3 = the flattened index)
// and slot_vertex ([3][n]).  false: a row's index is out of range or named twice (the tables are not a mesh scene's).
inline bool smooth_flat_indices(const unsigned char* rows, const uint32_t* slot_vertex, size_t n, std::vector<uint32_t>& flat)
{
    flat.assign(3 * n, 0xFFFFFFFFu);
    for (size_t slot = 0; slot < n; ++slot) {
        uint32_t index;
        memcpy(&index, rows + 48 * slot + 12, 4);
        if (index >= n || flat[3 * (size_t)index] != 0xFFFFFFFFu) return false;
        for (size_t c = 0; c < 3; ++c) flat[3 * (size_t)index + c] = slot_vertex[c * n + slot];
    }
    return true;
}

// The plan of `mode` over a scene's flattened triangles (`flat`: 3 corners each, concatenated vertex indices).
inline void build_smooth_plan(const RefitPlan& plan, const uint32_t* flat, const std::vector<uint8_t>& mode, SmoothPlan& sp)
{
    sp = SmoothPlan();
    sp.mode = mode;
    sp.n_vertices = plan.n_vertices();
    sp.n_tris = plan.n_slots;
    sp.bits.assign(((size_t)sp.n_tris + 31) / 32, 0u);
    for (uint32_t m = 0; m < plan.n_meshes(); ++m)
        if (sp.smooth(m)) sp.n_faces += plan.tri_first[m + 1u] - plan.tri_first[m];
    const size_t nf = sp.n_faces;
    sp.face_vertex.resize(3 * nf);
    sp.adj_first.assign((size_t)sp.n_vertices + 1, 0u);
    size_t j = 0;
    for (uint32_t m = 0; m < plan.n_meshes(); ++m) {
        if (!sp.smooth(m)) continue;
        for (uint32_t k = plan.tri_first[m]; k < plan.tri_first[m + 1u]; ++k, ++j) {
            sp.bits[k >> 5] |= 1u << (k & 31u);
            const uint32_t a = flat[3 * (size_t)k], b = flat[3 * (size_t)k + 1], c = flat[3 * (size_t)k + 2];
            sp.face_vertex[j] = a; sp.face_vertex[nf + j] = b; sp.face_vertex[2 * nf + j] = c;
            sp.adj_first[(size_t)a + 1] += 1u;
            if (b != a) sp.adj_first[(size_t)b + 1] += 1u;
            if (c != a && c != b) sp.adj_first[(size_t)c + 1] += 1u;
        }
    }
    for (size_t v = 0; v < sp.n_vertices; ++v) sp.adj_first[v + 1] += sp.adj_first[v];
    sp.n_adj = sp.adj_first[sp.n_vertices];
    sp.adj.resize(sp.n_adj);
    std::vector<uint32_t> at(sp.adj_first.begin(), sp.adj_first.end() - 1);
    for (size_t f = 0; f < nf; ++f) {                               // ascending faces: every vertex's list comes out ascending
        const uint32_t a = sp.face_vertex[f], b = sp.face_vertex[nf + f], c = sp.face_vertex[2 * nf + f];
        sp.adj[at[a]++] = (uint32_t)f;
        if (b != a) sp.adj[at[b]++] = (uint32_t)f;
        if (c != a && c != b) sp.adj[at[c]++] = (uint32_t)f;
    }
}

// `err` = "rpt_set_mesh_shading: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int shading_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_set_mesh_shading", code, fmt, a...); }

// Every check of rpt_set_mesh_shading but the NULL context (include/rpt.h), in one fixed order.  RPT_OK: `mode` is `current` (empty:
// every mesh FLAT) with the named meshes' new modes, one entry per mesh.
inline int check_mesh_shading(const RefitPlan& plan, bool mesh_scene, const rpt_mesh_shading* items, uint32_t n_items,
                              const std::vector<uint8_t>& current, std::vector<uint8_t>& mode, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!mesh_scene) return shading_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!plan.ok) return shading_error(err, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    if (!items && n_items) return shading_error(err, INVALID, "items is NULL");
    mode = current;
    mode.resize(plan.n_meshes(), (uint8_t)RPT_MESH_SHADING_FLAT);
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const rpt_mesh_shading& it = items[i];
        if (it.mesh >= plan.n_meshes()) return shading_error(err, INVALID, "item %u: mesh %u out of range (the scene has %u)", i, it.mesh, plan.n_meshes());
        if (named[it.mesh]) return shading_error(err, INVALID, "item %u: mesh %u is named twice", i, it.mesh);
        named[it.mesh] = 1;
        if (it.mode != RPT_MESH_SHADING_FLAT && it.mode != RPT_MESH_SHADING_SMOOTH)
            return shading_error(err, INVALID, "item %u: mode %u of mesh %u is neither RPT_MESH_SHADING_FLAT nor RPT_MESH_SHADING_SMOOTH", i, it.mode, it.mesh);
        mode[it.mesh] = (uint8_t)it.mode;
    }
    return RPT_OK;
}

// ---- the host reference: what k_smooth.hip's two passes compute, statement for statement ------------------------------------------
// `face`: 4 floats per face of scratch; `normals`: 4 floats per vertex of the scene (the fourth is 0), as the device stores them.
inline void smooth_normals_reference(const float* vertices, const SmoothPlan& sp, float* face, float* normals)
{
    const size_t nf = sp.n_faces;
    for (size_t f = 0; f < nf; ++f) {
        float* g = face + 4 * f;
        smooth_face_vector(vertices + 3 * (size_t)sp.face_vertex[f], vertices + 3 * (size_t)sp.face_vertex[nf + f],
                           vertices + 3 * (size_t)sp.face_vertex[2 * nf + f], g);
        g[3] = 0.0f;
    }
    for (size_t v = 0; v < sp.n_vertices; ++v) {
        float* n = normals + 4 * v;
        smooth_vertex_normal(face, sp.adj.data(), sp.adj_first[v], sp.adj_first[v + 1], n);
        n[3] = 0.0f;
    }
}

// The normal of a winning triangle of a SMOOTH mesh (include/rpt.h): u and v as the triangle test computes them for the ray (o, d)
// and the row (a, e1 = b - a, e2 = c - a), the interpolation of the corners' normals, and the fall-back to the flat normal
// normalize(cross(e1, e2)) — the reference's normalize: the root of dot, three divides, no guard.
inline void smooth_hit_normal_reference(const float* o, const float* d, const float* a, const float* e1, const float* e2,
                                        const float* na, const float* nb, const float* nc, float* out)
{
    float p[3], q[3];
    smooth_cross(d, e2, p);
    const float det = smooth_dot(e1, p);
    const float inv = 1.0f / det;
    const float s[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    const float u = smooth_dot(s, p) * inv;
    smooth_cross(s, e1, q);
    const float v = smooth_dot(d, q) * inv;
    const float w = (1.0f - u) - v;
    float m[3];
    for (int i = 0; i < 3; ++i) m[i] = (w * na[i] + u * nb[i]) + v * nc[i];
    if (smooth_normalize(m, out)) return;
    float g[3];
    smooth_cross(e1, e2, g);
    const float len = __builtin_sqrtf(smooth_dot(g, g));
    out[0] = g[0] / len; out[1] = g[1] / len; out[2] = g[2] / len;
}

}  // namespace rpthost
