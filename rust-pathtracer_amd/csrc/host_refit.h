// host_refit.h — the host half of rpt_update_meshes (include/rpt.h, "moving meshes"): what a refit of a mesh scene's hierarchy needs
// beyond the scene's own tables, the checks of an update, and a host reference of the refit itself.  Plain C++ with no HIP type in it,
// like host_bvh.h: host_upload.h includes it (prepare_scene fills a RefitPlan), capi.hip copies the plan to every device at the
// context's first update, and tests/refit_harness.cpp runs this file under the address and undefined-behaviour sanitizers
// (tests/test_mesh_update_host.py).
//
// A refit keeps the hierarchy's shape — the child words, the leaves' slot ranges, the order of the triangle table — and recomputes,
// from new vertex positions, the float part of every triangle row and every box.  host_bvh.h stores in a node the EXACT box of its
// triangles' boxes (min / max only), and the union of the children's boxes is that same box, so a refit gives the boxes a fresh
// build would store for the same shape; the walk (dev_scene_mesh.h) returns the ordered loop's answer for any hierarchy whose boxes
// contain their triangles' boxes, so the frame is the frame of a fresh upload whatever shape that would have chosen.
// (One footnote on "the same bytes": where a box's bound is zero and zeros of both signs reach it, the sign a build stores depends
// on the order its partitions left, and a refit's on the slot order.  -0 == +0 in every comparison of the walk: no result depends on it.)
//
// Interior nodes are stored in pre-order (a node's index is below its children's), so one pass gives every node's depth; the refit
// order is the node ids sorted by depth with one offset per level — at most kBvhMaxDepth levels — processed deepest first.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_bvh.h"
#include "host_map.h"

namespace rpthost {

struct RefitPlan {
    bool ok = false;                           // a mesh scene whose meshes hold fewer than 2^32 vertices in all
    uint32_t n_slots = 0, n_nodes = 0;
    // kept for the life of the scene
    std::vector<uint32_t> mesh_first;          // mesh -> its first vertex in the concatenated vertex array; n_meshes + 1 entries
    std::vector<uint32_t> tri_first;           // mesh -> its first triangle in the flattened list; n_meshes + 1 entries (host_smooth.h)
    std::vector<uint32_t> mesh_material;       // mesh -> rpt_mesh.material (host_light.h: a mesh light's emission)
    std::vector<uint8_t> referenced;           // concatenated vertex -> some triangle uses it (upload's 2^60 rule looks at those only)
    std::vector<float> mesh_max_abs;           // mesh -> the largest |coordinate| of its referenced vertices (0: none)
    std::vector<uint32_t> level_first;         // depth -> offset into level_nodes; n_levels + 1 entries
    // what every device gets at the context's first update; released once they all hold it (capi.hip, ensure_refit)
    std::vector<float> vertices;               // xyz, all meshes concatenated
    std::vector<uint32_t> slot_vertex;         // [3][n_slots]: slot -> its three indices into `vertices` (one array per corner: coalesced)
    std::vector<uint32_t> level_nodes;         // interior node ids sorted by depth

    uint32_t n_meshes() const { return mesh_first.empty() ? 0u : (uint32_t)mesh_first.size() - 1u; }
    uint32_t n_levels() const { return level_first.empty() ? 0u : (uint32_t)level_first.size() - 1u; }
    uint32_t n_vertices() const { return mesh_first.empty() ? 0u : mesh_first.back(); }
    void release_staging()
    {
        std::vector<float>().swap(vertices);
        std::vector<uint32_t>().swap(slot_vertex);
        std::vector<uint32_t>().swap(level_nodes);
    }
};

// The device's refit tables (DevState::refit), one allocation: vertices, slot_vertex, the slots' boxes (24 B each, scratch), level_nodes.
struct RefitLayout {
    size_t off_vertices = 0, off_slot_vertex = 0, off_slot_box = 0, off_level_nodes = 0, total = 0;
    RefitLayout(uint32_t n_vertices, uint32_t n_slots, uint32_t n_nodes)
    {
        const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        off_slot_vertex = round16(12 * (size_t)n_vertices);
        off_slot_box = off_slot_vertex + round16(12 * (size_t)n_slots);
        off_level_nodes = off_slot_box + round16(24 * (size_t)n_slots);
        total = off_level_nodes + round16(4 * (size_t)n_nodes);
    }
};

// The refit order of a hierarchy: level_first / level_nodes of `plan` (depth 0 is the root).
inline void refit_levels(const BvhNode* nodes, uint32_t n_nodes, RefitPlan& plan)
{
    std::vector<uint32_t> depth(n_nodes, 0u);
    uint32_t deepest = 0;
    for (uint32_t i = 0; i < n_nodes; ++i)
        for (int c = 0; c < 2; ++c) {
            const uint32_t ch = nodes[i].child[c];
            if (ch & kBvhLeaf) continue;
            depth[ch] = depth[i] + 1u;                              // (pre-order: ch > i, so depth[i] is final)
            deepest = std::max(deepest, depth[ch]);
        }
    plan.level_first.assign(n_nodes ? deepest + 2u : 0u, 0u);
    for (uint32_t i = 0; i < n_nodes; ++i) plan.level_first[depth[i] + 1u] += 1u;
    for (size_t k = 1; k < plan.level_first.size(); ++k) plan.level_first[k] += plan.level_first[k - 1];
    plan.level_nodes.resize(n_nodes);
    std::vector<uint32_t> at(plan.level_first.begin(), plan.level_first.end());
    for (uint32_t i = 0; i < n_nodes; ++i) plan.level_nodes[at[depth[i]]++] = i;
}

// The plan of a checked mesh scene (prepare_scene): `s`'s meshes hold at least one triangle, `bvh` is the hierarchy over them.
inline void build_refit_plan(const rpt_scene_desc* s, const HostBvh& bvh, RefitPlan& plan)
{
    plan = RefitPlan();
    uint64_t n_vertices = 0, n_tris = 0;
    for (uint32_t m = 0; m < s->n_meshes; ++m) { n_vertices += s->meshes[m].n_vertices; n_tris += s->meshes[m].n_triangles; }
    if (n_vertices > 0xFFFFFFFFull) return;                         // (48 GiB of vertices: rpt_update_meshes answers RPT_ERR_UNSUPPORTED)
    plan.ok = true;
    plan.n_slots = (uint32_t)n_tris;
    plan.n_nodes = (uint32_t)bvh.nodes.size();
    plan.mesh_first.assign(s->n_meshes + 1u, 0u);
    plan.tri_first.assign(s->n_meshes + 1u, 0u);
    plan.mesh_material.assign(s->n_meshes, 0u);
    plan.vertices.resize(3 * (size_t)n_vertices);
    plan.referenced.assign((size_t)n_vertices, 0);
    plan.mesh_max_abs.assign(s->n_meshes, 0.0f);
    std::vector<uint32_t> flat(3 * (size_t)n_tris);                 // flattened triangle -> its three concatenated vertex indices
    size_t k = 0;
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const rpt_mesh& me = s->meshes[m];
        const uint32_t first = plan.mesh_first[m];
        plan.mesh_first[m + 1u] = first + me.n_vertices;
        plan.tri_first[m + 1u] = plan.tri_first[m] + me.n_triangles;
        plan.mesh_material[m] = me.material;
        if (me.n_vertices) memcpy(&plan.vertices[3 * (size_t)first], me.vertices, 12 * (size_t)me.n_vertices);
        for (size_t i = 0; i < 3 * (size_t)me.n_triangles; ++i, ++k) {
            flat[k] = first + me.indices[i];
            plan.referenced[flat[k]] = 1;
        }
        float big = 0.0f;
        for (uint32_t v = 0; v < me.n_vertices; ++v)
            if (plan.referenced[first + v])
                for (int a = 0; a < 3; ++a) big = std::max(big, std::fabs(me.vertices[3 * (size_t)v + a]));
        plan.mesh_max_abs[m] = big;
    }
    const size_t n = plan.n_slots;
    plan.slot_vertex.resize(3 * n);
    for (size_t slot = 0; slot < n; ++slot)
        for (size_t c = 0; c < 3; ++c) plan.slot_vertex[c * n + slot] = flat[3 * (size_t)bvh.order[slot] + c];
    refit_levels(bvh.nodes.data(), plan.n_nodes, plan);
}

// upload's rule (host_upload.h, use_bvh): the walk serves the scene while no coordinate a triangle uses lies beyond 2^60
inline bool refit_use_bvh(const std::vector<float>& mesh_max_abs)
{
    for (float x : mesh_max_abs) if (!(x <= 0x1p60f)) return false;
    return true;
}

// `err` = "rpt_update_meshes: " + the message; returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int update_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_update_meshes", code, fmt, a...); }

// Every check of rpt_update_meshes but the NULL context (include/rpt.h), in one fixed order: an update with several faults always
// answers the first.  `mesh_scene`: the context holds a scene with triangles, and `plan` is its plan.  RPT_OK: `max_abs` is
// plan.mesh_max_abs with the named meshes' new values.  n_updates > 0.
inline int check_mesh_update(const RefitPlan& plan, bool mesh_scene, const rpt_mesh_vertices* updates, uint32_t n_updates,
                             std::vector<float>& max_abs, std::string& err)
{
    const int INVALID = RPT_ERR_INVALID_ARG;
    if (!updates) return update_error(err, INVALID, "updates is NULL");
    if (!mesh_scene) return update_error(err, RPT_ERR_NO_SCENE, "needs an uploaded scene with meshes");
    if (!plan.ok) return update_error(err, RPT_ERR_UNSUPPORTED, "the scene's meshes hold 2^32 vertices or more");
    std::vector<uint8_t> named(plan.n_meshes(), 0);
    max_abs = plan.mesh_max_abs;
    for (uint32_t u = 0; u < n_updates; ++u) {
        const rpt_mesh_vertices& up = updates[u];
        if (up.mesh >= plan.n_meshes()) return update_error(err, INVALID, "update %u: mesh %u out of range (the scene has %u)", u, up.mesh, plan.n_meshes());
        if (named[up.mesh]) return update_error(err, INVALID, "update %u: mesh %u is named twice", u, up.mesh);
        named[up.mesh] = 1;
        const uint32_t first = plan.mesh_first[up.mesh], count = plan.mesh_first[up.mesh + 1u] - first;
        if (up.n_vertices != count) return update_error(err, INVALID, "mesh %u: n_vertices %u != the uploaded mesh's %u", up.mesh, up.n_vertices, count);
        if (count && !up.vertices) return update_error(err, INVALID, "mesh %u: vertices is NULL", up.mesh);
        float big = 0.0f;
        for (uint32_t v = 0; v < count; ++v)
            for (int a = 0; a < 3; ++a) {
                const float x = up.vertices[3 * (size_t)v + a];
                if (!std::isfinite(x)) return update_error(err, INVALID, "mesh %u vertex %u is not finite", up.mesh, v);
                if (plan.referenced[first + v]) big = std::max(big, std::fabs(x));
            }
        max_abs[up.mesh] = big;
    }
    return RPT_OK;
}

// ---- the refit on the host: what k_refit.hip's two kernels compute, statement for statement ---------------------------------------
// Step 1 (refit_triangles_kernel), one slot: the float part of its 48-byte row {a, .}, {b - a, .}, {c - a, .} — the .w words (flattened
// index, unused, material) stay — and its box.  The box is host_bvh.h's triangle_box: the union of the three VERTICES and of
// a + min(0, e1, e2) / a + max(0, e1, e2) in f32; a + e1 is not always b, so the row alone does not give it.
inline void refit_slot(const float* vertices, const uint32_t* slot_vertex, size_t n_slots, size_t slot, unsigned char* row, float* box)
{
    float v[9];
    for (size_t c = 0; c < 3; ++c) memcpy(&v[3 * c], &vertices[3 * (size_t)slot_vertex[c * n_slots + slot]], 12);
    const float r[9] = {v[0], v[1], v[2], v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    for (size_t c = 0; c < 3; ++c) memcpy(row + 16 * c, &r[3 * c], 12);
    const bvh_detail::Box x = bvh_detail::triangle_box(v);
    bvh_detail::pad_box(x, box);
}

// Step 2 (refit_nodes_kernel), one interior node: each child's box — a leaf's from its slots' boxes in slot order (an empty child
// keeps lo = +inf, hi = -inf), an interior child's from that node's two boxes (left, then right), which a deeper level wrote.
inline void refit_node(BvhNode* nodes, const float* slot_box, uint32_t node)
{
    using bvh_detail::Box;
    for (int c = 0; c < 2; ++c) {
        const uint32_t ch = nodes[node].child[c];
        Box x, y;
        x.empty();
        if (ch & kBvhLeaf) {
            const uint32_t cnt = (ch >> kBvhCountShift) & 15u, first = ch & kBvhSlotMask;
            for (uint32_t s = first; s < first + cnt; ++s) {
                memcpy(y.lo, &slot_box[6 * (size_t)s], 12); memcpy(y.hi, &slot_box[6 * (size_t)s + 3], 12);
                x.grow(y);
            }
        } else {
            memcpy(y.lo, nodes[ch].lbox, 12); memcpy(y.hi, nodes[ch].lbox + 3, 12);
            x.grow(y);
            memcpy(y.lo, nodes[ch].rbox, 12); memcpy(y.hi, nodes[ch].rbox + 3, 12);
            x.grow(y);
        }
        bvh_detail::pad_box(x, c ? nodes[node].rbox : nodes[node].lbox);
    }
}

// The whole refit over host copies of the two tables: `rows` (48 B per slot) and `nodes`, for the topology they hold, the plan's
// slot_vertex / level order and `vertices` (the concatenated array).  `slot_box`: 6 floats per slot of scratch.
inline void refit_reference(const float* vertices, const uint32_t* slot_vertex, uint32_t n_slots, const uint32_t* level_nodes,
                            const uint32_t* level_first, uint32_t n_levels, unsigned char* rows, BvhNode* nodes, float* slot_box)
{
    for (size_t slot = 0; slot < n_slots; ++slot) refit_slot(vertices, slot_vertex, n_slots, slot, rows + 48 * slot, slot_box + 6 * slot);
    for (uint32_t level = n_levels; level-- > 0;)
        for (uint32_t k = level_first[level]; k < level_first[level + 1u]; ++k) refit_node(nodes, slot_box, level_nodes[k]);
}

}  // namespace rpthost
