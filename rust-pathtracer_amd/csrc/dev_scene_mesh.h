// dev_scene_mesh.h — scene queries of mesh scenes (include/rpt.h, "triangle meshes"): a large scene (dev_scene_large.h: spheres in
// HBM, grid or brute force, up to 4 planes, the lights, full sphere materials) plus triangles under a bounding volume hierarchy built
// on the host (host_bvh.h).
//
// Exactness.  The ordered loop of include/rpt.h accepts a triangle when t < dist, so it ends with the triangle of least t below the
// distance the spheres and planes left, the lowest flattened index on ties — an answer that does not depend on the order the
// triangles are tested in, as long as every triangle that can still win is tested: the walk below accepts t < best || (t == best &&
// index < best index) (best index 0 while no triangle is accepted: a tie with a sphere or plane loses, as in the loop), and culls a
// box only when the ray provably does not reach it at t <= best (`<=`: a box holding a tie is still opened).  "Provably": the triangle
// test of include/rpt.h ends with the point check — the f32 point p = o + t*d lies within w = 2^-16 (max(|lo|, |hi|) + |o|) of the
// triangle's box, per axis — so the exact point P = o + t d of an accepted hit lies within w + |p - P| of it, and |p - P| <=
// 2^-22 (|p| + |o|).  A node's box contains its triangles' boxes (host_bvh.h), and box_enter widens it per axis by
// W = 2^-14 (max(|lo|, |hi|) + |o|) > w + |p - P| (rounding of the widened bounds included): P lies in the widened box, so the exact
// slab interval [T0, T1] holds t.  The computed slab bounds carry a relative error below 2^-21 (the subtraction, the 1-ulp
// reciprocal, the product), and the interval is widened by 2^-14 relative on both ends: the computed entry is <= T0 <= t <= best and
// the computed exit >= T1 >= the entry, so the box is opened.  The argument needs finite slab bounds: rays with an infinite component,
// a direction component non-zero but below 2^-60, or an origin coordinate beyond 2^60, and scenes with a vertex coordinate beyond
// 2^60 (capi.hip: use_bvh 0), take the ordered loop; a ray with a NaN component misses everything (its det or u is NaN) and ends at
// once.  tests/test_gpu_mesh.py holds the walk to a numpy float32 restatement of the loop bit for bit, rays in a triangle's plane
// included.
//
// The stack.  A 256-lane workgroup's walks keep their stacks in LDS: kMeshStack words per lane, lane-interleaved (entry k of lane l at
// word k * 256 + l: no bank conflicts), 24 KiB per workgroup.  No leaf lies deeper than kMeshStack below the root (host_bvh.h,
// kBvhMaxDepth) and the walk pushes at most one entry per level, so the stack cannot overflow.
#ifndef RPT_NS                        // (the namespace of this pass: dev_math.h, "two passes")
#define RPT_NS rptdev
#endif
#if (defined(RPT_PLAIN_PASS) && !defined(RPT_DEV_SCENE_MESH_H_PLAIN)) || (!defined(RPT_PLAIN_PASS) && !defined(RPT_DEV_SCENE_MESH_H_NORMAL))
#ifdef RPT_PLAIN_PASS
#define RPT_DEV_SCENE_MESH_H_PLAIN
#else
#define RPT_DEV_SCENE_MESH_H_NORMAL
#endif

#include "dev_scene_large.h"

namespace RPT_NS {
using namespace rptscene;

constexpr uint32_t kMeshStack = 24;                 // == host_bvh.h kBvhMaxDepth
constexpr uint32_t kMeshLanes = 256;                // workgroup size of every kernel that walks the hierarchy
constexpr uint32_t kMeshLeaf = 0x80000000u;         // host_bvh.h: kBvhLeaf, kBvhCountShift, kBvhSlotMask
constexpr uint32_t kMeshCountShift = 27;
constexpr uint32_t kMeshSlotMask = (1u << 27) - 1u;
constexpr uint32_t kNoTriangle = 0xFFFFFFFFu;

RPT_DEV uint32_t* mesh_lane_stack()
{
    __shared__ uint32_t s_mesh_stack[kMeshStack * kMeshLanes];
    return s_mesh_stack + threadIdx.x;
}

// include/rpt.h, "triangle test": two-sided Moller-Trumbore in the header's operation order (dot3 / cross3 are fx.rs's, fdiv the
// correctly rounded divide).  e1 = b - a and e2 = c - a come from the table, computed by the host in f32: the same numbers.
// min / max of finite numbers (the point check and the widened boxes see no NaN)
RPT_DEV float mesh_min(float a, float b) { return a < b ? a : b; }
RPT_DEV float mesh_max(float a, float b) { return a < b ? b : a; }

// The point check (include/rpt.h) of one axis: p = o + t*d within w = 2^-16 (max(|lo|, |hi|) + |o|) of [lo, hi] = a + [min(0, e1, e2),
// max(0, e1, e2)].
RPT_DEV bool tri_point_in(float o, float d, float t, float a, float e1, float e2)
{
    const float lo = a + mesh_min(mesh_min(0.0f, e1), e2);
    const float hi = a + mesh_max(mesh_max(0.0f, e1), e2);
    const float w = (mesh_max(__builtin_fabsf(lo), __builtin_fabsf(hi)) + __builtin_fabsf(o)) * 0x1p-16f;
    const float p = o + t * d;
    return lo - w <= p && p <= hi + w;
}

RPT_DEV bool hit_triangle(const RayD& ray, v3 a, v3 e1, v3 e2, float& t)
{
    const v3 p = cross3(ray.d, e2);
    const float det = dot3(e1, p);
    if (!(det < 0.0f || det > 0.0f)) return false;
    const float inv = fdiv(1.0f, det);
    const v3 s = ray.o - a;
    const float u = dot3(s, p) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    const v3 q = cross3(s, e1);
    const float v = dot3(ray.d, q) * inv;
    if (!(v >= 0.0f && u + v <= 1.0f)) return false;
    const float tt = dot3(e2, q) * inv;
    if (!(tt >= 0.0f && tt < 3.40282347e+38f)) return false;
    if (!(tri_point_in(ray.o.x, ray.d.x, tt, a.x, e1.x, e2.x) && tri_point_in(ray.o.y, ray.d.y, tt, a.y, e1.y, e2.y) &&
          tri_point_in(ray.o.z, ray.d.z, tt, a.z, e1.z, e2.z))) return false;
    t = tt;
    return true;
}

struct TriRec {
    v3 a, e1, e2;
    uint32_t index, material;
};

RPT_DEV TriRec tri_at(const SceneMesh& sc, uint32_t slot)
{
    const float4 r0 = gather32(sc.tris, 3u * slot), r1 = gather32(sc.tris, 3u * slot + 1u), r2 = gather32(sc.tris, 3u * slot + 2u);
    TriRec r;
    r.a = mk3(r0.x, r0.y, r0.z); r.e1 = mk3(r1.x, r1.y, r1.z); r.e2 = mk3(r2.x, r2.y, r2.z);
    r.index = rpt_f2u(r0.w);
    r.material = rpt_f2u(r2.w);
    return r;
}

// What a walk precomputes of its ray.
struct MeshRay {
    float o[3], inv[3];
    bool flat[3];
};

// A ray with a NaN component hits no triangle: det or u is NaN (include/rpt.h).
RPT_DEV bool mesh_ray_nan(const RayD& ray)
{
    return !(ray.o.x == ray.o.x && ray.o.y == ray.o.y && ray.o.z == ray.o.z && ray.d.x == ray.d.x && ray.d.y == ray.d.y && ray.d.z == ray.d.z);
}

// Can the slab arithmetic serve this ray exactly (see the head of this file)?
RPT_DEV bool mesh_ray_usable(const RayD& ray, MeshRay& mr)
{
    const float o[3] = {ray.o.x, ray.o.y, ray.o.z}, d[3] = {ray.d.x, ray.d.y, ray.d.z};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ad = __builtin_fabsf(d[a]);
        mr.o[a] = o[a];
        mr.flat[a] = d[a] == 0.0f;
        mr.inv[a] = __builtin_amdgcn_rcpf(mr.flat[a] ? 1.0f : d[a]);
        ok = ok && (__builtin_fabsf(o[a]) <= 0x1p60f) && (mr.flat[a] || (ad >= 0x1p-60f && ad <= 3.40282347e+38f));
    }
    return ok;
}

// The slab test of one box {lo xyz, hi xyz}, widened: true when the ray may reach the box at some t in [0, limit]; `tn` its entry.
// (An empty box, lo = +inf > hi = -inf, is entered by rays with no zero direction component: the empty child it stands for holds no
// triangle, so that costs one pop.)
RPT_DEV bool box_enter(const MeshRay& mr, const float* bx, float limit, float& tn)
{
    float t0 = 0.0f, t1 = 3.40282347e+38f;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float wa = (mesh_max(__builtin_fabsf(bx[a]), __builtin_fabsf(bx[3 + a])) + __builtin_fabsf(mr.o[a])) * 0x1p-14f;
        const float blo = bx[a] - wa, bhi = bx[3 + a] + wa;         // (the head of this file: W)
        const float ta = (blo - mr.o[a]) * mr.inv[a];
        const float tb = (bhi - mr.o[a]) * mr.inv[a];
        const float lo = ta < tb ? ta : tb;
        const float hi = ta < tb ? tb : ta;
        t0 = (!mr.flat[a] && lo > t0) ? lo : t0;
        t1 = (!mr.flat[a] && hi < t1) ? hi : t1;
        ok = ok && (!mr.flat[a] || (mr.o[a] >= blo && mr.o[a] <= bhi));
    }
    tn = t0 * (1.0f - 0x1p-14f);
    t1 = t1 * (1.0f + 0x1p-14f);
    return ok && tn <= t1 && tn <= limit;
}

struct MeshNode {
    float lbox[6], rbox[6];
    uint32_t child[2];
};

RPT_DEV MeshNode node_at(const SceneMesh& sc, uint32_t i)
{
    const float4 r0 = gather32(sc.nodes, 4u * i), r1 = gather32(sc.nodes, 4u * i + 1u), r2 = gather32(sc.nodes, 4u * i + 2u);
    const float4 r3 = gather32(sc.nodes, 4u * i + 3u);
    MeshNode n;
    n.lbox[0] = r0.x; n.lbox[1] = r0.y; n.lbox[2] = r0.z; n.lbox[3] = r0.w; n.lbox[4] = r1.x; n.lbox[5] = r1.y;
    n.rbox[0] = r1.z; n.rbox[1] = r1.w; n.rbox[2] = r2.x; n.rbox[3] = r2.y; n.rbox[4] = r2.z; n.rbox[5] = r2.w;
    n.child[0] = rpt_f2u(r3.x); n.child[1] = rpt_f2u(r3.y);
    return n;
}

// One candidate of the closest walk: accepted by the rule in the head of this file.
RPT_DEV void mesh_test_slot(const SceneMesh& sc, const RayD& ray, uint32_t slot, float& best_t, uint32_t& best_index, uint32_t& best_slot)
{
    const TriRec r = tri_at(sc, slot);
    float t;
    if (hit_triangle(ray, r.a, r.e1, r.e2, t) && (t < best_t || (t == best_t && r.index < best_index))) {
        best_t = t; best_index = r.index; best_slot = slot;
    }
}

// The nearest triangle nearer than `dist` (in-out): its slot, or kNoTriangle.  The ordered loop's answer (see the head of this file).
RPT_DEV uint32_t mesh_closest(const SceneMesh& sc, const RayD& ray, float& dist)
{
    float best_t = dist;
    uint32_t best_index = 0u, best_slot = kNoTriangle;
    MeshRay mr;
    if (mesh_ray_nan(ray)) return kNoTriangle;
    if (!sc.use_bvh || !mesh_ray_usable(ray, mr)) {
        for (uint32_t k = 0; k < sc.n_tris; ++k) mesh_test_slot(sc, ray, k, best_t, best_index, best_slot);
    } else {
        uint32_t* stk = mesh_lane_stack();
        uint32_t sp = 0;
        uint32_t cur = 0;                                           // the root: an interior node
        for (;;) {
            if (!(cur & kMeshLeaf)) {
                const MeshNode n = node_at(sc, cur);
                float tl, tr;
                const bool hl = box_enter(mr, n.lbox, best_t, tl);
                const bool hr = box_enter(mr, n.rbox, best_t, tr);
                if (hl && hr) {
                    const bool left_first = tl <= tr;
                    stk[sp * kMeshLanes] = left_first ? n.child[1] : n.child[0];
                    sp += 1u;
                    cur = left_first ? n.child[0] : n.child[1];
                    continue;
                }
                if (hl || hr) { cur = hl ? n.child[0] : n.child[1]; continue; }
            } else {
                const uint32_t first = cur & kMeshSlotMask, count = (cur >> kMeshCountShift) & 15u;
                for (uint32_t k = 0; k < count; ++k) mesh_test_slot(sc, ray, first + k, best_t, best_index, best_slot);
            }
            if (sp == 0u) break;
            sp -= 1u;
            cur = stk[sp * kMeshLanes];
        }
    }
    if (best_slot != kNoTriangle) dist = best_t;
    return best_slot;
}

// Any triangle hit with (!use_max || t < max_dist): include/rpt.h, any_hit.
RPT_DEV bool mesh_any(const SceneMesh& sc, const RayD& ray, bool use_max, float max_dist)
{
    MeshRay mr;
    if (mesh_ray_nan(ray)) return false;
    if (!sc.use_bvh || !mesh_ray_usable(ray, mr)) {
        for (uint32_t k = 0; k < sc.n_tris; ++k) {
            const TriRec r = tri_at(sc, k);
            float t;
            if (hit_triangle(ray, r.a, r.e1, r.e2, t) && (!use_max || t < max_dist)) return true;
        }
        return false;
    }
    const float limit = use_max ? max_dist : 3.40282347e+38f;
    uint32_t* stk = mesh_lane_stack();
    uint32_t sp = 0;
    uint32_t cur = 0;
    for (;;) {
        if (!(cur & kMeshLeaf)) {
            const MeshNode n = node_at(sc, cur);
            float tl, tr;
            const bool hl = box_enter(mr, n.lbox, limit, tl);
            const bool hr = box_enter(mr, n.rbox, limit, tr);
            if (hl && hr) {
                stk[sp * kMeshLanes] = n.child[1];
                sp += 1u;
                cur = n.child[0];
                continue;
            }
            if (hl || hr) { cur = hl ? n.child[0] : n.child[1]; continue; }
        } else {
            const uint32_t first = cur & kMeshSlotMask, count = (cur >> kMeshCountShift) & 15u;
            for (uint32_t k = 0; k < count; ++k) {
                const TriRec r = tri_at(sc, first + k);
                float t;
                if (hit_triangle(ray, r.a, r.e1, r.e2, t) && (!use_max || t < max_dist)) return true;
            }
        }
        if (sp == 0u) break;
        sp -= 1u;
        cur = stk[sp * kMeshLanes];
    }
    return false;
}

// GeomHit.code of a mesh scene: the large scenes' layout (nearest sphere in the low 28 bits, accepted planes above), where a WINNING
// triangle is n_spheres + its slot in the low 28 bits and no plane: its full patch overwrites every field the spheres and planes
// accepted before it wrote (rpt_upload_scene refuses n_spheres + triangles >= kNoSphere).
RPT_DEV uint32_t mesh_slot_of(const SceneMesh& sc, uint32_t code)
{
    const uint32_t best = code & kNoSphere;
    return (best != kNoSphere && best >= sc.n_spheres) ? best - sc.n_spheres : kNoTriangle;
}

// AnalyticalScene::closest_hit with the triangles after the planes, then Scene::sample_lights (include/rpt.h, "triangle meshes").
RPT_DEV bool closest_geom(const SceneMesh& sc, const RayD& ray, PathState& ps, GeomHit& g, EmitterHit& e)
{
    float dist = 3.40282347e+38f;
    bool hit = false;
    uint32_t best = 0xFFFFFFFFu;                                    // nearest sphere so far
    if (sc.use_accel) grid_closest_sphere(sc, ray, dist, best, hit);
    else brute_closest_sphere(sc, ray, dist, best, hit);
    uint32_t accepted_planes = 0;
    for (uint32_t k = 0; k < sc.n_planes; ++k) {                    // as closest_geom_finish
        const DevPlane& p = sc.planes[k];
        float t;
        bool h = hit_plane(ray, p, t);
        bool acc = h && ((sc.n_spheres == 0 && k == 0) || t < dist);
        if (acc) {
            dist = t;
            hit = true;
            accepted_planes |= 1u << k;
        }
    }
    uint32_t code = (best == 0xFFFFFFFFu ? kNoSphere : best) | (accepted_planes << 28);
    const uint32_t slot = mesh_closest(sc, ray, dist);
    if (slot != kNoTriangle) { hit = true; code = sc.n_spheres + slot; }
    if (hit) ps.hit_dist = dist;
    g.code = code;
    return sample_lights_large(sc, ray, ps, e, hit);
}

RPT_DEV v3 hit_normal(const SceneMesh& sc, const RayD& ray, float dist, const GeomHit& g)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return normal_large(sc, ray, dist, g);
    const TriRec r = tri_at(sc, slot);
    return norm3(cross3(r.e1, r.e2));
}

// The winning triangle's full patch over Material::new(); otherwise the large scenes' layering.
RPT_DEV void hit_material(const SceneMesh& sc, const RayD& ray, const GeomHit& g, Mat& mat)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) { material_large(sc, ray, g.code, mat); return; }
    mat_defaults(mat);
    const DevMaterial m = gather32(sc.materials, tri_at(sc, slot).material);
    mat.rgb = mk3(m.rgb[0], m.rgb[1], m.rgb[2]);
    mat.emission = mk3(m.emission[0], m.emission[1], m.emission[2]);
    mat.anisotropic = m.anisotropic; mat.metallic = m.metallic; mat.roughness = m.roughness;
    mat.subsurface = m.subsurface; mat.specular_tint = m.specular_tint; mat.sheen = m.sheen;
    mat.sheen_tint = m.sheen_tint; mat.clearcoat = m.clearcoat; mat.clearcoat_gloss = m.clearcoat_gloss;
    mat.spec_trans = m.spec_trans; mat.ior = m.ior;
}

RPT_DEV v3 hit_emission(const SceneMesh& sc, const GeomHit& g)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return hit_emission(static_cast<const SceneLarge&>(sc), g);
    const DevMaterial m = gather32(sc.materials, tri_at(sc, slot).material);
    return mk3(m.emission[0], m.emission[1], m.emission[2]);
}

RPT_DEV bool any_hit(const SceneMesh& sc, const RayD& ray, float max_dist)
{
    const bool use_max = (sc.flags & RPT_SCENE_ANYHIT_USES_MAX_DIST) != 0;
    bool occluded = sc.use_accel ? grid_any_sphere(sc, ray, use_max, max_dist) : brute_any_sphere(sc, ray, use_max, max_dist);
    for (uint32_t k = 0; k < sc.n_planes; ++k) {
        float t;
        bool h = hit_plane(ray, sc.planes[k], t);
        occluded = occluded || (h && (!use_max || t < max_dist));
    }
    if (!occluded) occluded = mesh_any(sc, ray, use_max, max_dist);
    return occluded;
}

}  // namespace RPT_NS
#endif  // this pass
