// dev_mesh_cut.h — mesh cutouts on the device (include/rpt.h, "mesh cutouts"): the triangle test with its last line, the cut test,
// and the two walks of dev_scene_mesh.h restated with that test behind their distance compare; closest_geom and any_hit of
// SceneMeshCutT call them.  dev_integrator.h reaches both by overload resolution alone: the other scene classes' kernels contain none
// of this, and dev_scene_mesh.h is what it was (its walks are restated here rather than turned into templates, so that the existing
// code objects are built from unchanged text).  Included after dev_mesh_env.h and launch_cut.h, before regen_body.h.
//
// Exactness.  The cut test is one more rejection in the per-triangle test, a function of (ray, triangle) alone.  The walks below
// accept and cull exactly as dev_scene_mesh.h's do — the argument at the head of that file never uses that an accepted candidate is
// accepted, only that a triangle that CAN be accepted lies in a box that is opened — so they return the ordered loop's answer over
// the triangles that pass the test.  The cut test is applied only to a candidate that the distance compare would accept: rejecting
// one that would not have been accepted changes nothing, and it saves its loads.
#pragma once

namespace rptdev {

template <class Base> struct MeshLights<SceneMeshCutT<Base>> { static constexpr bool value = true; };
template <> struct MeshEnv<SceneMeshCutEnv> { static constexpr bool value = true; };

// hit_triangle (dev_scene_mesh.h) returning its own u and v: the same operations on the same words.
RPT_DEV bool hit_triangle_uv(const RayD& ray, v3 a, v3 e1, v3 e2, float& t, float& u_out, float& v_out)
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
    t = tt; u_out = u; v_out = v;
    return true;
}

// The cut test of the triangle in `slot` with flattened index `index`, at the triangle test's u and v: false where the mask has a
// hole.  One gather of tri_tex, one 16 B descriptor; for a cutout mesh three slot_vertex words, three UVs and one mask word more.
template <class S> RPT_DEV bool cut_passes(const S& sc, uint32_t slot, uint32_t index, float u, float v)
{
    const uint32_t ord = sc.tri_tex[index];
    if (ord == rpthost::kTexNone) return true;
    const rpthost::CutDesc d = sc.cut_desc[ord];
    if (d.flags == 0u) return true;
    const float* ta = sc.uvs + 2u * (size_t)sc.slot_vertex[slot];
    const float* tb = sc.uvs + 2u * (size_t)sc.slot_vertex[(size_t)sc.n_tris + slot];
    const float* tc = sc.uvs + 2u * (size_t)sc.slot_vertex[2u * (size_t)sc.n_tris + slot];
    const uint32_t wrap = (d.flags & 2u) ? (uint32_t)RPT_TEX_WRAP_CLAMP : (uint32_t)RPT_TEX_WRAP_REPEAT;
    const uint32_t k = rpthost::cut_texel(u, v, ta[0], ta[1], tb[0], tb[1], tc[0], tc[1], d.width, d.height, wrap);
    return rpthost::cut_bit(sc.cut_bits + d.first, k);
}

// mesh_test_slot with the cut test behind the compare.
template <class S> RPT_DEV void mesh_test_slot_cut(const S& sc, const RayD& ray, uint32_t slot, float& best_t, uint32_t& best_index, uint32_t& best_slot)
{
    const TriRec r = tri_at(sc, slot);
    float t, u, v;
    if (hit_triangle_uv(ray, r.a, r.e1, r.e2, t, u, v) && (t < best_t || (t == best_t && r.index < best_index)) && cut_passes(sc, slot, r.index, u, v)) {
        best_t = t; best_index = r.index; best_slot = slot;
    }
}

// mesh_closest (dev_scene_mesh.h) over the triangles that pass the cut test.
template <class S> RPT_DEV uint32_t mesh_closest_cut(const S& sc, const RayD& ray, float& dist)
{
    float best_t = dist;
    uint32_t best_index = 0u, best_slot = kNoTriangle;
    MeshRay mr;
    if (mesh_ray_nan(ray)) return kNoTriangle;
    if (!sc.use_bvh || !mesh_ray_usable(ray, mr)) {
        for (uint32_t k = 0; k < sc.n_tris; ++k) mesh_test_slot_cut(sc, ray, k, best_t, best_index, best_slot);
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
                for (uint32_t k = 0; k < count; ++k) mesh_test_slot_cut(sc, ray, first + k, best_t, best_index, best_slot);
            }
            if (sp == 0u) break;
            sp -= 1u;
            cur = stk[sp * kMeshLanes];
        }
    }
    if (best_slot != kNoTriangle) dist = best_t;
    return best_slot;
}

// One candidate of the any-hit walk.
template <class S> RPT_DEV bool mesh_any_slot_cut(const S& sc, const RayD& ray, uint32_t slot, bool use_max, float max_dist)
{
    const TriRec r = tri_at(sc, slot);
    float t, u, v;
    return hit_triangle_uv(ray, r.a, r.e1, r.e2, t, u, v) && (!use_max || t < max_dist) && cut_passes(sc, slot, r.index, u, v);
}

// mesh_any (dev_scene_mesh.h) over the triangles that pass the cut test.
template <class S> RPT_DEV bool mesh_any_cut(const S& sc, const RayD& ray, bool use_max, float max_dist)
{
    MeshRay mr;
    if (mesh_ray_nan(ray)) return false;
    if (!sc.use_bvh || !mesh_ray_usable(ray, mr)) {
        for (uint32_t k = 0; k < sc.n_tris; ++k)
            if (mesh_any_slot_cut(sc, ray, k, use_max, max_dist)) return true;
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
            for (uint32_t k = 0; k < count; ++k)
                if (mesh_any_slot_cut(sc, ray, first + k, use_max, max_dist)) return true;
        }
        if (sp == 0u) break;
        sp -= 1u;
        cur = stk[sp * kMeshLanes];
    }
    return false;
}

// closest_geom of the mesh scenes (dev_scene_mesh.h) with the cut-aware walk.
template <class Base> RPT_DEV bool closest_geom(const SceneMeshCutT<Base>& sc, const RayD& ray, PathState& ps, GeomHit& g, EmitterHit& e)
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
    const uint32_t slot = mesh_closest_cut(sc, ray, dist);
    if (slot != kNoTriangle) { hit = true; code = sc.n_spheres + slot; }
    if (hit) ps.hit_dist = dist;
    g.code = code;
    return sample_lights_large(sc, ray, ps, e, hit);
}

// any_hit of the mesh scenes with the cut-aware walk.
template <class Base> RPT_DEV bool any_hit(const SceneMeshCutT<Base>& sc, const RayD& ray, float max_dist)
{
    const bool use_max = (sc.flags & RPT_SCENE_ANYHIT_USES_MAX_DIST) != 0;
    bool occluded = sc.use_accel ? grid_any_sphere(sc, ray, use_max, max_dist) : brute_any_sphere(sc, ray, use_max, max_dist);
    for (uint32_t k = 0; k < sc.n_planes; ++k) {
        float t;
        bool h = hit_plane(ray, sc.planes[k], t);
        occluded = occluded || (h && (!use_max || t < max_dist));
    }
    if (!occluded) occluded = mesh_any_cut(sc, ray, use_max, max_dist);
    return occluded;
}

}  // namespace rptdev
