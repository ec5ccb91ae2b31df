// dev_mesh_smooth.h — the normal a winning triangle is shaded with in a scene some mesh of which may be SMOOTH (include/rpt.h, "smooth
// mesh shading"): the one function SceneMeshSmooth overloads over dev_scene_mesh.h.  A header of its own because two kernels call
// it: k_smooth.hip's and, for scenes with mesh lights, k_light.hip's.  Included after dev_scene_mesh.h and launch_smooth.h.
#pragma once

namespace rptdev {

// include/rpt.h, "normal of a winning triangle of a SMOOTH mesh".  u and v are recomputed from the ray and the row the walk tested:
// the same operations on the same words give the same bits (hit_triangle above; nothing here is contracted or reassociated).
RPT_DEV v3 hit_normal(const SceneMeshSmooth& sc, const RayD& ray, float dist, const GeomHit& g)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return normal_large(sc, ray, dist, g);
    const TriRec r = tri_at(sc, slot);
    if (((sc.smooth_bits[r.index >> 5] >> (r.index & 31u)) & 1u) != 0u) {
        const v3 p = cross3(ray.d, r.e2);
        const float det = dot3(r.e1, p);
        const float inv = fdiv(1.0f, det);
        const v3 s = ray.o - r.a;
        const float u = dot3(s, p) * inv;
        const v3 q = cross3(s, r.e1);
        const float v = dot3(ray.d, q) * inv;
        const float w = (1.0f - u) - v;
        const float4 na = sc.vnormals[sc.slot_vertex[slot]];
        const float4 nb = sc.vnormals[sc.slot_vertex[(size_t)sc.n_tris + slot]];
        const float4 nc = sc.vnormals[sc.slot_vertex[2u * (size_t)sc.n_tris + slot]];
        const v3 m = mk3((w * na.x + u * nb.x) + v * nc.x, (w * na.y + u * nb.y) + v * nc.y, (w * na.z + u * nb.z) + v * nc.z);
        const float l2 = dot3(m, m);
        if (l2 > 0.0f && l2 <= 3.40282347e+38f) return norm3(m);    // (norm3: the root of this very sum, three divides)
    }
    return norm3(cross3(r.e1, r.e2));
}

}  // namespace rptdev
