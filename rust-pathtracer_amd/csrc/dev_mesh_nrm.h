// dev_mesh_nrm.h — mesh normal maps on the device (include/rpt.h, "mesh normal maps"): the normal a winning triangle of a
// normal-mapped mesh is shaded with, the one function SceneMeshNrmT overloads over its base.  dev_integrator.h reaches it by overload
// resolution alone: the other scene classes' kernels contain none of this.  Included after dev_mesh_cut.h and launch_nrm.h, before
// regen_body.h.
#pragma once

namespace rptdev {

// The normal-mapped forms sample and weigh mesh lights as their bases do (flat normal: the bend does not touch them), and have an
// environment exactly when their base has one.
template <class Base> struct MeshLights<SceneMeshNrmT<Base>> { static constexpr bool value = true; };
template <class Base> struct MeshEnv<SceneMeshNrmT<Base>> { static constexpr bool value = MeshEnv<Base>::value; };

// hit_normal of the base — flat, or "smooth mesh shading"'s — then the bend at a winning triangle of a mesh whose map is ON.  u and
// v are recomputed from the ray and the row the walk tested as dev_mesh_tex.h's hit_material does: the same operations on the same
// words give the same bits.  The interpolation, the wrap, the filter and the bend are host_tex.h's and host_nrm.h's statement,
// compiled here for the device.
template <class Base> RPT_DEV v3 hit_normal(const SceneMeshNrmT<Base>& sc, const RayD& ray, float dist, const GeomHit& g)
{
    const v3 n = hit_normal(static_cast<const Base&>(sc), ray, dist, g);
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return n;
    const TriRec r = tri_at(sc, slot);
    const uint32_t ord = sc.tri_tex[r.index];
    if (ord == rpthost::kTexNone) return n;
    const rpthost::NrmDesc d = sc.nrm_desc[ord];
    if (d.flags == 0u) return n;
    const v3 p = cross3(ray.d, r.e2);
    const float det = dot3(r.e1, p);
    const float inv = fdiv(1.0f, det);
    const v3 s = ray.o - r.a;
    const float u = dot3(s, p) * inv;
    const v3 q = cross3(s, r.e1);
    const float v = dot3(ray.d, q) * inv;
    const float* ta = sc.uvs + 2u * (size_t)sc.slot_vertex[slot];
    const float* tb = sc.uvs + 2u * (size_t)sc.slot_vertex[(size_t)sc.n_tris + slot];
    const float* tc = sc.uvs + 2u * (size_t)sc.slot_vertex[2u * (size_t)sc.n_tris + slot];
    const float nn[3] = {n.x, n.y, n.z}, e1[3] = {r.e1.x, r.e1.y, r.e1.z}, e2[3] = {r.e2.x, r.e2.y, r.e2.z};
    float out[3];
    rpthost::nrm_shade(nn, e1, e2, u, v, ta[0], ta[1], tb[0], tb[1], tc[0], tc[1],
                       reinterpret_cast<const rpthost::TexTexel*>(sc.nrm_texels) + d.first, d.width, d.height,
                       (d.flags & 2u) ? (uint32_t)RPT_TEX_WRAP_CLAMP : (uint32_t)RPT_TEX_WRAP_REPEAT,
                       (d.flags & 4u) ? (uint32_t)RPT_TEX_FILTER_BILINEAR : (uint32_t)RPT_TEX_FILTER_NEAREST, out);
    return mk3(out[0], out[1], out[2]);
}

}  // namespace rptdev
