// dev_mesh_mmap.h — mesh material maps on the device (include/rpt.h, "mesh material maps"): the material a winning triangle of a
// material-mapped mesh is shaded with, the one function SceneMeshMapT overloads over its base.  dev_integrator.h reaches it by
// overload resolution alone: the other scene classes' kernels contain none of this.  Included after dev_mesh_nrm.h and
// launch_mmap.h, before regen_body.h.
#pragma once

namespace rptdev {

// The material-mapped forms sample and weigh mesh lights as their bases do (emission is untouched), and have an environment
// exactly when their base has one.
template <class Base> struct MeshLights<SceneMeshMapT<Base>> { static constexpr bool value = true; };
template <class Base> struct MeshEnv<SceneMeshMapT<Base>> { static constexpr bool value = MeshEnv<Base>::value; };

// hit_material of the base — "mesh textures"' one, which has written rgb — then roughness *= fr and metallic *= fm at a winning
// triangle of a mesh whose map is ON.  u and v are recomputed from the ray and the row the walk tested as dev_mesh_tex.h's
// hit_material does: the same operations on the same words give the same bits.  The interpolation, the wrap and the filter are
// host_tex.h's statement and the lookup host_mmap.h's, compiled here for the device.
template <class Base> RPT_DEV void hit_material(const SceneMeshMapT<Base>& sc, const RayD& ray, const GeomHit& g, Mat& mat)
{
    hit_material(static_cast<const Base&>(sc), ray, g, mat);
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return;
    const TriRec r = tri_at(sc, slot);
    const uint32_t ord = sc.tri_tex[r.index];
    if (ord == rpthost::kTexNone) return;
    const rpthost::MmapDesc d = sc.map_desc[ord];
    if (d.flags == 0u) return;
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
    float f[2];
    rpthost::mmap_factors(u, v, ta[0], ta[1], tb[0], tb[1], tc[0], tc[1], reinterpret_cast<const rpthost::TexTexel*>(sc.map_texels) + d.first, d.width,
                          d.height, (d.flags & 2u) ? (uint32_t)RPT_TEX_WRAP_CLAMP : (uint32_t)RPT_TEX_WRAP_REPEAT,
                          (d.flags & 4u) ? (uint32_t)RPT_TEX_FILTER_BILINEAR : (uint32_t)RPT_TEX_FILTER_NEAREST, f);
    rpthost::mmap_apply(mat.roughness, mat.metallic, f);
}

}  // namespace rptdev
