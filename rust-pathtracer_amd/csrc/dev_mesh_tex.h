// dev_mesh_tex.h — mesh textures on the device (include/rpt.h, "mesh textures"): the material a winning triangle of a textured mesh
// is shaded with, the one function SceneMeshTexT overloads over its base.  dev_integrator.h reaches it by overload resolution alone:
// the other scene classes' kernels contain none of this.  Included after dev_scene_mesh.h, launch_tex.h, dev_mesh_smooth.h and
// dev_mesh_light.h, before regen_body.h.
#pragma once

namespace rptdev {

// The textured form over a scene with mesh lights samples and weighs them as its base does.
template <> struct MeshLights<SceneMeshLightTex> { static constexpr bool value = true; };

// hit_material of the mesh scenes, then rgb.c = m.rgb[c] * tex.c at a winning triangle of a textured mesh.  u and v are recomputed
// from the ray and the row the walk tested as dev_mesh_smooth.h's hit_normal does: the same operations on the same words give the
// same bits.  The interpolation, the wrap and the filter are host_tex.h's statement, compiled here for the device.
template <class Base> RPT_DEV void hit_material(const SceneMeshTexT<Base>& sc, const RayD& ray, const GeomHit& g, Mat& mat)
{
    hit_material(static_cast<const SceneMesh&>(sc), ray, g, mat);
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return;
    const TriRec r = tri_at(sc, slot);
    const uint32_t ord = sc.tri_tex[r.index];
    if (ord == rpthost::kTexNone) return;
    const v3 p = cross3(ray.d, r.e2);
    const float det = dot3(r.e1, p);
    const float inv = fdiv(1.0f, det);
    const v3 s = ray.o - r.a;
    const float u = dot3(s, p) * inv;
    const v3 q = cross3(s, r.e1);
    const float v = dot3(ray.d, q) * inv;
    const float w = (1.0f - u) - v;
    const float* ta = sc.uvs + 2u * (size_t)sc.slot_vertex[slot];
    const float* tb = sc.uvs + 2u * (size_t)sc.slot_vertex[(size_t)sc.n_tris + slot];
    const float* tc = sc.uvs + 2u * (size_t)sc.slot_vertex[2u * (size_t)sc.n_tris + slot];
    const float ss = rpthost::tex_interp(w, u, v, ta[0], tb[0], tc[0]);
    const float tt = rpthost::tex_interp(w, u, v, ta[1], tb[1], tc[1]);
    const rpthost::TexDesc d = sc.tex_desc[ord];
    float tex[3];
    rpthost::tex_lookup(sc.texels + d.first, d.width, d.height, d.wrap, d.filter, ss, tt, tex);
    mat.rgb = mk3(mat.rgb.x * tex[0], mat.rgb.y * tex[1], mat.rgb.z * tex[2]);
}

}  // namespace rptdev
