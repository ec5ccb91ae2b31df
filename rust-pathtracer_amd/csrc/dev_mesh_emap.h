// dev_mesh_emap.h — mesh emission maps on the device (include/rpt.h, "mesh emission maps"): the emission a winning triangle of an
// emission-mapped mesh is shaded with, the emission the emitter exit adds for such a triangle behind an rpt_light, and the emission
// the mesh-light sampler hands out for a point on such a mesh — the three functions SceneMeshEmitT overloads over its base.
// dev_integrator.h reaches them by overload resolution alone: the other scene classes' kernels contain none of this.  Included after
// dev_mesh_mmap.h and launch_emap.h, before regen_body.h.
#pragma once

namespace rptdev {

// The emission-mapped forms sample and weigh mesh lights as their bases do (the pdf and the hit weight are untouched), and have an
// environment exactly when their base has one.
template <class Base> struct MeshLights<SceneMeshEmitT<Base>> { static constexpr bool value = true; };
template <class Base> struct MeshEnv<SceneMeshEmitT<Base>> { static constexpr bool value = MeshEnv<Base>::value; };

// e.c = e.c * E.c at the hit `g` of `ray`, when it is a winning triangle of a mesh whose map is ON.  u and v are recomputed from the
// ray and the row the walk tested as dev_mesh_mmap.h's hit_material does: the same operations on the same words give the same bits.
template <class Base> RPT_DEV void mesh_emit_apply(const SceneMeshEmitT<Base>& sc, const RayD& ray, const GeomHit& g, v3& e)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return;
    const TriRec r = tri_at(sc, slot);
    const uint32_t ord = sc.tri_tex[r.index];
    if (ord == rpthost::kTexNone) return;
    const rpthost::EmapDesc d = sc.emit_desc[ord];
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
    float E[3];
    rpthost::emap_lookup_desc(d, reinterpret_cast<const rpthost::TexTexel*>(sc.emit_texels), u, v, ta, tb, tc, E);
    float em[3] = {e.x, e.y, e.z};
    rpthost::emap_apply(em, E);
    e = mk3(em[0], em[1], em[2]);
}

// hit_material of the base — which has written emission, and roughness and metallic under a material map — then the product.
template <class Base> RPT_DEV void hit_material(const SceneMeshEmitT<Base>& sc, const RayD& ray, const GeomHit& g, Mat& mat)
{
    hit_material(static_cast<const Base&>(sc), ray, g, mat);
    mesh_emit_apply(sc, ray, g, mat.emission);
}

// The emitter exit's term (dev_integrator.h, hit_emission_at): the base's hit_emission, then the same product.
template <class Base> RPT_DEV v3 hit_emission_at(const SceneMeshEmitT<Base>& sc, const RayD& ray, const GeomHit& g)
{
    v3 e = hit_emission(static_cast<const Base&>(sc), g);
    mesh_emit_apply(sc, ray, g, e);
    return e;
}

// "Sampling an ON mesh" with the emission line of an emission-mapped mesh: the base's sampler — triangle, point, normal, pdf, all
// unchanged — then, when ON mesh `ord` has a map, emission.c = N_f * (m.emission[c] * E.c) with E looked up at the sampled point's
// (bu, bv), recomputed from r1 and r2 by the sampler's own three operations.  Returns the sampler's k.
template <class Base> RPT_DEV uint32_t mesh_light_sample_emit(const SceneMeshEmitT<Base>& sc, uint32_t ord, v3 scatter_pos, float r0a, float r0b, float r1, float r2,
                                                            LightSample& ls, float& light_area)
{
    const uint32_t k = mesh_light_sample(static_cast<const SceneMeshLight&>(sc), ord, scatter_pos, r0a, r0b, r1, r2, ls, light_area);
    if (k == kNoMeshLight) return k;
    const rpthost::EmapDesc d = sc.emit_light_desc[ord];
    if (d.flags == 0u) return k;
    const LightMeshDesc* ld = sc.light_desc + ord;
    const size_t f = (size_t)ld->first + k, nf = sc.n_faces;
    const float* ta = sc.uvs + 2u * (size_t)sc.face_vertex[f];
    const float* tb = sc.uvs + 2u * (size_t)sc.face_vertex[nf + f];
    const float* tc = sc.uvs + 2u * (size_t)sc.face_vertex[2u * nf + f];
    const float su = fsqrt(r1);
    const float bu = 1.0f - su;
    const float bv = r2 * su;
    float E[3];
    rpthost::emap_lookup_desc(d, reinterpret_cast<const rpthost::TexTexel*>(sc.emit_texels), bu, bv, ta, tb, tc, E);
    const DevMaterial m = gather32(sc.materials, ld->material);
    float out[3];
    rpthost::emap_sample_emission(m.emission, E, sc.n_lights_f, out);
    ls.emission = mk3(out[0], out[1], out[2]);
    return k;
}

// nee_sample's branch for a light index at or past n_lights: the four draws, always, then the sampler above.  Returns light.area.
template <class Base> RPT_DEV float mesh_light_nee(const SceneMeshEmitT<Base>& sc, uint32_t ord, v3 scatter_pos, LightSample& ls, Rng& rng)
{
    const float r0a = rng.gen();
    const float r0b = rng.gen();
    const float r1 = rng.gen();
    const float r2 = rng.gen();
    float light_area;
    (void)mesh_light_sample_emit(sc, ord, scatter_pos, r0a, r0b, r1, r2, ls, light_area);
    return light_area;
}

}  // namespace rptdev
