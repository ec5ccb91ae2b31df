// dev_mesh_light.h — mesh lights on the device (include/rpt.h, "mesh lights"): the sampler over an ON mesh's surface and the weight of
// a hit on one, for SceneMeshLight only.  dev_integrator.h reaches both through `if constexpr (MeshLights<S>::value)`: the other
// scene classes' kernels contain none of this.  Included after dev_scene_mesh.h and launch_light.h, before regen_body.h.
#pragma once

namespace rptdev {

template <> struct MeshLights<SceneMeshLight> { static constexpr bool value = true; };

constexpr uint32_t kNoMeshLight = 0xFFFFFFFFu;

// Sampling ON mesh `ord` from scatter_pos with the draws r0a, r0b, r1, r2 (multiples of 2^-24 in [0, 1)).  Returns the triangle's
// index within the mesh (0xFFFFFFFF: the mesh is dark and `ls` keeps LightSampleRec::new()'s zeros) and, in light_area, A_tot.
RPT_DEV uint32_t mesh_light_sample(const SceneMeshLight& sc, uint32_t ord, v3 scatter_pos, float r0a, float r0b, float r1, float r2, LightSample& ls,
                                   float& light_area)
{
    ls.normal = mk3(0.0f, 0.0f, 0.0f); ls.emission = mk3(0.0f, 0.0f, 0.0f); ls.direction = mk3(0.0f, 0.0f, 0.0f);
    ls.dist = 0.0f; ls.pdf = 0.0f;                                  // LightSampleRec::new, globals.rs:119-129
    const LightMeshDesc* d = sc.light_desc + ord;
    const float a_tot = d->area;
    light_area = a_tot;
    if (!(a_tot > 0.0f)) return kNoMeshLight;
    const uint32_t first = d->first, n = d->n;
    const uint64_t* cdf = sc.light_cdf + first;
    // the triangle: J has 48 bits, T = (J * Q) >> 48 < Q, k = the first index with C_k > T
    const uint64_t j = ((uint64_t)(uint32_t)(r0a * 16777216.0f) << 24) | (uint64_t)(uint32_t)(r0b * 16777216.0f);
    const uint64_t t = __umul64hi(j << 16, cdf[n - 1u]);
    uint32_t lo = 0u, hi = n - 1u;                                  // C_{n-1} = Q > T: the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1u;
    }
    const uint32_t k = lo;
    const size_t f = (size_t)first + k, nf = sc.n_faces;
    const float* pa = sc.vertices + 3u * (size_t)sc.face_vertex[f];
    const float* pb = sc.vertices + 3u * (size_t)sc.face_vertex[nf + f];
    const float* pc = sc.vertices + 3u * (size_t)sc.face_vertex[2u * nf + f];
    const v3 a = mk3(pa[0], pa[1], pa[2]);
    const v3 e1 = mk3(pb[0], pb[1], pb[2]) - a, e2 = mk3(pc[0], pc[1], pc[2]) - a;
    // the point
    const float su = fsqrt(r1);
    const float bu = 1.0f - su;
    const float bv = r2 * su;
    const v3 p = mk3((a.x + bu * e1.x) + bv * e2.x, (a.y + bu * e1.y) + bv * e2.y, (a.z + bu * e1.z) + bv * e2.z);
    ls.direction = p - scatter_pos;
    ls.dist = len3(ls.direction);
    const float dist_sq = ls.dist * ls.dist;
    ls.direction = divs3(ls.direction, ls.dist);
    // the normal, turned against the direction: the mesh emits from both sides
    const v3 nrm = norm3(cross3(e1, e2));
    const float c = dot3(nrm, ls.direction);
    ls.normal = (c > 0.0f) ? -nrm : nrm;
    const DevMaterial m = gather32(sc.materials, d->material);
    ls.emission = sc.n_lights_f * mk3(m.emission[0], m.emission[1], m.emission[2]);
    ls.pdf = fdiv(dist_sq, a_tot * __builtin_fabsf(c));
    return k;
}

// nee_sample's branch for a light index at or past n_lights: the four draws, always, then the sampler.  Returns light.area.
RPT_DEV float mesh_light_nee(const SceneMeshLight& sc, uint32_t ord, v3 scatter_pos, LightSample& ls, Rng& rng)
{
    const float r0a = rng.gen();
    const float r0b = rng.gen();
    const float r1 = rng.gen();
    const float r2 = rng.gen();
    float light_area;
    (void)mesh_light_sample(sc, ord, scatter_pos, r0a, r0b, r1, r2, ls, light_area);
    return light_area;
}

// The weight w of the emission term of the hit `g` (include/rpt.h, "hit side"): 1 unless the ray won a triangle of an ON, not dark,
// mesh after the first bounce; then the power heuristic of the previous bounce's scatter pdf against the pdf the sampler has for
// this point, with the flat normal whatever the mesh's shading mode.
RPT_DEV float mesh_light_hit_weight(const SceneMeshLight& sc, const RayD& ray, const PathState& ps, uint32_t bounce, const GeomHit& g)
{
    if (bounce == 0u) return 1.0f;
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return 1.0f;
    const TriRec r = tri_at(sc, slot);
    const uint32_t ord = sc.tri_light[r.index];
    if (ord == kNoMeshLight) return 1.0f;
    const float a_tot = sc.light_desc[ord].area;
    if (!(a_tot > 0.0f)) return 1.0f;
    const float c = __builtin_fabsf(dot3(ray.d, norm3(cross3(r.e1, r.e2))));
    if (!(c > 0.0f)) return 1.0f;
    const float lp = fdiv(ps.hit_dist * ps.hit_dist, a_tot * c);
    return power_heuristic(ps.scatter_pdf, lp);
}

}  // namespace rptdev
