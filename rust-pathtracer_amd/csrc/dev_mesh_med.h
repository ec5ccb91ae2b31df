// dev_mesh_med.h — mesh media on the device (include/rpt.h, "mesh media"): which medium a hit carries, that medium's row, and the
// normal step 4's side test reads — the three functions SceneMeshMedT overloads.  Everything else is its base's (the walks, the
// normals, the materials, the samplers, the hit weights) and dev_media.h's (phase_hg, sample_hg, medium_transmittance) through the
// media branches of dev_integrator.h, which reach these by overload resolution alone: the other scene classes' kernels contain none
// of this.  Included after dev_mesh_emap.h and launch_med.h, before regen_body.h.
#pragma once

namespace rptdev {

// The media forms sample and weigh mesh lights as their bases do, and have an environment exactly when their base has one.
template <class Base> struct MeshLights<SceneMeshMedT<Base>> { static constexpr bool value = true; };
template <class Base> struct MeshEnv<SceneMeshMedT<Base>> { static constexpr bool value = MeshEnv<Base>::value; };

// "Which medium a hit carries": the winning triangle's mesh's ordinal; a sphere, a plane or a triangle of a mesh without a medium
// carries none.
template <class Base> RPT_DEV uint32_t hit_medium_index(const SceneMeshMedT<Base>& sc, const GeomHit& g)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return kNoMediumIdx;
    static_assert(rpthost::kMedNone == kNoMediumIdx, "host_med.h's none is dev_media.h's");
    return rpthost::med_ordinal_of(sc.tri_medium, tri_at(sc, slot).index);
}

// The row of medium ordinal `index` (per lane: two 16-byte gathers).  The anisotropy was clamped by the setter.
template <class Base> RPT_DEV DevMedium mesh_medium_row(const SceneMeshMedT<Base>& sc, uint32_t index)
{
    const float4* rows = reinterpret_cast<const float4*>(sc.med_rows);
    const float4 r0 = gather32(rows, 2u * index), r1 = gather32(rows, 2u * index + 1u);
    return DevMedium{rpt_f2u(r0.x), r0.y, mk3(r0.z, r0.w, r1.x), r1.y};
}

// Step 4's side test reads G, the flat normal of the winning triangle, whatever smooth shading or a normal map made of `normal`.
// (Only called for a hit that carries a medium: a winning triangle.)
template <class Base> RPT_DEV v3 medium_side_normal(const SceneMeshMedT<Base>& sc, const GeomHit& g, v3 normal)
{
    const uint32_t slot = mesh_slot_of(sc, g.code);
    if (slot == kNoTriangle) return normal;
    const TriRec r = tri_at(sc, slot);
    return norm3(cross3(r.e1, r.e2));
}

}  // namespace rptdev

// medium_at(sc, index) has no argument of rptdev's: the path functions of dev_integrator.h, defined before this file is read, find an
// overload for these scene types only in the namespace of the scene type itself (argument-dependent lookup).  So it lives here and
// forwards.  (hit_medium_index and medium_side_normal take a GeomHit, which is rptdev's.)
namespace rptscene {

template <class Base> RPT_DEV rptdev::DevMedium medium_at(const SceneMeshMedT<Base>& sc, uint32_t index) { return rptdev::mesh_medium_row(sc, index); }

}  // namespace rptscene
