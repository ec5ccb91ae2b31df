// mesh_args_query.h — mesh_args_emap.h's part for ray queries: the kernel arguments of the four surface kernels (launch_query.h),
// which sit over the emission-mapped forms without an environment and are taken by EVERY mesh scene, whatever it has ON.  Host code
// over plain structs, as mesh_args.h is: tests/query_harness.cpp runs it on the host (tests/test_query_host.py).  mesh_args.h,
// mesh_args_mmap.h and mesh_args_emap.h stay as they are: the parts a scene has bind through their own binders.
//
// The empty tables.  A surface kernel reads the smooth bits, tri_light, tri_tex and the material-map and emission-map descriptors of
// scenes that have none of them.  The query's own allocation (host_query.h, QueryLayout) carries all-zero smooth bits, an
// all-0xFFFFFFFF table and all-zero descriptors, lent exactly while the feature is absent: each stands for it as the tables the
// base composers lend, so a kernel reads the same values whichever allocation they come from.  The cutout and normal-map parts have
// no empty form: a kernel that has one is only taken while the feature is present (query_surface_kind_of).
#pragma once

#include "mesh_args_emap.h"
#include "launch_query.h"

namespace rptargs {

static_assert(sizeof(rpthost::MmapDesc) <= rpthost::kQueryDescBytes && sizeof(rpthost::EmapDesc) <= rpthost::kQueryDescBytes,
              "the query allocation's zero descriptors stand for every map descriptor");

// One device's query allocation: its base and layout.
struct QueryView {
    void* query;
    rpthost::QueryLayout layout;
};

// The kernel argument of the surface kernel over S (SceneMeshEmit, ...Cut, ...Nrm, ...NrmCut).  v.refit is present (the caller makes
// it: mesh_scene_of binds slot_vertex from it).
template <class S> S mesh_query_scene_of(const MeshView& v, const MmapView& maps, bool material_maps, const EmapView& emits, bool emission_maps, const QueryView& qv)
{
    using MapS = typename emit_base_of<S>::type;
    using Base = typename map_base_of<MapS>::type;
    S s{};
    static_cast<Base&>(s) = mesh_scene_of<Base>(v);
    const uint32_t* none = table_at<const uint32_t>(qv.query, qv.layout.off_none);
    if (!v.has_smooth()) s.smooth_bits = table_at<const uint32_t>(qv.query, qv.layout.off_flat_bits);
    if (!v.has_lights()) s.tri_light = none;
    if (!v.has_tex()) s.tri_tex = none;
    if (material_maps) {
        bind_mmap(maps, static_cast<MapS&>(s));
    } else {
        s.map_desc = table_at<const rpthost::MmapDesc>(qv.query, qv.layout.off_zero);
        s.map_texels = nullptr;                                     // (not read: no descriptor names a map)
    }
    if (emission_maps) {
        bind_emap(emits, s);
    } else {
        s.emit_desc = table_at<const rpthost::EmapDesc>(qv.query, qv.layout.off_zero);
        s.emit_light_desc = s.emit_desc;
        s.emit_texels = nullptr;
    }
    return s;
}

// Which of the four surface kernels, and of the two closest / occluded kernels (bit 0 alone), a query takes.
enum : uint32_t { kQueryCut = 1u, kQueryNrm = 2u };
inline uint32_t query_surface_kind_of(bool cutouts, bool normal_maps) { return (cutouts ? kQueryCut : 0u) | (normal_maps ? kQueryNrm : 0u); }

}  // namespace rptargs
