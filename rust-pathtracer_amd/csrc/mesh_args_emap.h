// mesh_args_emap.h — mesh_args_mmap.h's next part: the kernel arguments of the eight emission-mapped forms (launch_emap.h) and which
// of twenty-eight forms a launch takes.  Host code over plain structs, as mesh_args.h is: tests/emap_harness.cpp runs it under the
// address and undefined-behaviour sanitizers (tests/test_mesh_emission_map_host.py).  mesh_args.h and mesh_args_mmap.h stay as they
// are: every base part binds through mesh_map_scene_of<Base>.
//
// The one empty table this adds.  An emission-mapped form sits over a material-mapped one and is also taken by a scene with no
// material map ON.  The emission map's own allocation carries a block laid out as the material maps' tables with no texel
// (host_emap.h, EmapLayout::off_zero: all-zero descriptors — MmapDesc.flags == 0 already means "no map on this mesh" — and the
// all-0xFFFFFFFF table of MmapLayout::off_none), and mmap_view_of lends it exactly then; no rule of mesh_args_mmap.h changes.
#pragma once

#include "mesh_args_mmap.h"
#include "launch_emap.h"

namespace rptargs {

// One device's emission maps: the base of its allocation and the context's plan.
struct EmapView {
    void* emap;
    const rpthost::EmapPlan& emap_plan;
};

// The material maps an emission-mapped form binds: the device's own while some material map is ON, else the zero block.
inline MmapView mmap_view_of(const MmapView& maps, bool material_maps, const EmapView& e)
{
    if (material_maps) return maps;
    return MmapView{table_at<unsigned char>(e.emap, e.emap_plan.layout().off_zero), e.emap_plan.zero};
}

template <class S> struct emit_base_of;
template <class Base> struct emit_base_of<SceneMeshEmitT<Base>> { using type = Base; };

template <class Base> void bind_emap(const EmapView& e, SceneMeshEmitT<Base>& s)
{
    const rpthost::EmapLayout el = e.emap_plan.layout();
    s.emit_desc = table_at<const rpthost::EmapDesc>(e.emap, el.off_desc);
    s.emit_light_desc = table_at<const rpthost::EmapDesc>(e.emap, el.off_light_desc);
    s.emit_texels = table_at<const float4>(e.emap, el.off_texels);
}

// The kernel argument of the emission-mapped form S: Base's, from mesh_map_scene_of<Base>, then the map's part.
template <class S> S mesh_emit_scene_of(const MeshView& v, const MmapView& maps, bool material_maps, const EmapView& e)
{
    using Base = typename emit_base_of<S>::type;
    S s{};
    static_cast<Base&>(s) = mesh_map_scene_of<Base>(v, mmap_view_of(maps, material_maps, e));
    bind_emap(e, s);
    return s;
}

// Forms 20 .. 27: an emission map over the eight material-mapped forms, in their order.
constexpr uint32_t kMeshFormEmitFirst = 20u;
enum class MeshEmitForm : uint32_t { light_tex = 20, env, cut, cut_env, nrm, nrm_env, nrm_cut, nrm_cut_env };

// The form of a launch as a number: mesh_form_ext_of's value (0 .. 19) while no emission map is ON, else 20 + the index of the
// material-mapped form that would have run had a material map been ON — whether one is or not.  (An emission map needs a texture, so
// the three untextured forms cannot occur with one; they are kept.)
inline uint32_t mesh_form_emit_of(bool smooth, bool lights, bool textured, bool environment, bool cutouts, bool normal_maps, bool material_maps,
                                  bool emission_maps)
{
    if (!emission_maps) return mesh_form_ext_of(smooth, lights, textured, environment, cutouts, normal_maps, material_maps);
    const uint32_t over = mesh_form_ext_of(smooth, lights, textured, environment, cutouts, normal_maps, true);
    return over >= kMeshFormMapFirst ? over + (kMeshFormEmitFirst - kMeshFormMapFirst) : over;
}

}  // namespace rptargs
