// mesh_args_mmap.h — mesh_args.h's next part: the kernel arguments of the eight material-mapped forms (launch_mmap.h) and which of
// twenty forms a launch takes.  Host code over plain structs, as mesh_args.h is: tests/mmap_harness.cpp runs it under the address
// and undefined-behaviour sanitizers (tests/test_mesh_material_map_host.py).  mesh_args.h stays as it is: MeshView, mesh_form_of,
// the twelve MeshForm values and mesh_scene_of<> are what they were, and every base part binds through mesh_scene_of<Base>.
//
// The one empty table this adds.  The form over SceneMeshLightTex is also taken by a scene with no mesh ON (mesh_form_ext_of), and
// that base has no part to borrow the all-0xFFFFFFFF tri_light from (all_ones_of: null).  The map's own allocation carries one
// (MmapLayout::off_none) and bind_mmap lends it exactly then; no rule of mesh_args.h changes.
#pragma once

#include "mesh_args.h"
#include "launch_mmap.h"

namespace rptargs {

// One device's material maps: the base of its allocation and the context's plan.
struct MmapView {
    void* mmap;
    const rpthost::MmapPlan& mmap_plan;
};

template <class S> struct map_base_of;
template <class Base> struct map_base_of<SceneMeshMapT<Base>> { using type = Base; };

template <class Base> void bind_mmap(const MmapView& m, SceneMeshMapT<Base>& s)
{
    const rpthost::MmapLayout ml = m.mmap_plan.layout();
    s.map_desc = table_at<const rpthost::MmapDesc>(m.mmap, ml.off_desc);
    s.map_texels = table_at<const float4>(m.mmap, ml.off_texels);
    if (!s.tri_light) s.tri_light = table_at<const uint32_t>(m.mmap, ml.off_none);     // (no mesh ON and no part of Base to lend the table)
}

// The kernel argument of the material-mapped form S: Base's, from mesh_scene_of<Base>, then the map's part.
template <class S> S mesh_map_scene_of(const MeshView& v, const MmapView& m)
{
    using Base = typename map_base_of<S>::type;
    S s{};
    static_cast<Base&>(s) = mesh_scene_of<Base>(v);
    bind_mmap(m, s);
    return s;
}

// Forms 12 .. 19: a material map over the eight textured forms that hold every table, in this order.
constexpr uint32_t kMeshFormMapFirst = 12u;
enum class MeshMapForm : uint32_t { light_tex = 12, env, cut, cut_env, nrm, nrm_env, nrm_cut, nrm_cut_env };

// The form of a launch as a number: mesh_form_of's value (0 .. 11) while no material map is ON, else 12 + the index of the textured
// form that would have run.  A scene whose base form is `tex` (no mesh ON) takes the map form over light_tex with empty light
// tables, as normal maps do.  (A material map needs a texture, so the three untextured forms cannot occur with one; they are kept.)
inline uint32_t mesh_form_ext_of(bool smooth, bool lights, bool textured, bool environment, bool cutouts, bool normal_maps, bool material_maps)
{
    const MeshForm base = mesh_form_of(smooth, lights, textured, environment, cutouts, normal_maps);
    if (!material_maps) return (uint32_t)base;
    switch (base) {
    case MeshForm::tex:
    case MeshForm::light_tex: return (uint32_t)MeshMapForm::light_tex;
    case MeshForm::env: return (uint32_t)MeshMapForm::env;
    case MeshForm::cut: return (uint32_t)MeshMapForm::cut;
    case MeshForm::cut_env: return (uint32_t)MeshMapForm::cut_env;
    case MeshForm::nrm: return (uint32_t)MeshMapForm::nrm;
    case MeshForm::nrm_env: return (uint32_t)MeshMapForm::nrm_env;
    case MeshForm::nrm_cut: return (uint32_t)MeshMapForm::nrm_cut;
    case MeshForm::nrm_cut_env: return (uint32_t)MeshMapForm::nrm_cut_env;
    default: return (uint32_t)base;
    }
}

}  // namespace rptargs
