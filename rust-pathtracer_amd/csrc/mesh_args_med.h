// mesh_args_med.h — mesh_args_emap.h's next part: the kernel arguments of the eight media forms (launch_med.h) and which of
// thirty-six forms a launch takes.  Host code over plain structs, as mesh_args.h is: tests/med_harness.cpp runs it on the host
// (tests/test_mesh_media_host.py).  mesh_args.h, mesh_args_mmap.h and mesh_args_emap.h stay as they are: every base part binds
// through mesh_emit_scene_of<Base>.
//
// The empty tables this adds.  A media form sits over an emission-mapped one and is also taken by a scene with no emission map, no
// texture, no mesh light and no smooth mesh: a glass mesh with a medium and nothing else.  The media's own allocation carries what
// such a scene lacks (host_med.h, MedLayout): an emission-map block with no map ON, lent as the EmapView while no emission map is
// ON; its all-0xFFFFFFFF table, lent as tri_tex while no mesh is textured and as tri_light while no mesh is ON; all-zero smooth
// bits, lent while no mesh is SMOOTH.  Each stands for an absent feature exactly as the tables the base composers lend, so a form
// reads the same values whichever allocation they come from.
#pragma once

#include "mesh_args_emap.h"
#include "launch_med.h"

namespace rptargs {

// One device's media: the base of its allocation and the context's plan.
struct MedView {
    void* med;
    const rpthost::MedPlan& med_plan;
};

// The emission maps a media form binds: the device's own while some emission map is ON, else the empty block.
inline EmapView emap_view_of(const EmapView& emits, bool emission_maps, const MedView& m)
{
    if (emission_maps) return emits;
    return EmapView{table_at<unsigned char>(m.med, m.med_plan.layout().off_emap), m.med_plan.zero_emap};
}

template <class S> struct med_base_of;
template <class Base> struct med_base_of<SceneMeshMedT<Base>> { using type = Base; };

template <class Base> void bind_med(const MeshView& v, const MedView& m, SceneMeshMedT<Base>& s)
{
    const rpthost::MedLayout ml = m.med_plan.layout();
    s.med_rows = table_at<const rpthost::MedRow>(m.med, ml.off_rows);
    s.tri_medium = table_at<const uint32_t>(m.med, ml.off_tri_medium);
    const uint32_t* all_ones = table_at<const uint32_t>(m.med, ml.off_all_ones());
    if (!v.has_smooth()) s.smooth_bits = table_at<const uint32_t>(m.med, ml.off_flat_bits);
    if (!v.has_lights()) s.tri_light = all_ones;
    if (!v.has_tex()) s.tri_tex = all_ones;
}

// The kernel argument of the media form S: Base's, from mesh_emit_scene_of<Base>, then the media's part.
template <class S> S mesh_med_scene_of(const MeshView& v, const MmapView& maps, bool material_maps, const EmapView& emits, bool emission_maps, const MedView& m)
{
    using Base = typename med_base_of<S>::type;
    S s{};
    static_cast<Base&>(s) = mesh_emit_scene_of<Base>(v, maps, material_maps, emap_view_of(emits, emission_maps, m));
    bind_med(v, m, s);
    return s;
}

// Forms 28 .. 35: a medium over the eight emission-mapped forms, in their order.
constexpr uint32_t kMeshFormMedFirst = 28u;
enum class MeshMedForm : uint32_t { light_tex = 28, env, cut, cut_env, nrm, nrm_env, nrm_cut, nrm_cut_env };

// The form of a launch as a number: mesh_form_emit_of's value (0 .. 27) while no mesh carries a medium, else 28 + the index of the
// emission-mapped form that would have run had an emission map been ON — whether one is or not.  The five forms that hold no
// environment, cutout or normal map (flat, smooth, light, tex, light_tex) all take the form over light_tex, with empty tables for
// what they lack.
inline uint32_t mesh_form_med_of(bool smooth, bool lights, bool textured, bool environment, bool cutouts, bool normal_maps, bool material_maps,
                                 bool emission_maps, bool media)
{
    if (!media) return mesh_form_emit_of(smooth, lights, textured, environment, cutouts, normal_maps, material_maps, emission_maps);
    switch (mesh_form_of(smooth, lights, textured, environment, cutouts, normal_maps)) {
    case MeshForm::env: return (uint32_t)MeshMedForm::env;
    case MeshForm::cut: return (uint32_t)MeshMedForm::cut;
    case MeshForm::cut_env: return (uint32_t)MeshMedForm::cut_env;
    case MeshForm::nrm: return (uint32_t)MeshMedForm::nrm;
    case MeshForm::nrm_env: return (uint32_t)MeshMedForm::nrm_env;
    case MeshForm::nrm_cut: return (uint32_t)MeshMedForm::nrm_cut;
    case MeshForm::nrm_cut_env: return (uint32_t)MeshMedForm::nrm_cut_env;
    default: return (uint32_t)MeshMedForm::light_tex;
    }
}

}  // namespace rptargs
