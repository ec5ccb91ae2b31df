// mesh_args_rad.h — mesh_args_med.h's part for radiance queries: the kernel arguments of the eight radiance forms (launch_rad.h),
// which sit over the media forms' scene types and are taken by EVERY mesh scene, whatever it has ON.  Host code over plain structs, as
// mesh_args.h is: tests/rad_harness.cpp runs it on the host (tests/test_radiance_f64.py).  mesh_args.h, mesh_args_mmap.h,
// mesh_args_emap.h and mesh_args_med.h stay as they are: every part binds through mesh_med_scene_of<S>.
//
// The one choice this adds.  mesh_med_scene_of binds the media's allocation and lends from it the tables of every feature below the
// media that is absent.  While some mesh carries a medium that allocation is the device's own (MedView{d.med, ctx->med}), and a
// radiance form reads the very tables the render's media form reads.  While none does, it is the radiance query's own
// (host_rad.h): the media tables of a scene without media — tri_medium all kMedNone, so no hit carries a medium and no path enters
// one.  The environment, cutout and normal-map parts have no empty form: a form that has one is only taken while the feature is
// present (rad_form_of).
#pragma once

#include "mesh_args_med.h"
#include "launch_rad.h"

namespace rptargs {

// One device's radiance allocation: its base and the context's plan of it.
struct RadView {
    void* rad;
    const rpthost::MedPlan& rad_plan;
};

// The media a radiance form binds: the device's own while some mesh carries a medium, else the query's.
inline MedView rad_med_view_of(const MedView& meds, bool media, const RadView& r)
{
    if (media) return meds;
    return MedView{r.rad, r.rad_plan};
}

// The kernel argument of the radiance form over S (SceneMeshMed, ...Env, ...Cut, ... NrmCutEnv).  v.refit is present (the caller
// makes it: mesh_scene_of binds slot_vertex and the vertices from it).
template <class S> S mesh_rad_scene_of(const MeshView& v, const MmapView& maps, bool material_maps, const EmapView& emits, bool emission_maps, const MedView& meds,
                                       bool media, const RadView& r)
{
    return mesh_med_scene_of<S>(v, maps, material_maps, emits, emission_maps, rad_med_view_of(meds, media, r));
}

}  // namespace rptargs
