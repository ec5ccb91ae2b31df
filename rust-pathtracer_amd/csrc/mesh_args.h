// mesh_args.h — a mesh scene's kernel arguments, bound from per-feature parts (capi.hip: launch_render and the debug hooks), and which
// of the twelve render forms a launch takes.  Host code over plain structs: no context, no HIP call, so tests/args_harness.cpp runs it
// under the address and undefined-behaviour sanitizers (tests/test_mesh_args_host.py).
//
// The argument types form a chain — SceneMesh < SceneMeshSmooth < SceneMeshLight, then SceneMeshTexT<>, SceneMeshEnvT<>,
// SceneMeshCutT<>, SceneMeshNrmT<> over them (launch_*.h) — and mesh_scene_of<S> walks S's chain: one binder per part S has.  A binder
// binds its feature's tables while the feature is PRESENT (the device holds the allocation and the plan says some mesh uses it), else
// the empty tables that make the kernel skip the feature: all-zero smooth bits (every hit takes the flat normal), an all-0xFFFFFFFF
// tri_light / tri_tex (no triangle belongs to an ON or a textured mesh).  The cutout and normal-map parts have no empty form: a form
// that has one is only taken while the feature is present (mesh_form_of), and so is the environment part.
//
// Where the empty tables come from — every allocation that may have to lend one carries it, sized by the scene's triangles
// (host_*.h, the layouts' off_flat_bits / off_none), and S's own parts decide, in this order:
//   flat smooth bits:  the light allocation while S has the light part and lights are present; else the environment allocation if S
//                      has the environment part; else the texture allocation (if S has that part)
//   the all-ones table: the environment allocation if S has that part; else the cutout allocation if S has that part; else the
//                      normal-map allocation (if S has that part)
// A form with no part to borrow from never needs the table: it is only taken while its own features are present.
#pragma once

#include <type_traits>

#include "host_refit.h"
#include "host_smooth.h"
#include "host_light.h"
#include "launch_nrm.h"             // and through it launch_cut.h, launch_env.h, launch_tex.h, launch_light.h, launch_smooth.h

namespace rptargs {

using namespace rptscene;

// One device's mesh scene as the binders see it: its SceneMesh, the bases of its allocations (null: none), the context's plans.
struct MeshView {
    const SceneMesh& scene;
    void *refit, *smooth, *light, *tex, *env, *cut, *nrm;
    const rpthost::RefitPlan& refit_plan;
    const rpthost::SmoothPlan& smooth_plan;
    const rpthost::LightPlan& light_plan;
    const rpthost::TexPlan& tex_plan;
    const rpthost::EnvPlan& env_plan;
    const rpthost::CutPlan& cut_plan;
    const rpthost::NrmPlan& nrm_plan;

    bool has_smooth() const { return smooth && smooth_plan.any(); }
    bool has_lights() const { return light && light_plan.any(); }
    bool has_tex() const { return tex && tex_plan.any(); }
    // (the vertices and slot_vertex come first in the refit tables whatever follows them)
    rpthost::RefitLayout refit_layout() const { return rpthost::RefitLayout(refit_plan.n_vertices(), 0, 0); }
};

template <class T> T* table_at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + offset); }

// S has the part Part<some base>
template <template <class> class Part, class S> struct has_part {
    template <class B> static std::true_type test(const Part<B>*);
    static std::false_type test(const void*);
    static constexpr bool value = decltype(test(static_cast<const S*>(nullptr)))::value;
};

// ---- the empty tables (the rule at the top of this file) ---------------------------------------------------------------------------
template <class S> const uint32_t* flat_bits_of(const MeshView& v)
{
    if constexpr (std::is_base_of<SceneMeshLight, S>::value) {
        if (v.has_lights()) return table_at<uint32_t>(v.light, v.light_plan.layout().off_flat_bits);
    }
    if constexpr (has_part<SceneMeshEnvT, S>::value) return table_at<uint32_t>(v.env, v.env_plan.layout().off_flat_bits);
    else if constexpr (has_part<SceneMeshTexT, S>::value) return table_at<uint32_t>(v.tex, v.tex_plan.layout().off_flat_bits);
    else return nullptr;
}

template <class S> const uint32_t* all_ones_of(const MeshView& v)
{
    if constexpr (has_part<SceneMeshEnvT, S>::value) return table_at<uint32_t>(v.env, v.env_plan.layout().off_none);
    else if constexpr (has_part<SceneMeshCutT, S>::value) return table_at<uint32_t>(v.cut, v.cut_plan.layout().off_none);
    else if constexpr (has_part<SceneMeshNrmT, S>::value) return table_at<uint32_t>(v.nrm, v.nrm_plan.layout().off_none);
    else return nullptr;
}

// ---- one binder per part -----------------------------------------------------------------------------------------------------------
// smooth, or flat: the refit's slot_vertex and `flat_bits`
inline void bind_smooth(const MeshView& v, SceneMeshSmooth& s, const uint32_t* flat_bits)
{
    const rpthost::SmoothLayout sl = v.smooth_plan.layout();
    s.slot_vertex = table_at<const uint32_t>(v.refit, v.refit_layout().off_slot_vertex);
    s.vnormals = v.has_smooth() ? table_at<const float4>(v.smooth, sl.off_normals) : nullptr;      // (null: not read, no smooth bit is set)
    s.smooth_bits = v.has_smooth() ? table_at<const uint32_t>(v.smooth, sl.off_bits) : flat_bits;
}

// The table kernels' argument: pointers into the device's light tables.
inline LightTables light_tables_of(const MeshView& v)
{
    const rpthost::LightPlan& lp = v.light_plan;
    const rpthost::LightLayout ll = lp.layout();
    LightTables t{};
    t.desc = table_at<LightMeshDesc>(v.light, ll.off_desc);
    t.cdf = table_at<uint64_t>(v.light, ll.off_cdf);
    t.part = table_at<uint64_t>(v.light, ll.off_part);
    t.block = table_at<uint64_t>(v.light, ll.off_block);
    t.area = table_at<float>(v.light, ll.off_area);
    t.face_vertex = table_at<const uint32_t>(v.light, ll.off_face_vertex);
    t.face_mesh = table_at<const uint32_t>(v.light, ll.off_face_mesh);
    t.n_on = lp.n_on();
    t.n_faces = lp.n_faces;
    return t;
}

// mesh lights, or none: `all_ones` for tri_light and nothing to pick beyond the scene's own lights
inline void bind_lights(const MeshView& v, SceneMeshLight& s, const uint32_t* all_ones)
{
    s.vertices = table_at<const float>(v.refit, v.refit_layout().off_vertices);
    if (v.has_lights()) {
        const LightTables t = light_tables_of(v);
        s.face_vertex = t.face_vertex;
        s.light_desc = t.desc;
        s.light_cdf = t.cdf;
        s.tri_light = table_at<const uint32_t>(v.light, v.light_plan.layout().off_tri_light);
        s.n_faces = t.n_faces;
        s.n_pick = s.n_lights + t.n_on;
        s.n_lights_f = (float)s.n_pick;                             // include/rpt.h, "pickable lights": N_f
    } else {
        s.face_vertex = nullptr;                                    // (not read: no mesh is ON)
        s.light_desc = nullptr;
        s.light_cdf = nullptr;
        s.tri_light = all_ones;
        s.n_faces = 0u;
        s.n_pick = s.n_lights;
    }
}

// textures, or none: `all_ones` for tri_tex
template <class Base> void bind_tex(const MeshView& v, SceneMeshTexT<Base>& s, const uint32_t* all_ones)
{
    const rpthost::TexLayout tl = v.tex_plan.layout();
    const bool on = v.has_tex();                                    // (off: nothing but tri_tex is read, no triangle names a texture)
    s.tex_desc = on ? table_at<const rpthost::TexDesc>(v.tex, tl.off_desc) : nullptr;
    s.tri_tex = on ? table_at<const uint32_t>(v.tex, tl.off_tri_tex) : all_ones;
    s.uvs = on ? table_at<const float>(v.tex, tl.off_uvs) : nullptr;
    s.texels = on ? table_at<const rpthost::TexTexel>(v.tex, tl.off_texels) : nullptr;
}

// the environment; SAMPLED, it is the last of the pickable lights (include/rpt.h, "pickable lights")
template <class Base> void bind_env(const MeshView& v, SceneMeshEnvT<Base>& s)
{
    const rpthost::EnvPlan& ep = v.env_plan;
    const rpthost::EnvLayout el = ep.layout();
    s.env_texels = table_at<const rpthost::EnvTexel>(v.env, el.off_texels);
    s.env_cdf = ep.sampled() ? table_at<const uint64_t>(v.env, el.off_cdf) : nullptr;
    s.env_q = ep.q_total;
    s.env_q_f = (float)ep.q_total;
    s.env_scale = ep.scale;
    s.env_size = ep.size;
    s.env_pick = rpthost::kEnvNone;
    if (ep.sampled()) {
        s.env_pick = s.n_pick;
        s.n_pick += 1u;
        s.n_lights_f = (float)s.n_pick;
    }
}

template <class Base> void bind_cut(const MeshView& v, SceneMeshCutT<Base>& s)
{
    const rpthost::CutLayout cl = v.cut_plan.layout();
    s.cut_desc = table_at<const rpthost::CutDesc>(v.cut, cl.off_desc);
    s.cut_bits = table_at<const uint32_t>(v.cut, cl.off_bits);
}

template <class Base> void bind_nrm(const MeshView& v, SceneMeshNrmT<Base>& s)
{
    const rpthost::NrmLayout nl = v.nrm_plan.layout();
    s.nrm_desc = table_at<const rpthost::NrmDesc>(v.nrm, nl.off_desc);
    s.nrm_texels = table_at<const float4>(v.nrm, nl.off_texels);
}

// ---- the composer ------------------------------------------------------------------------------------------------------------------
// The kernel argument of form S (SceneMesh or any type of the chain over it) for the device of `v`; cam and flags are the scene's.
template <class S> S mesh_scene_of(const MeshView& v)
{
    S s{};
    static_cast<SceneMesh&>(s) = v.scene;
    if constexpr (std::is_base_of<SceneMeshSmooth, S>::value) bind_smooth(v, s, flat_bits_of<S>(v));
    if constexpr (std::is_base_of<SceneMeshLight, S>::value) bind_lights(v, s, all_ones_of<S>(v));
    if constexpr (has_part<SceneMeshTexT, S>::value) bind_tex(v, s, all_ones_of<S>(v));
    if constexpr (has_part<SceneMeshEnvT, S>::value) bind_env(v, s);
    if constexpr (has_part<SceneMeshCutT, S>::value) bind_cut(v, s);
    if constexpr (has_part<SceneMeshNrmT, S>::value) bind_nrm(v, s);
    return s;
}

// ---- which form ----------------------------------------------------------------------------------------------------------------------
// The twelve render forms, in the order of tests/kernel_census.py's MESH_RENDER_KERNELS.
enum class MeshForm { nrm_cut_env, nrm_cut, nrm_env, nrm, cut_env, cut, env, light_tex, tex, light, smooth, flat };

// The form of a launch from which features are present (rpt_debug_kernel_choice's bits 26-31): normal maps and cutouts sit over the
// environment's form or the textured mesh-light one, the environment's one form holds every table below it, textures sit over the
// lights' tables or the smooth ones.
inline MeshForm mesh_form_of(bool smooth, bool lights, bool textured, bool environment, bool cutouts, bool normal_maps)
{
    if (normal_maps && cutouts) return environment ? MeshForm::nrm_cut_env : MeshForm::nrm_cut;
    if (normal_maps) return environment ? MeshForm::nrm_env : MeshForm::nrm;
    if (cutouts) return environment ? MeshForm::cut_env : MeshForm::cut;
    if (environment) return MeshForm::env;
    if (textured) return lights ? MeshForm::light_tex : MeshForm::tex;
    return lights ? MeshForm::light : smooth ? MeshForm::smooth : MeshForm::flat;
}

}  // namespace rptargs
