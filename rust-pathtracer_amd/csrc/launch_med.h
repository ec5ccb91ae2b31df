// launch_med.h — the seam between capi.hip and the kernels of mesh media (k_med.hip, a code object library of its own: build.py,
// med_lib_of).  A header of its own beside launch_emap.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_med.h"
#include "launch_emap.h"

namespace rptscene {

// A mesh scene some mesh of which carries a medium (include/rpt.h, "mesh media"): WithMedia<> over any of the eight emission-mapped
// forms — the path functions carry the medium a path is in — plus the two tables the media overloads read.
template <class Base> struct SceneMeshMedT : WithMedia<Base> {
    const rpthost::MedRow* med_rows;            // medium ordinal -> its row
    const uint32_t* tri_medium;                 // flattened triangle index -> its mesh's medium ordinal, or rpthost::kMedNone
};
using SceneMeshMed = SceneMeshMedT<SceneMeshEmit>;
using SceneMeshMedEnv = SceneMeshMedT<SceneMeshEmitEnv>;
using SceneMeshMedCut = SceneMeshMedT<SceneMeshEmitCut>;
using SceneMeshMedCutEnv = SceneMeshMedT<SceneMeshEmitCutEnv>;
using SceneMeshMedNrm = SceneMeshMedT<SceneMeshEmitNrm>;
using SceneMeshMedNrmEnv = SceneMeshMedT<SceneMeshEmitNrmEnv>;
using SceneMeshMedNrmCut = SceneMeshMedT<SceneMeshEmitNrmCut>;
using SceneMeshMedNrmCutEnv = SceneMeshMedT<SceneMeshEmitNrmCutEnv>;

}  // namespace rptscene

namespace rptlaunch {

// mesh_regen_kernel's body over the eight media forms.
hipError_t render_mesh_med(const rptscene::SceneMeshMed& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_env(const rptscene::SceneMeshMedEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_cut(const rptscene::SceneMeshMedCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_cut_env(const rptscene::SceneMeshMedCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_nrm(const rptscene::SceneMeshMedNrm& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_nrm_env(const rptscene::SceneMeshMedNrmEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_nrm_cut(const rptscene::SceneMeshMedNrmCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_med_nrm_cut_env(const rptscene::SceneMeshMedNrmCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_media_query (include/rpt_test.h): per ray {o, d, l} -> {the winning triangle's flattened index or 0xFFFFFFFF, its
// medium ordinal or rpthost::kMedNone, the bits of dot(l, G), in_medium after step 4 started from false}
hipError_t mesh_media_query(const rptscene::SceneMeshMed& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
