// launch_nrm.h — the seam between capi.hip and the kernels of mesh normal maps (k_nrm.hip, a code object library of its own:
// build.py, nrm_lib_of).  A header of its own beside launch_cut.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_nrm.h"
#include "launch_cut.h"

namespace rptscene {

// A mesh scene some mesh of which has a normal map ON (include/rpt.h, "mesh normal maps"): a textured form's tables — the mesh
// lights' ones (no mesh ON: tri_light all 0xFFFFFFFF, as the environment form does it), the environment form's, or either cutout
// form's — plus what the bend at a hit reads.
template <class Base> struct SceneMeshNrmT : Base {
    const rpthost::NrmDesc* nrm_desc;     // texture ordinal -> the mesh's map (flags 0: none)
    const float4* nrm_texels;             // every map's decoded texels {x, y, z, 0}, 16 B each
};
using SceneMeshNrm = SceneMeshNrmT<SceneMeshLightTex>;
using SceneMeshNrmEnv = SceneMeshNrmT<SceneMeshEnv>;
using SceneMeshNrmCut = SceneMeshNrmT<SceneMeshCut>;
using SceneMeshNrmCutEnv = SceneMeshNrmT<SceneMeshCutEnv>;

}  // namespace rptscene

namespace rptlaunch {

// One map: `bytes` (RGBA8, device) -> `out`, one lane per texel: {sx * c(R), sy * c(G), c(B), 0}.  One launch.
hipError_t nrm_decode(const uint8_t* bytes, rpthost::TexTexel* out, uint32_t n_texels, float sx, float sy, hipStream_t st);
// mesh_regen_kernel's body over the four normal-mapped forms
hipError_t render_mesh_nrm(const rptscene::SceneMeshNrm& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_nrm_env(const rptscene::SceneMeshNrmEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_nrm_cut(const rptscene::SceneMeshNrmCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_nrm_cut_env(const rptscene::SceneMeshNrmCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_normal_map_query (include/rpt_test.h): per ray {the winning triangle's flattened index or 0xFFFFFFFF, its normal's bits}
hipError_t mesh_normal_map_query(const rptscene::SceneMeshNrm& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
