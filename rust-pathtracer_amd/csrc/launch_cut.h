// launch_cut.h — the seam between capi.hip and the kernels of mesh cutouts (k_cut.hip, a code object library of its own: build.py,
// cut_lib_of).  A header of its own beside launch_env.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_cut.h"
#include "launch_env.h"

namespace rptscene {

// A mesh scene some mesh of which has a cutout ON (include/rpt.h, "mesh cutouts"): a textured form's tables — the mesh lights' ones
// (no mesh ON: tri_light all 0xFFFFFFFF, as the environment form does it) or the environment form's — plus what the cut test reads.
template <class Base> struct SceneMeshCutT : Base {
    const rpthost::CutDesc* cut_desc;     // texture ordinal -> the mesh's cutout (flags 0: none)
    const uint32_t* cut_bits;             // every mask's words
};
using SceneMeshCut = SceneMeshCutT<SceneMeshLightTex>;
using SceneMeshCutEnv = SceneMeshCutT<SceneMeshEnv>;

}  // namespace rptscene

namespace rptlaunch {

// One mask: `alpha` (one byte per texel, device) -> its bits in `words` (cut_mask_words(width, height) of them, ZERO before: the
// padding is not written).  One launch.
hipError_t cut_mask(const uint8_t* alpha, uint32_t* words, uint32_t n_texels, uint32_t threshold, hipStream_t st);
// mesh_regen_kernel's body over a SceneMeshCut / a SceneMeshCutEnv
hipError_t render_mesh_cut(const rptscene::SceneMeshCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_cut_env(const rptscene::SceneMeshCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_cutout_query (include/rpt_test.h): per ray {t's bits or +inf's, the winning flattened index or 0xFFFFFFFF, any_hit}
hipError_t mesh_cutout_query(const rptscene::SceneMeshCut& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
