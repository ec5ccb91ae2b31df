// launch_env.h — the seam between capi.hip and the kernels of environment lighting (k_env.hip, a code object library of its own:
// build.py, env_lib_of).  A header of its own beside launch_tex.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_env.h"
#include "launch_tex.h"

namespace rptscene {

// What the table kernels read and write, on one device (host_env.h, EnvLayout).
struct EnvTables {
    const float* raw;                 // the image as given: 3 f32 per texel (staging, freed after the call)
    rpthost::EnvTexel* texels;        // per texel {r, g, b, w_k and then (float)q_k}
    uint64_t* cdf;                    // per texel: the scan's partial sums, then C_k (SAMPLED only)
    uint64_t* block;                  // per 256 texels: the scan's block sums (scratch)
    uint32_t* w_max;                  // the bits of W_max (scratch)
    uint32_t n_texels;
    uint32_t sampled;
};

// A mesh scene with an environment (include/rpt.h, "environment lighting"): the base form's tables — a feature the scene does not
// use goes through empty tables: all-zero smooth bits, tri_light and tri_tex all 0xFFFFFFFF, no ON mesh — plus what the miss and
// the sampler read.  n_pick and n_lights_f count the environment while it is SAMPLED.
template <class Base> struct SceneMeshEnvT : Base {
    const rpthost::EnvTexel* env_texels;
    const uint64_t* env_cdf;          // C_k (SAMPLED and not dark, else not read)
    uint64_t env_q;                   // Q; 0: BACKGROUND_ONLY, or the table is dark
    float env_q_f;                    // Q rounded to f32
    float env_scale;
    uint32_t env_size;
    uint32_t env_pick;                // the environment's index among the pickable lights (the last one), or 0xFFFFFFFF: not SAMPLED
};
using SceneMeshEnv = SceneMeshEnvT<SceneMeshLightTex>;

}  // namespace rptscene

namespace rptlaunch {

// The environment's tables from t.raw: texels and weights with their maximum, then (SAMPLED) quantise and scan within 256 texels,
// scan the block sums, CDF.  One launch or four, whatever the size.  t.w_max must be zero before.
hipError_t env_tables(const rptscene::EnvTables& t, hipStream_t st);
// mesh_regen_kernel's body over a SceneMeshEnv
hipError_t render_mesh_env(const rptscene::SceneMeshEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_env_query / rpt_debug_env_sample (include/rpt_test.h)
hipError_t env_query(const rptscene::SceneMeshEnv& sc, const float* dirs, uint32_t* out, uint64_t n, hipStream_t st);
hipError_t env_sample(const rptscene::SceneMeshEnv& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st);

}  // namespace rptlaunch
