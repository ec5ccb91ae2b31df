// k_med.hip — the device side of mesh media (include/rpt.h, "mesh media"): the mesh scenes' megakernel over a scene some mesh of which
// bounds a medium — WithMedia<> over each of the eight emission-mapped forms — and the probe of the join: which medium a hit carries
// and which side of the boundary a direction lies on.  host_med.h has the tables as plain functions this file compiles for the
// device; the media arithmetic is dev_media.h's, reached through the media branches of dev_integrator.h.  Strict arithmetic, built
// like k_emap.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshmed_* and live in a code object library of their own (build.py, med_lib_of): the other libraries'
// censuses stay what they were.  Only hit_medium_index, medium_at and medium_side_normal are overloaded (dev_mesh_med.h).
//
// Two translation units of this one file, as k_emap.hip (build.py): RPT_MED_PART 0 holds the probe and the four forms over the forms
// without a normal map, RPT_MED_PART 1 the four forms over the normal-mapped ones.
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#define RPT_ENV_FN __host__ __device__ inline
#define RPT_CUT_FN __host__ __device__ inline
#define RPT_NRM_FN __host__ __device__ inline
#define RPT_MMAP_FN __host__ __device__ inline
#define RPT_EMAP_FN __host__ __device__ inline
#define RPT_MED_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_med.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"
#include "dev_mesh_mmap.h"
#include "dev_mesh_emap.h"
#include "dev_mesh_med.h"

#include "regen_body.h"

using namespace rpthost;

#ifndef RPT_MED_PART
#error "k_med.hip is built twice: -DRPT_MED_PART=0 and -DRPT_MED_PART=1 (build.py)"
#endif
// Waves per SIMD of the media forms: a macro of their own, so that it can differ from the other mesh forms' (DESIGN.md, 4d).
#ifndef RPT_MED_WAVES_PER_SIMD
#define RPT_MED_WAVES_PER_SIMD 4
#endif

// mesh_regen_kernel (k_mesh.hip) over one media scene: the same body; and its launch function.
#define RPT_MED_FORM(kernel, launcher, Scene)                                                                                                       \
    __global__ __launch_bounds__(256, RPT_MED_WAVES_PER_SIMD) void kernel(const Scene sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }  \
    namespace rptlaunch {                                                                                                                           \
    __attribute__((visibility("default"))) hipError_t launcher(const Scene& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)           \
    {                                                                                                                                               \
        (void)hipGetLastError();                                                                                                                    \
        hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);                                                                        \
        return hipGetLastError();                                                                                                                   \
    }                                                                                                                                               \
    }

#if RPT_MED_PART == 0

RPT_MED_FORM(meshmed_regen_kernel, render_mesh_med, SceneMeshMed)
RPT_MED_FORM(meshmed_env_regen_kernel, render_mesh_med_env, SceneMeshMedEnv)
RPT_MED_FORM(meshmed_cut_regen_kernel, render_mesh_med_cut, SceneMeshMedCut)
RPT_MED_FORM(meshmed_cut_env_regen_kernel, render_mesh_med_cut_env, SceneMeshMedCutEnv)

// rpt_debug_mesh_media_query (include/rpt_test.h): the closest walk, then the hit_medium_index, the medium_at and the
// medium_side_normal the kernels above call, one ray per lane.  The normal handed to medium_side_normal is the form's own hit_normal
// (bent on a SMOOTH mesh): what comes back must be G all the same.
__global__ __launch_bounds__(256) void meshmed_query_kernel(const SceneMeshMed sc, const float* rays, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;                                             // (no barrier below: the walks do not share their stacks)
    const float* r = rays + 9u * i;
    RayD ray;
    ray.o = mk3(r[0], r[1], r[2]);
    ray.d = mk3(r[3], r[4], r[5]);
    const v3 l = mk3(r[6], r[7], r[8]);
    float dist = 3.40282347e+38f;
    const uint32_t slot = mesh_closest(sc, ray, dist);
    uint32_t index = 0xFFFFFFFFu, ord = kNoMediumIdx, in_medium = 0u;
    float side = 0.0f;
    if (slot != kNoTriangle) {
        GeomHit g;
        g.code = sc.n_spheres + slot;
        index = tri_at(sc, slot).index;
        ord = hit_medium_index(sc, g);
        side = dot3(l, medium_side_normal(sc, g, hit_normal(sc, ray, dist, g)));
        if (ord != kNoMediumIdx) {
            if (medium_at(sc, ord).type != RPT_MEDIUM_NONE) in_medium = (side < 0.0f) ? 1u : 0u;
        }
    }
    uint32_t* o = out + 4u * i;
    o[0] = index;
    o[1] = ord;
    o[2] = rpt_f2u(side);
    o[3] = in_medium;
}

// (built into librpt_hip_med.so, build.py med_lib_of: the nine launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t mesh_media_query(const SceneMeshMed& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshMed s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshmed_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch

#else

RPT_MED_FORM(meshmed_nrm_regen_kernel, render_mesh_med_nrm, SceneMeshMedNrm)
RPT_MED_FORM(meshmed_nrm_env_regen_kernel, render_mesh_med_nrm_env, SceneMeshMedNrmEnv)
RPT_MED_FORM(meshmed_nrm_cut_regen_kernel, render_mesh_med_nrm_cut, SceneMeshMedNrmCut)
RPT_MED_FORM(meshmed_nrm_cut_env_regen_kernel, render_mesh_med_nrm_cut_env, SceneMeshMedNrmCutEnv)

#endif
