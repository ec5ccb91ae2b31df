// k_emap.hip — the device side of mesh emission maps (include/rpt.h, "mesh emission maps"): the mesh scenes' megakernel over a scene
// whose winning triangle, emitter exit and mesh-light sampler may take a looked-up emission — one form over each of the eight
// material-mapped forms — and the probes of its hit side and of its sampler.  host_emap.h has the statement as plain functions this
// file compiles for the device.  The decode is "mesh textures"' own launch (k_tex.hip): there is none here.  Strict arithmetic,
// built like k_mmap.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshemit_* and live in a code object library of their own (build.py, emap_lib_of): the other libraries'
// censuses stay what they were.  The walks, the normals, the sampler's pick, point and pdf and the hit weights are the bases'; only
// hit_material, hit_emission_at and mesh_light_nee are overloaded (dev_mesh_emap.h).
//
// Two translation units of this one file, as k_mmap.hip (build.py): RPT_EMAP_PART 0 holds the probes and the four forms over the
// forms without a normal map, RPT_EMAP_PART 1 the four forms over the normal-mapped ones.
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
#include "host_light.h"
#include "launch_emap.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"
#include "dev_mesh_mmap.h"
#include "dev_mesh_emap.h"

#include "regen_body.h"

using namespace rpthost;

#ifndef RPT_EMAP_PART
#error "k_emap.hip is built twice: -DRPT_EMAP_PART=0 and -DRPT_EMAP_PART=1 (build.py)"
#endif
#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif

// mesh_regen_kernel (k_mesh.hip) over one emission-mapped scene: the same body, the same launch bounds; and its launch function.
#define RPT_EMAP_FORM(kernel, launcher, Scene)                                                                                                       \
    __global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void kernel(const Scene sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }  \
    namespace rptlaunch {                                                                                                                            \
    __attribute__((visibility("default"))) hipError_t launcher(const Scene& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)            \
    {                                                                                                                                                \
        (void)hipGetLastError();                                                                                                                     \
        hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);                                                                         \
        return hipGetLastError();                                                                                                                    \
    }                                                                                                                                                \
    }

#if RPT_EMAP_PART == 0

RPT_EMAP_FORM(meshemit_regen_kernel, render_mesh_emit, SceneMeshEmit)
RPT_EMAP_FORM(meshemit_env_regen_kernel, render_mesh_emit_env, SceneMeshEmitEnv)
RPT_EMAP_FORM(meshemit_cut_regen_kernel, render_mesh_emit_cut, SceneMeshEmitCut)
RPT_EMAP_FORM(meshemit_cut_env_regen_kernel, render_mesh_emit_cut_env, SceneMeshEmitCutEnv)

// rpt_debug_mesh_emission_map_query (include/rpt_test.h): the closest walk, then the hit_material and the hit_emission_at the kernels
// above call, one ray per lane.
__global__ __launch_bounds__(256) void meshemit_query_kernel(const SceneMeshEmit sc, const float* rays, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;                                             // (no barrier below: the walks do not share their stacks)
    const float* r = rays + 7u * i;
    RayD ray;
    ray.o = mk3(r[0], r[1], r[2]);
    ray.d = mk3(r[3], r[4], r[5]);
    float dist = 3.40282347e+38f;
    const uint32_t slot = mesh_closest(sc, ray, dist);
    uint32_t index = 0xFFFFFFFFu;
    v3 em = mk3(0.0f, 0.0f, 0.0f), ex = mk3(0.0f, 0.0f, 0.0f);
    if (slot != kNoTriangle) {
        GeomHit g;
        g.code = sc.n_spheres + slot;
        index = tri_at(sc, slot).index;
        Mat mat;
        hit_material(sc, ray, g, mat);
        em = mat.emission;
        ex = hit_emission_at(sc, ray, g);
    }
    uint32_t* o = out + 7u * i;
    o[0] = index;
    o[1] = rpt_f2u(em.x); o[2] = rpt_f2u(em.y); o[3] = rpt_f2u(em.z);
    o[4] = rpt_f2u(ex.x); o[5] = rpt_f2u(ex.y); o[6] = rpt_f2u(ex.z);
}

// rpt_debug_mesh_emission_map_sample (include/rpt_test.h): the sampler mesh_light_nee above calls, one record per lane.
__global__ __launch_bounds__(256) void meshemit_sample_kernel(const SceneMeshEmit sc, const float* in, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* r = in + 8u * i;
    uint32_t* o = out + 8u * i;
    const uint32_t ord = rpt_f2u(r[7]);
    LightSample ls;
    ls.normal = mk3(0.0f, 0.0f, 0.0f); ls.emission = mk3(0.0f, 0.0f, 0.0f); ls.direction = mk3(0.0f, 0.0f, 0.0f);
    ls.dist = 0.0f; ls.pdf = 0.0f;
    uint32_t k = kNoMeshLight;
    float light_area;
    if (ord < sc.n_pick - sc.n_lights) k = mesh_light_sample_emit(sc, ord, mk3(r[0], r[1], r[2]), r[3], r[4], r[5], r[6], ls, light_area);
    o[0] = k;
    o[1] = rpt_f2u(ls.emission.x); o[2] = rpt_f2u(ls.emission.y); o[3] = rpt_f2u(ls.emission.z);
    o[4] = rpt_f2u(ls.direction.x); o[5] = rpt_f2u(ls.direction.y); o[6] = rpt_f2u(ls.direction.z);
    o[7] = rpt_f2u(ls.pdf);
}

// (built into librpt_hip_emap.so, build.py emap_lib_of: the ten launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t mesh_emission_map_query(const SceneMeshEmit& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                          hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshEmit s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshemit_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_emission_map_sample(const SceneMeshEmit& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshemit_sample_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, in, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch

#else

RPT_EMAP_FORM(meshemit_nrm_regen_kernel, render_mesh_emit_nrm, SceneMeshEmitNrm)
RPT_EMAP_FORM(meshemit_nrm_env_regen_kernel, render_mesh_emit_nrm_env, SceneMeshEmitNrmEnv)
RPT_EMAP_FORM(meshemit_nrm_cut_regen_kernel, render_mesh_emit_nrm_cut, SceneMeshEmitNrmCut)
RPT_EMAP_FORM(meshemit_nrm_cut_env_regen_kernel, render_mesh_emit_nrm_cut_env, SceneMeshEmitNrmCutEnv)

#endif
