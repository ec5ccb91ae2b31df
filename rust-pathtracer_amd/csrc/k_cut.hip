// k_cut.hip — the device side of mesh cutouts (include/rpt.h, "mesh cutouts"): the kernel that packs an A8 mask into bits (host_cut.h
// has its statement and the plain-loop reference the tests hold it to), the mesh scenes' megakernel over a scene whose walks reject a
// candidate where its mesh's mask has a hole — once over SceneMeshLightTex, once over SceneMeshEnv — and the probe of those walks.
// Strict arithmetic, built like k_tex.hip and k_env.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshcut_* and live in a code object library of their own (build.py, cut_lib_of): the other libraries'
// censuses stay what they were.  Normals, materials, emission, the samplers and the hit weights are the bases'; only closest_geom and
// any_hit are overloaded (dev_mesh_cut.h).
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#define RPT_ENV_FN __host__ __device__ inline
#define RPT_CUT_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_cut.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"

#include "regen_body.h"

using namespace rpthost;

// The mask, one lane per texel: its byte against the threshold, the wave's 64 answers by one ballot, two ordinary 4 B stores by the
// wave's first lane.  Texel k is bit k % 32 of word k / 32 whatever the launch shape; a wave that starts past the last texel stores
// nothing, and a mask's padding (host_cut.h, kCutPadTexels) keeps a wave's two words inside its own mask.
__global__ __launch_bounds__(256) void meshcut_mask_kernel(const uint8_t* __restrict__ alpha, uint32_t* __restrict__ words, uint32_t n_texels,
                                                           uint32_t threshold)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool opaque = k < n_texels && cut_opaque_byte(alpha[k], threshold);
    const uint64_t wave = __ballot(opaque);
    const uint32_t k0 = k & ~63u;                                   // the wave's first texel
    if ((threadIdx.x & 63u) == 0u && k0 < n_texels) {
        words[k0 >> 5] = (uint32_t)wave;
        words[(k0 >> 5) + 1u] = (uint32_t)(wave >> 32);
    }
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over the two cutout scenes: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshcut_regen_kernel(const SceneMeshCut sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshcut_env_regen_kernel(const SceneMeshCutEnv sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_cutout_query (include/rpt_test.h): the walks the kernels above run, one ray per lane.
__global__ __launch_bounds__(256) void meshcut_query_kernel(const SceneMeshCut sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;                                             // (no barrier below: the walks do not share their stacks)
    const float* r = rays + 7u * i;
    RayD ray;
    ray.o = mk3(r[0], r[1], r[2]);
    ray.d = mk3(r[3], r[4], r[5]);
    const float max_dist = r[6];
    float dist = 3.40282347e+38f;
    const uint32_t slot = mesh_closest_cut(sc, ray, dist);
    out[3u * i] = slot == kNoTriangle ? 0x7F800000u : rpt_f2u(dist);
    out[3u * i + 1u] = slot == kNoTriangle ? 0xFFFFFFFFu : tri_at(sc, slot).index;
    out[3u * i + 2u] = mesh_any_cut(sc, ray, (flags & 1u) != 0u, max_dist) ? 1u : 0u;      // (bit 0: RPT_MESH_QUERY_USE_MAX)
}

// (built into librpt_hip_cut.so, build.py cut_lib_of: the four launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t cut_mask(const uint8_t* alpha, uint32_t* words, uint32_t n_texels, uint32_t threshold, hipStream_t st)
{
    if (n_texels == 0u) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshcut_mask_kernel, dim3((n_texels + 255u) / 256u), dim3(256), 0, st, alpha, words, n_texels, threshold);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_cut(const SceneMeshCut& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshcut_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_cut_env(const SceneMeshCutEnv& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshcut_env_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_cutout_query(const SceneMeshCut& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                    hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshCut s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshcut_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n, flags);
    return hipGetLastError();
}

}  // namespace rptlaunch
