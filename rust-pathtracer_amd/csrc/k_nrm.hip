// k_nrm.hip — the device side of mesh normal maps (include/rpt.h, "mesh normal maps"): the decode of an RGBA8 map into the f32
// texels the bend gathers (host_nrm.h has its statement as plain functions this file compiles for the device, and the plain-loop
// reference the tests hold it to), the mesh scenes' megakernel over a scene whose winning triangle may take a bent normal — over
// SceneMeshLightTex, SceneMeshEnv, SceneMeshCut and SceneMeshCutEnv — and the probe of its hit_normal.  Strict arithmetic, built like
// k_tex.hip and k_cut.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshnrm_* and live in a code object library of their own (build.py, nrm_lib_of): the other libraries'
// censuses stay what they were.  The walks, the materials, the emission, the samplers and the hit weights are the bases'; only
// hit_normal is overloaded (dev_mesh_nrm.h).
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#define RPT_ENV_FN __host__ __device__ inline
#define RPT_CUT_FN __host__ __device__ inline
#define RPT_NRM_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_nrm.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"

#include "regen_body.h"

using namespace rpthost;

// The decode, one lane per texel: one 4 B load, three divides, one 16 B store.
__global__ __launch_bounds__(256) void meshnrm_decode_kernel(const uint32_t* __restrict__ bytes, TexTexel* __restrict__ out, uint32_t n_texels, float sx,
                                                             float sy)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_texels) return;
    out[i] = nrm_decode_texel(bytes[i], sx, sy);                    // R, G, B, A from the low byte up
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over the four normal-mapped scenes: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshnrm_regen_kernel(const SceneMeshNrm sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshnrm_env_regen_kernel(const SceneMeshNrmEnv sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshnrm_cut_regen_kernel(const SceneMeshNrmCut sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshnrm_cut_env_regen_kernel(const SceneMeshNrmCutEnv sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_normal_map_query (include/rpt_test.h): the closest walk, then the hit_normal the kernels above call, one ray per lane.
__global__ __launch_bounds__(256) void meshnrm_query_kernel(const SceneMeshNrm sc, const float* rays, uint32_t* out, uint64_t n)
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
    v3 nrm = mk3(0.0f, 0.0f, 0.0f);
    if (slot != kNoTriangle) {
        GeomHit g;
        g.code = sc.n_spheres + slot;
        index = tri_at(sc, slot).index;
        nrm = hit_normal(sc, ray, dist, g);
    }
    out[4u * i] = index;
    out[4u * i + 1u] = rpt_f2u(nrm.x); out[4u * i + 2u] = rpt_f2u(nrm.y); out[4u * i + 3u] = rpt_f2u(nrm.z);
}

// (built into librpt_hip_nrm.so, build.py nrm_lib_of: the six launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t nrm_decode(const uint8_t* bytes, TexTexel* out, uint32_t n_texels, float sx, float sy, hipStream_t st)
{
    if (n_texels == 0u) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_decode_kernel, dim3((n_texels + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(bytes), out, n_texels, sx, sy);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_nrm(const SceneMeshNrm& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_nrm_env(const SceneMeshNrmEnv& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_env_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_nrm_cut(const SceneMeshNrmCut& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_cut_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_nrm_cut_env(const SceneMeshNrmCutEnv& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_cut_env_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_normal_map_query(const SceneMeshNrm& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                        hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshNrm s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshnrm_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
