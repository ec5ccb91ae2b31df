// k_mmap.hip — the device side of mesh material maps (include/rpt.h, "mesh material maps"): the decode of an RGBA8 map into the
// f32 factors the hit gathers (host_mmap.h has its statement as plain functions this file compiles for the device, and the
// plain-loop reference the tests hold it to), the mesh scenes' megakernel over a scene whose winning triangle may take a scaled
// roughness and metallic — over the eight textured forms that hold every table — and the probe of its hit_material.  Strict
// arithmetic, built like k_nrm.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshmap_* and live in a code object library of their own (build.py, mmap_lib_of): the other libraries'
// censuses stay what they were.  The walks, the normals, the emission, the samplers and the hit weights are the bases'; only
// hit_material is overloaded (dev_mesh_mmap.h).
//
// Two translation units of this one file, to halve the build's longest step (build.py): RPT_MMAP_PART 0 holds the decode, the
// probe and the four forms over the forms without a normal map, RPT_MMAP_PART 1 the four forms over the normal-mapped ones.
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#define RPT_ENV_FN __host__ __device__ inline
#define RPT_CUT_FN __host__ __device__ inline
#define RPT_NRM_FN __host__ __device__ inline
#define RPT_MMAP_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_mmap.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"
#include "dev_mesh_mmap.h"

#include "regen_body.h"

using namespace rpthost;

#ifndef RPT_MMAP_PART
#error "k_mmap.hip is built twice: -DRPT_MMAP_PART=0 and -DRPT_MMAP_PART=1 (build.py)"
#endif
#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif

// mesh_regen_kernel (k_mesh.hip) over one material-mapped scene: the same body, the same launch bounds; and its launch function.
#define RPT_MMAP_FORM(kernel, launcher, Scene)                                                                                                       \
    __global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void kernel(const Scene sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }  \
    namespace rptlaunch {                                                                                                                            \
    __attribute__((visibility("default"))) hipError_t launcher(const Scene& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)            \
    {                                                                                                                                                \
        (void)hipGetLastError();                                                                                                                     \
        hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);                                                                         \
        return hipGetLastError();                                                                                                                    \
    }                                                                                                                                                \
    }

#if RPT_MMAP_PART == 0

// The decode, one lane per texel: one 4 B load, at most two divides, one 16 B store.
__global__ __launch_bounds__(256) void meshmap_decode_kernel(const uint32_t* __restrict__ bytes, TexTexel* __restrict__ out, uint32_t n_texels,
                                                             uint32_t roughness_channel, uint32_t metallic_channel)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_texels) return;
    out[i] = mmap_decode_texel(bytes[i], roughness_channel, metallic_channel);     // R, G, B, A from the low byte up
}

RPT_MMAP_FORM(meshmap_regen_kernel, render_mesh_map, SceneMeshMap)
RPT_MMAP_FORM(meshmap_env_regen_kernel, render_mesh_map_env, SceneMeshMapEnv)
RPT_MMAP_FORM(meshmap_cut_regen_kernel, render_mesh_map_cut, SceneMeshMapCut)
RPT_MMAP_FORM(meshmap_cut_env_regen_kernel, render_mesh_map_cut_env, SceneMeshMapCutEnv)

// rpt_debug_mesh_material_map_query (include/rpt_test.h): the closest walk, then the hit_material the kernels above call, one ray per lane.
__global__ __launch_bounds__(256) void meshmap_query_kernel(const SceneMeshMap sc, const float* rays, uint32_t* out, uint64_t n)
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
    float roughness = 0.0f, metallic = 0.0f;
    if (slot != kNoTriangle) {
        GeomHit g;
        g.code = sc.n_spheres + slot;
        index = tri_at(sc, slot).index;
        Mat mat;
        hit_material(sc, ray, g, mat);
        roughness = mat.roughness; metallic = mat.metallic;
    }
    out[4u * i] = index;
    out[4u * i + 1u] = rpt_f2u(roughness); out[4u * i + 2u] = rpt_f2u(metallic); out[4u * i + 3u] = 0u;
}

// (built into librpt_hip_mmap.so, build.py mmap_lib_of: the ten launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t mmap_decode(const uint8_t* bytes, TexTexel* out, uint32_t n_texels, uint32_t roughness_channel,
                                                              uint32_t metallic_channel, hipStream_t st)
{
    if (n_texels == 0u) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshmap_decode_kernel, dim3((n_texels + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(bytes), out, n_texels,
                       roughness_channel, metallic_channel);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_material_map_query(const SceneMeshMap& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                          hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshMap s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshmap_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch

#else

RPT_MMAP_FORM(meshmap_nrm_regen_kernel, render_mesh_map_nrm, SceneMeshMapNrm)
RPT_MMAP_FORM(meshmap_nrm_env_regen_kernel, render_mesh_map_nrm_env, SceneMeshMapNrmEnv)
RPT_MMAP_FORM(meshmap_nrm_cut_regen_kernel, render_mesh_map_nrm_cut, SceneMeshMapNrmCut)
RPT_MMAP_FORM(meshmap_nrm_cut_env_regen_kernel, render_mesh_map_nrm_cut_env, SceneMeshMapNrmCutEnv)

#endif
