// k_tex.hip — the device side of mesh textures (include/rpt.h, "mesh textures"): the decode of an RGBA8 image into the f32 texels the
// lookup gathers (host_tex.h has its statement as plain functions this file compiles for the device, and the same decode on the host,
// which the tests hold these kernels to), the mesh scenes' megakernel over a scene whose winning triangle may take a textured base
// colour — once over SceneMeshSmooth, once over SceneMeshLight — and the probe of its hit_material.  Strict arithmetic, built like
// k_mesh.hip, k_smooth.hip and k_light.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshtex_* and live in a code object library of their own (build.py, tex_lib_of): the other libraries'
// censuses stay what they were.  The walks, the normals, the emission, the sampler of mesh lights and the hit weight are the bases';
// only hit_material is overloaded (dev_mesh_tex.h).
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_tex.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"

#include "regen_body.h"

using namespace rpthost;

// L[k], one lane per byte value: 254 rpt_powf per image, not one per texel.
__global__ __launch_bounds__(256) void meshtex_table_kernel(float* __restrict__ table, float gamma)
{
    table[threadIdx.x] = tex_decode_value(threadIdx.x, gamma);
}

// The decode, one lane per texel: the workgroup's copy of L in LDS, one 4 B load and one 16 B store per lane.
__global__ __launch_bounds__(256) void meshtex_decode_kernel(const uint32_t* __restrict__ bytes, const float* __restrict__ table,
                                                             TexTexel* __restrict__ out, uint32_t n_texels)
{
    __shared__ float s_l[256];
    s_l[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_texels) return;
    const uint32_t w = bytes[i];                                    // R, G, B, A from the low byte up
    out[i] = TexTexel{s_l[w & 255u], s_l[(w >> 8) & 255u], s_l[(w >> 16) & 255u], 0.0f};
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over the two textured scenes: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshtex_regen_kernel(const SceneMeshTex sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshtex_light_regen_kernel(const SceneMeshLightTex sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_texture_query (include/rpt_test.h): the closest walk, then the hit_material the kernels above call, one ray per lane.
__global__ __launch_bounds__(256) void meshtex_query_kernel(const SceneMeshTex sc, const float* rays, uint32_t* out, uint64_t n)
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
    v3 rgb = mk3(0.0f, 0.0f, 0.0f);
    if (slot != kNoTriangle) {
        GeomHit g;
        g.code = sc.n_spheres + slot;
        index = tri_at(sc, slot).index;
        Mat mat;
        hit_material(sc, ray, g, mat);
        rgb = mat.rgb;
    }
    out[4u * i] = index;
    out[4u * i + 1u] = rpt_f2u(rgb.x); out[4u * i + 2u] = rpt_f2u(rgb.y); out[4u * i + 3u] = rpt_f2u(rgb.z);
}

// (built into librpt_hip_tex.so, build.py tex_lib_of: the four launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t tex_decode(const uint8_t* bytes, float* table, TexTexel* out, uint32_t n_texels, float gamma, hipStream_t st)
{
    if (n_texels == 0u) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshtex_table_kernel, dim3(1), dim3(256), 0, st, table, gamma);
    hipLaunchKernelGGL(meshtex_decode_kernel, dim3((n_texels + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(bytes), table, out, n_texels);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_tex(const SceneMeshTex& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshtex_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_light_tex(const SceneMeshLightTex& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshtex_light_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_texture_query(const SceneMeshTex& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                     hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshTex s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshtex_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
