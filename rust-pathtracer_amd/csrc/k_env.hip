// k_env.hip — the device side of environment lighting (include/rpt.h, "environment lighting"): the kernels that make the
// environment's tables (host_env.h has their statement as plain functions this file compiles for the device, and the same table on the
// host, which the tests hold these kernels to), the mesh scenes' megakernel over a scene with an environment, and the probes of its
// lookup and its sampler.  Strict arithmetic, built like k_light.hip and k_tex.hip (-ffp-contract=off, the range tests next to every
// operation).
//
// The kernels are named meshenv_* and live in a code object library of their own (build.py, env_lib_of): the other libraries'
// censuses stay what they were.  ONE render kernel serves every mesh scene with an environment: SceneMeshEnv derives from
// SceneMeshLightTex, and a feature the scene does not use goes through empty tables (all-zero smooth bits, no ON mesh, tri_light and
// tri_tex all 0xFFFFFFFF), the way the textured forms already serve FLAT meshes.
//
// The table.  Weights are f32, everything after them is integer: the maximum is an atomicMax on the bits of non-negative floats, the
// quanta are uint64, their running sums are uint64.  Integer addition is associative, so the scan below — within 256 texels, then
// over the block sums, then the offsets — gives the bits of any other order.
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#define RPT_TEX_FN __host__ __device__ inline
#define RPT_ENV_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_env.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"

#include "regen_body.h"

using namespace rpthost;

// The weight pass, one lane per texel: the 12 B texel as given becomes the 16 B one, with w_k in its fourth word for the next pass
// (0 for a BACKGROUND_ONLY environment, which has no next pass); W_max by one atomicMax per workgroup on the bits (weights are >= 0).
__global__ __launch_bounds__(256) void meshenv_weight_kernel(const EnvTables t)
{
    __shared__ uint32_t s_max[256];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t bits = 0u;
    if (k < t.n_texels) {
        const float r = t.raw[3u * (size_t)k], g = t.raw[3u * (size_t)k + 1u], b = t.raw[3u * (size_t)k + 2u];
        const float w = t.sampled ? env_weight(r, g, b) : 0.0f;
        t.texels[k] = EnvTexel{r, g, b, w};
        bits = rpt_f2u(w);
    }
    if (!t.sampled) return;                                         // (uniform: no lane reaches the barriers below)
    s_max[threadIdx.x] = bits;
    __syncthreads();
    for (uint32_t step = 128u; step > 0u; step >>= 1) {
        if (threadIdx.x < step) { const uint32_t o = s_max[threadIdx.x + step]; if (o > s_max[threadIdx.x]) s_max[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0u && s_max[0] != 0u) atomicMax(t.w_max, s_max[0]);
}

// The quantise pass and the scan within a workgroup's 256 texels: cdf[k] = q of the workgroup's texels up to k, block[b] = their sum;
// the texel's fourth word becomes (float)q_k.
__global__ __launch_bounds__(256) void meshenv_quantise_kernel(const EnvTables t)
{
    __shared__ uint64_t s_sum[256];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const float w_max = rpt_u2f(*t.w_max);
    uint64_t q = 0;
    if (k < t.n_texels) {
        if (w_max > 0.0f) q = env_quantum(t.texels[k].q, env_exponent(w_max));
        t.texels[k].q = (float)q;
    }
    s_sum[threadIdx.x] = q;
    __syncthreads();
    for (uint32_t step = 1u; step < 256u; step <<= 1) {
        const uint64_t below = threadIdx.x >= step ? s_sum[threadIdx.x - step] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += below;
        __syncthreads();
    }
    if (k < t.n_texels) t.cdf[k] = s_sum[threadIdx.x];
    if (threadIdx.x == 255u) t.block[blockIdx.x] = s_sum[255];
}

// The scan of the block sums, in place, by one workgroup: 256 at a time, the carry in LDS — 4096 x 4096 texels make 65 536 block
// sums, 256 rounds.
__global__ __launch_bounds__(256) void meshenv_block_kernel(uint64_t* __restrict__ block, uint32_t n_blocks)
{
    __shared__ uint64_t s_sum[256];
    __shared__ uint64_t s_carry;
    if (threadIdx.x == 0u) s_carry = 0ull;
    __syncthreads();
    for (uint32_t base = 0u; base < n_blocks; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        s_sum[threadIdx.x] = i < n_blocks ? block[i] : 0ull;
        __syncthreads();
        for (uint32_t step = 1u; step < 256u; step <<= 1) {
            const uint64_t below = threadIdx.x >= step ? s_sum[threadIdx.x - step] : 0ull;
            __syncthreads();
            s_sum[threadIdx.x] += below;
            __syncthreads();
        }
        const uint64_t carry = s_carry;
        if (i < n_blocks) block[i] = carry + s_sum[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 255u) s_carry = carry + s_sum[255];
        __syncthreads();
    }
}

// The last pass, one lane per texel: C_k = the partial sum plus the sum of the blocks before its own.
__global__ __launch_bounds__(256) void meshenv_cdf_kernel(const EnvTables t)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= t.n_texels || blockIdx.x == 0u) return;
    t.cdf[k] += t.block[blockIdx.x - 1u];
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over a SceneMeshEnv: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshenv_regen_kernel(const SceneMeshEnv sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_env_query (include/rpt_test.h): the lookup the miss exit of the kernel above calls, one direction per lane.
__global__ __launch_bounds__(256) void meshenv_query_kernel(const SceneMeshEnv sc, const float* dirs, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    v3 radiance;
    float lp;
    const uint32_t k = mesh_env_lookup(sc, mk3(dirs[3u * i], dirs[3u * i + 1u], dirs[3u * i + 2u]), radiance, lp);
    uint32_t* o = out + 5u * i;
    o[0] = k;
    o[1] = rpt_f2u(radiance.x); o[2] = rpt_f2u(radiance.y); o[3] = rpt_f2u(radiance.z);
    o[4] = rpt_f2u(lp);
}

// rpt_debug_env_sample (include/rpt_test.h): the sampler the kernel above calls, one record per lane.
__global__ __launch_bounds__(256) void meshenv_sample_kernel(const SceneMeshEnv sc, const float* in, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* r = in + 7u * i;                                   // (scatter_pos, r[0 .. 2], does not enter: the light is at infinity)
    uint32_t* o = out + 8u * i;
    LightSample ls;
    const uint32_t k = mesh_env_sample(sc, r[3], r[4], r[5], r[6], ls);
    o[0] = k;
    o[1] = rpt_f2u(ls.direction.x); o[2] = rpt_f2u(ls.direction.y); o[3] = rpt_f2u(ls.direction.z);
    o[4] = rpt_f2u(ls.pdf);
    o[5] = rpt_f2u(ls.emission.x); o[6] = rpt_f2u(ls.emission.y); o[7] = rpt_f2u(ls.emission.z);
}

// (built into librpt_hip_env.so, build.py env_lib_of: the four launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t env_tables(const EnvTables& t, hipStream_t st)
{
    if (t.n_texels == 0u) return hipSuccess;
    const uint32_t n_blocks = (t.n_texels + 255u) / 256u;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshenv_weight_kernel, dim3(n_blocks), dim3(256), 0, st, t);
    if (t.sampled) {
        hipLaunchKernelGGL(meshenv_quantise_kernel, dim3(n_blocks), dim3(256), 0, st, t);
        hipLaunchKernelGGL(meshenv_block_kernel, dim3(1), dim3(256), 0, st, t.block, n_blocks);
        hipLaunchKernelGGL(meshenv_cdf_kernel, dim3(n_blocks), dim3(256), 0, st, t);
    }
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_env(const SceneMeshEnv& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshenv_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t env_query(const SceneMeshEnv& sc, const float* dirs, uint32_t* out, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshenv_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, dirs, out, n);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t env_sample(const SceneMeshEnv& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshenv_sample_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, in, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
