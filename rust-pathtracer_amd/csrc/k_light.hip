// k_light.hip — the device side of mesh lights (include/rpt.h, "mesh lights"): the kernels that keep the table of every ON mesh
// current (host_light.h has their statement as plain functions this file compiles for the device, and the same table on the host,
// which the tests hold these kernels to), the mesh scenes' megakernel over a scene whose lights include meshes, and the probe of its
// sampler.  Strict arithmetic, built like k_mesh.hip and k_smooth.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named meshlight_* and live in a code object library of their own (build.py, light_lib_of).  One render kernel
// serves FLAT and SMOOTH meshes alike: SceneMeshLight derives from SceneMeshSmooth, whose hit_normal reads one bit per triangle
// (dev_mesh_smooth.h); while no mesh is SMOOTH those bits are all zero.
//
// The table.  Areas are f32, everything after them is integer: the maximum is an atomicMax on the bits of non-negative floats, the
// quanta are uint64, their running sums are uint64.  Integer addition is associative, so the scan below — within 256 faces, then
// over the block sums, then the offsets — gives the bits of any other order.  The scan runs over the faces of ALL ON meshes at
// once (below 2^63: fewer than 2^27 faces of fewer than 2^36 each) and a mesh's C_k is the running sum less the sum before the
// mesh's first face.
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#define RPT_LIGHT_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_light.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"

#include "regen_body.h"

using namespace rpthost;

// One lane per ON mesh: the mesh is dark until the last pass says otherwise.
__global__ __launch_bounds__(256) void meshlight_reset_kernel(LightMeshDesc* __restrict__ desc, uint32_t n_on)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_on) return;
    desc[j].area = 0.0f;
    desc[j].exponent = 0;
    desc[j].a_max = 0u;
}

// The area pass, one lane per face: host_light.h, light_tri_area; its mesh's A_max by atomicMax on the bits (areas are >= 0).
__global__ __launch_bounds__(256) void meshlight_area_kernel(const float* __restrict__ vertices, const LightTables t)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= t.n_faces) return;
    const float* pa = vertices + 3u * (size_t)t.face_vertex[f];
    const float* pb = vertices + 3u * (size_t)t.face_vertex[(size_t)t.n_faces + f];
    const float* pc = vertices + 3u * (size_t)t.face_vertex[2u * (size_t)t.n_faces + f];
    const float a[3] = {pa[0], pa[1], pa[2]}, b[3] = {pb[0], pb[1], pb[2]}, c[3] = {pc[0], pc[1], pc[2]};
    const float area = light_tri_area(a, b, c);
    t.area[f] = area;
    const uint32_t bits = rpt_f2u(area);
    if (bits != 0u) atomicMax(&t.desc[t.face_mesh[f]].a_max, bits);
}

// The quantise pass and the scan within a workgroup's 256 faces: part[f] = q of the workgroup's faces up to f, block[b] = their sum.
__global__ __launch_bounds__(256) void meshlight_quantise_kernel(const LightTables t)
{
    __shared__ uint64_t s_sum[256];
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    uint64_t q = 0;
    if (f < t.n_faces) q = light_quantum(t.area[f], light_exponent(rpt_u2f(t.desc[t.face_mesh[f]].a_max)));
    s_sum[threadIdx.x] = q;
    __syncthreads();
    for (uint32_t step = 1u; step < 256u; step <<= 1) {
        const uint64_t below = threadIdx.x >= step ? s_sum[threadIdx.x - step] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += below;
        __syncthreads();
    }
    if (f < t.n_faces) t.part[f] = s_sum[threadIdx.x];
    if (threadIdx.x == 255u) t.block[blockIdx.x] = s_sum[255];
}

// The scan of the block sums, in place, by one workgroup: 256 at a time, the carry in LDS.
__global__ __launch_bounds__(256) void meshlight_block_kernel(uint64_t* __restrict__ block, uint32_t n_blocks)
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

// The running sum over all faces up to and including face i.
__device__ inline uint64_t meshlight_sum_to(const LightTables& t, uint32_t i)
{
    const uint32_t b = i / 256u;
    return t.part[i] + (b ? t.block[b - 1u] : 0ull);
}

// The last pass, one lane per face: C_k, and by the lane of a mesh's first face E and A_tot.  Every lane works out its own mesh's Q
// (two more reads): a mesh whose A_tot is not finite is dark, and then all its C_k are 0.
__global__ __launch_bounds__(256) void meshlight_cdf_kernel(const LightTables t)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= t.n_faces) return;
    LightMeshDesc* d = t.desc + t.face_mesh[f];
    const uint32_t first = d->first, n = d->n;
    const float a_max = rpt_u2f(d->a_max);
    const uint64_t before = first ? meshlight_sum_to(t, first - 1u) : 0ull;
    const uint64_t q_all = meshlight_sum_to(t, first + n - 1u) - before;
    const int32_t e = light_exponent(a_max);
    const float a_tot = light_total_area(q_all, e);
    const bool dark = !(a_max > 0.0f) || !(a_tot <= kSmoothFMax);
    t.cdf[f] = dark ? 0ull : meshlight_sum_to(t, f) - before;
    if (f == first) {
        d->area = dark ? 0.0f : a_tot;
        d->exponent = dark ? 0 : e;
    }
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over a SceneMeshLight: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshlight_regen_kernel(const SceneMeshLight sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_light_sample (include/rpt_test.h): the sampler the kernel above calls, one record per lane.
__global__ __launch_bounds__(256) void meshlight_sample_kernel(const SceneMeshLight sc, const float* in, uint32_t* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* r = in + 8u * i;
    uint32_t* o = out + 9u * i;
    const uint32_t ord = rpt_f2u(r[7]);
    LightSample ls;
    ls.normal = mk3(0.0f, 0.0f, 0.0f); ls.emission = mk3(0.0f, 0.0f, 0.0f); ls.direction = mk3(0.0f, 0.0f, 0.0f);
    ls.dist = 0.0f; ls.pdf = 0.0f;
    uint32_t k = kNoMeshLight;
    float light_area;
    if (ord < sc.n_pick - sc.n_lights) k = mesh_light_sample(sc, ord, mk3(r[0], r[1], r[2]), r[3], r[4], r[5], r[6], ls, light_area);
    o[0] = k;
    o[1] = rpt_f2u(ls.direction.x); o[2] = rpt_f2u(ls.direction.y); o[3] = rpt_f2u(ls.direction.z);
    o[4] = rpt_f2u(ls.normal.x); o[5] = rpt_f2u(ls.normal.y); o[6] = rpt_f2u(ls.normal.z);
    o[7] = rpt_f2u(ls.dist);
    o[8] = rpt_f2u(ls.pdf);
}

// (built into librpt_hip_light.so, build.py light_lib_of: the three launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t light_tables(const float* vertices, const LightTables& t, hipStream_t st)
{
    (void)hipGetLastError();
    if (t.n_on) hipLaunchKernelGGL(meshlight_reset_kernel, dim3((t.n_on + 255u) / 256u), dim3(256), 0, st, t.desc, t.n_on);
    if (t.n_faces) {
        const uint32_t n_blocks = (t.n_faces + 255u) / 256u;
        hipLaunchKernelGGL(meshlight_area_kernel, dim3(n_blocks), dim3(256), 0, st, vertices, t);
        hipLaunchKernelGGL(meshlight_quantise_kernel, dim3(n_blocks), dim3(256), 0, st, t);
        hipLaunchKernelGGL(meshlight_block_kernel, dim3(1), dim3(256), 0, st, t.block, n_blocks);
        hipLaunchKernelGGL(meshlight_cdf_kernel, dim3(n_blocks), dim3(256), 0, st, t);
    }
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_light(const SceneMeshLight& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshlight_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_light_sample(const SceneMeshLight& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshlight_sample_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, in, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
