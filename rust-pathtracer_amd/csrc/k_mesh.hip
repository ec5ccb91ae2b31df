// k_mesh.hip — mesh scenes (include/rpt.h, "triangle meshes"): a large scene's tables plus triangles under a bounding volume
// hierarchy, in HBM (dev_scene_mesh.h).  The large scenes' megakernel body (regen_body.h) over SceneMesh; strict arithmetic only,
// built with the range tests next to every operation (kernel_common.h).  The kernels are named mesh_*: the render_* names are the
// other classes' census.
#include "kernel_common.h"

#include "dev_scene_mesh.h"
#include "regen_body.h"

// The walk's stack is 24 KiB of LDS per workgroup (dev_scene_mesh.h) on top of the body's tables; see DESIGN.md for the resources
// this build reports.
#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void mesh_regen_kernel(const SceneMesh sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_query (include/rpt_test.h): the walks the kernel above runs, one ray per lane.
__global__ __launch_bounds__(256) void mesh_query_kernel(const SceneMesh sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;                                             // (no barrier below: the walks do not share their stacks)
    const float* r = rays + 7u * i;
    RayD ray;
    ray.o = mk3(r[0], r[1], r[2]);
    ray.d = mk3(r[3], r[4], r[5]);
    const float max_dist = r[6];
    float dist = 3.40282347e+38f;
    const uint32_t slot = mesh_closest(sc, ray, dist);
    out[3u * i] = slot == kNoTriangle ? 0x7F800000u : rpt_f2u(dist);
    out[3u * i + 1u] = slot == kNoTriangle ? 0xFFFFFFFFu : tri_at(sc, slot).index;
    out[3u * i + 2u] = mesh_any(sc, ray, (flags & 1u) != 0u, max_dist) ? 1u : 0u;      // (bit 0: RPT_MESH_QUERY_USE_MAX)
}

// (built into librpt_hip_mesh.so, build.py mesh_lib_of: the two launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t render_mesh(const SceneMesh& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(mesh_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_query(const SceneMesh& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMesh s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(mesh_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n, flags);
    return hipGetLastError();
}

}  // namespace rptlaunch
