// k_smooth.hip — the device side of smooth mesh shading (include/rpt.h, "smooth mesh shading"): the two passes that keep the vertex
// normals of the SMOOTH meshes current (host_smooth.h has their statement as plain functions this file compiles for the device, and
// the same passes on the host, which the tests hold these kernels to), and the mesh scenes' megakernel over a scene whose winning
// triangle may take an interpolated normal.  Strict arithmetic, built like k_mesh.hip (-ffp-contract=off, the range tests next to
// every operation: build.py): a fused multiply-add in a cross product would change bits.
//
// The kernels are named meshsmooth_* and live in a code object library of their own (build.py, smooth_lib_of): the other libraries'
// censuses stay what they were, and k_mesh.hip is what it was.  The walks, the material and the emission are dev_scene_mesh.h's:
// SceneMeshSmooth derives from SceneMesh, and only hit_normal is overloaded for it (dev_mesh_smooth.h: k_light.hip's kernel shades
// with it too).
#include "kernel_common.h"

#include "dev_scene_mesh.h"

#define RPT_SMOOTH_FN __host__ __device__ inline
#include "host_smooth.h"
#include "launch_smooth.h"
#include "dev_mesh_smooth.h"

#include "regen_body.h"

using namespace rpthost;

// The face pass, one lane per face: host_smooth.h, smooth_face_vector.
__global__ __launch_bounds__(256) void meshsmooth_face_kernel(const float* __restrict__ vertices, const uint32_t* __restrict__ face_vertex,
                                                              float4* __restrict__ face, uint32_t n_faces)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n_faces) return;
    const float* pa = vertices + 3u * (size_t)face_vertex[f];
    const float* pb = vertices + 3u * (size_t)face_vertex[(size_t)n_faces + f];
    const float* pc = vertices + 3u * (size_t)face_vertex[2u * (size_t)n_faces + f];
    const float a[3] = {pa[0], pa[1], pa[2]}, b[3] = {pb[0], pb[1], pb[2]}, c[3] = {pc[0], pc[1], pc[2]};
    float g[3];
    smooth_face_vector(a, b, c, g);
    face[f] = make_float4(g[0], g[1], g[2], 0.0f);
}

// The vertex pass, one lane per vertex of the scene: host_smooth.h, smooth_vertex_normal — the vertex's faces in ascending order, the
// sum left to right, the guarded normalize.  A vertex of a FLAT mesh has no face and stores (0, 0, 0).
__global__ __launch_bounds__(256) void meshsmooth_vertex_kernel(const float4* __restrict__ face, const uint32_t* __restrict__ adj_first,
                                                                const uint32_t* __restrict__ adj, float4* __restrict__ normals, uint32_t n_vertices)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n_vertices) return;
    float n[3];
    smooth_vertex_normal(reinterpret_cast<const float*>(face), adj, adj_first[v], adj_first[v + 1u], n);
    normals[v] = make_float4(n[0], n[1], n[2], 0.0f);
}

#ifndef RPT_MESH_WAVES_PER_SIMD
#define RPT_MESH_WAVES_PER_SIMD 4
#endif
// mesh_regen_kernel (k_mesh.hip) over a SceneMeshSmooth: the same body, the same launch bounds.
__global__ __launch_bounds__(256, RPT_MESH_WAVES_PER_SIMD) void meshsmooth_regen_kernel(const SceneMeshSmooth sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }

// rpt_debug_mesh_normal_query (include/rpt_test.h): the closest walk, then the hit_normal the kernel above calls, one ray per lane.
__global__ __launch_bounds__(256) void meshsmooth_query_kernel(const SceneMeshSmooth sc, const float* rays, uint32_t* out, uint64_t n)
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

// (built into librpt_hip_smooth.so, build.py smooth_lib_of: the three launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t smooth_normals(const float* vertices, const uint32_t* face_vertex, float4* face, uint32_t n_faces,
                                                                 const uint32_t* adj_first, const uint32_t* adj, float4* normals, uint32_t n_vertices,
                                                                 hipStream_t st)
{
    (void)hipGetLastError();
    if (n_faces) hipLaunchKernelGGL(meshsmooth_face_kernel, dim3((n_faces + 255u) / 256u), dim3(256), 0, st, vertices, face_vertex, face, n_faces);
    if (n_vertices) hipLaunchKernelGGL(meshsmooth_vertex_kernel, dim3((n_vertices + 255u) / 256u), dim3(256), 0, st, face, adj_first, adj, normals, n_vertices);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t render_mesh_smooth(const SceneMeshSmooth& sc, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshsmooth_regen_kernel, dim3(nblocks), dim3(256), 0, st, sc, rp);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t mesh_normal_query(const SceneMeshSmooth& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags,
                                                                    hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SceneMeshSmooth s = sc;
    if (flags & 2u) s.use_bvh = 0u;                                // (RPT_MESH_QUERY_BRUTE)
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshsmooth_query_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, s, rays, out, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
