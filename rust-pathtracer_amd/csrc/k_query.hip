// k_query.hip — the device side of ray queries (include/rpt.h, "ray queries"): the closest hit, occlusion and the surface at the hit
// for rays the caller brings, and the camera's rays.  One ray per lane, 256-lane workgroups (the walks' LDS stack: dev_scene_mesh.h),
// no path state, no random numbers.  Strict arithmetic, built like k_med.hip (-ffp-contract=off, the range tests next to every
// operation).
//
// The kernels are named query_* and live in a code object library of their own (build.py, query_lib_of): the other libraries'
// censuses stay what they were.  The device functions are the render forms': the sphere and plane tests and the walks of
// closest_geom, any_hit, hit_normal, hit_material, hit_emission_at, camera_ray and pixel_coords.  closest_geom itself ends in
// Scene::sample_lights and writes its distance into a PathState; query_geom below is its geometry pass alone — the same calls in
// the same order — handing the distance out instead.
//
// Nine kernels.  Geometry-only traces and occlusion carry no surface code: closest and occluded, each without and with the cut
// test in its walk.  The surface kernels exist per combination that changes a function's body — normal map x cutout — over
// SceneMeshEmit, the form that holds the smooth, light, texture, material-map and emission-map tables; a feature that is absent is
// reached through the empty tables of the query's own allocation (host_query.h, mesh_args_query.h).  And the camera's rays.
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
#define RPT_QUERY_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_query.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"
#include "dev_mesh_mmap.h"
#include "dev_mesh_emap.h"

using namespace rpthost;

// Workgroups per CU the kernels are compiled for: the LDS stack (24 KiB of 160) allows six, and the register counts the build
// reports ("ray queries") stay below the 80 that six workgroups of four waves leave each lane.
#ifndef RPT_QUERY_WAVES_PER_SIMD
#define RPT_QUERY_WAVES_PER_SIMD 6
#endif

namespace {

constexpr float kQueryFar = 3.40282347e+38f;                        // F::MAX: where closest_geom starts
constexpr uint32_t kQueryInfBits = 0x7F800000u;

struct QueryRay {
    RayD ray;
    float max_dist;
};

// rpt_ray as two 16-byte loads
RPT_DEV QueryRay query_load(const rpt_ray* rays, uint64_t i)
{
    const float4* r = reinterpret_cast<const float4*>(rays + i);
    const float4 a = r[0], b = r[1];
    QueryRay q;
    q.ray.o = mk3(a.x, a.y, a.z);
    q.ray.d = mk3(b.x, b.y, b.z);
    q.max_dist = a.w;
    return q;
}

// The geometry pass of closest_geom (dev_scene_mesh.h; dev_mesh_cut.h for CUT): spheres, planes, the walk.  True when something was
// accepted: `dist` its distance, g.code the integrator's code, `slot` the winning triangle's slot or kNoTriangle.
template <bool CUT, class S> RPT_DEV bool query_geom(const S& sc, const RayD& ray, float& dist, GeomHit& g, uint32_t& slot)
{
    dist = kQueryFar;
    bool hit = false;
    uint32_t best = 0xFFFFFFFFu;                                    // nearest sphere so far
    if (sc.use_accel) grid_closest_sphere(sc, ray, dist, best, hit);
    else brute_closest_sphere(sc, ray, dist, best, hit);
    uint32_t accepted_planes = 0;
    for (uint32_t k = 0; k < sc.n_planes; ++k) {                    // as closest_geom_finish
        const DevPlane& p = sc.planes[k];
        float t;
        bool h = hit_plane(ray, p, t);
        bool acc = h && ((sc.n_spheres == 0 && k == 0) || t < dist);
        if (acc) {
            dist = t;
            hit = true;
            accepted_planes |= 1u << k;
        }
    }
    uint32_t code = (best == 0xFFFFFFFFu ? kNoSphere : best) | (accepted_planes << 28);
    if constexpr (CUT) slot = mesh_closest_cut(sc, ray, dist);
    else slot = mesh_closest(sc, ray, dist);
    if (slot != kNoTriangle) { hit = true; code = sc.n_spheres + slot; }
    g.code = code;
    return hit;
}

// The winner of a hit as rpt_hit names it (include/rpt.h): the triangle, else the last accepted plane, else the nearest sphere.
struct QueryWinner {
    uint32_t kind, primitive, material;
};

template <class S> RPT_DEV QueryWinner query_winner(const S& sc, const GeomHit& g, uint32_t slot, const TriRec& tri, bool with_material)
{
    QueryWinner w;
    const uint32_t accepted_planes = g.code >> 28;
    if (slot != kNoTriangle) {
        w.kind = RPT_HIT_TRIANGLE; w.primitive = tri.index; w.material = tri.material;
    } else if (accepted_planes != 0u) {
        w.kind = RPT_HIT_PLANE; w.primitive = 31u - (uint32_t)__builtin_clz(accepted_planes);
        w.material = sc.planes[w.primitive].material;
    } else {
        w.kind = RPT_HIT_SPHERE; w.primitive = g.code & kNoSphere;
        w.material = with_material ? gather32(sc.sphere_material, w.primitive) : 0u;
    }
    return w;
}

// One ray's closest query: rpt_hit as two 16-byte stores, and, for a surface kernel, rpt_surface as four.
template <bool CUT, bool SURFACE, class S> RPT_DEV void query_trace(const S& sc, const QueryArgs& q)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= q.n) return;                                           // (no barrier below: the walks do not share their stacks)
    const QueryRay qr = query_load(q.rays, i);
    float dist;
    GeomHit g;
    uint32_t slot;
    const bool hit = query_geom<CUT>(sc, qr.ray, dist, g, slot);
    uint4 h0 = make_uint4(kQueryInfBits, RPT_HIT_NONE, 0xFFFFFFFFu, 0xFFFFFFFFu), h1 = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
    float4 s0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s1 = s0, s2 = s0, s3 = s0;
    if (hit) {
        TriRec tri;
        tri.index = 0u; tri.material = 0u;
        float u = 0.0f, v = 0.0f;
        uint32_t mesh = 0xFFFFFFFFu, within = 0xFFFFFFFFu;
        if (slot != kNoTriangle) {
            tri = tri_at(sc, slot);
            // the triangle test's u and v (hit_triangle, dev_scene_mesh.h): the same operations on the same words
            const v3 p = cross3(qr.ray.d, tri.e2);
            const float det = dot3(tri.e1, p);
            const float inv = fdiv(1.0f, det);
            const v3 s = qr.ray.o - tri.a;
            u = dot3(s, p) * inv;
            const v3 qq = cross3(s, tri.e1);
            v = dot3(qr.ray.d, qq) * inv;
            mesh = query_mesh_of(q.tri_first, q.n_meshes, tri.index);
            if (mesh != kQueryNone) within = tri.index - q.tri_first[mesh];
        }
        const QueryWinner w = query_winner(sc, g, slot, tri, SURFACE);
        h0 = make_uint4(rpt_f2u(dist), w.kind, w.primitive, mesh);
        h1 = make_uint4(within, rpt_f2u(u), rpt_f2u(v), 0u);
        if constexpr (SURFACE) {
            const v3 ns = hit_normal(sc, qr.ray, dist, g);
            const v3 ng = slot != kNoTriangle ? norm3(cross3(tri.e1, tri.e2)) : normal_large(sc, qr.ray, dist, g);
            Mat mat;
            hit_material(sc, qr.ray, g, mat);
            const v3 em = hit_emission_at(sc, qr.ray, g);
            s0 = make_float4(ng.x, ng.y, ng.z, ns.x);
            s1 = make_float4(ns.y, ns.z, mat.rgb.x, mat.rgb.y);
            s2 = make_float4(mat.rgb.z, em.x, em.y, em.z);
            s3 = make_float4(mat.roughness, mat.metallic, rpt_u2f(w.material), 0.0f);
        }
    }
    uint4* ho = reinterpret_cast<uint4*>(q.hits + i);
    ho[0] = h0; ho[1] = h1;
    if constexpr (SURFACE) {
        float4* so = reinterpret_cast<float4*>(q.surfaces + i);
        so[0] = s0; so[1] = s1; so[2] = s2; so[3] = s3;
    }
}

// One ray's occlusion query: any_hit of the scene, whose flags carry RPT_SCENE_ANYHIT_USES_MAX_DIST (query_occluded* below).
template <class S> RPT_DEV void query_any(const S& sc, const QueryArgs& q)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= q.n) return;
    const QueryRay qr = query_load(q.rays, i);
    q.occluded[i] = any_hit(sc, qr.ray, qr.max_dist) ? (uint8_t)1 : (uint8_t)0;
}

}  // namespace

#define RPT_QUERY_BOUNDS __launch_bounds__(256, RPT_QUERY_WAVES_PER_SIMD)

__global__ RPT_QUERY_BOUNDS void query_closest_kernel(const SceneMesh sc, const QueryArgs q) { query_trace<false, false>(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_closest_cut_kernel(const SceneMeshCut sc, const QueryArgs q) { query_trace<true, false>(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_occluded_kernel(const SceneMesh sc, const QueryArgs q) { query_any(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_occluded_cut_kernel(const SceneMeshCut sc, const QueryArgs q) { query_any(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_surface_kernel(const SceneMeshEmit sc, const QueryArgs q) { query_trace<false, true>(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_surface_cut_kernel(const SceneMeshEmitCut sc, const QueryArgs q) { query_trace<true, true>(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_surface_nrm_kernel(const SceneMeshEmitNrm sc, const QueryArgs q) { query_trace<false, true>(sc, q); }
__global__ RPT_QUERY_BOUNDS void query_surface_nrm_cut_kernel(const SceneMeshEmitNrmCut sc, const QueryArgs q) { query_trace<true, true>(sc, q); }

// rpt_camera_rays_device: pixel (x, y), row 0 on top, as a one-device render launch computes its coordinates (pixel_coords), both
// jitter draws 0.5f.
__global__ __launch_bounds__(256) void query_camera_rays_kernel(const DevCamera cam, uint32_t width, uint32_t height, rpt_ray* rays)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)width * height) return;
    RenderParams rp = {};
    rp.width = width; rp.height = height;
    rp.tile_rows = height; rp.rank = 0u; rp.world = 1u;             // one block: local row == global row (capi.hip, launch_render)
    float px, py;
    uint32_t pixel_index;
    pixel_coords(rp, (uint32_t)(i % width), (uint32_t)(i / width), px, py, pixel_index);
    const RayD ray = camera_ray(cam, px, py, 0.5f, 0.5f);
    float4* o = reinterpret_cast<float4*>(rays + i);
    o[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, rpt_u2f(kQueryInfBits));
    o[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f);
}

// (built into librpt_hip_query.so, build.py query_lib_of: the nine launch functions are what the libraries that load it call)
namespace rptlaunch {

template <class S, class K> static hipError_t query_launch(K kernel, const S& sc, const QueryArgs& q, hipStream_t st)
{
    if (q.n == 0) return hipSuccess;
    const uint64_t blocks = q.n / 256u + (q.n % 256u ? 1u : 0u);     // (no n + 255: that wraps for n near 2^64)
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, q);
    return hipGetLastError();
}

// occlusion always honours the ray's max_dist (include/rpt.h, "ray queries")
template <class S> static S query_with_max(const S& sc)
{
    S s = sc;
    s.flags |= (uint32_t)RPT_SCENE_ANYHIT_USES_MAX_DIST;
    return s;
}

__attribute__((visibility("default"))) hipError_t query_closest(const SceneMesh& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_closest_kernel, sc, q, st); }
__attribute__((visibility("default"))) hipError_t query_closest_cut(const SceneMeshCut& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_closest_cut_kernel, sc, q, st); }
__attribute__((visibility("default"))) hipError_t query_occluded(const SceneMesh& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_occluded_kernel, query_with_max(sc), q, st); }
__attribute__((visibility("default"))) hipError_t query_occluded_cut(const SceneMeshCut& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_occluded_cut_kernel, query_with_max(sc), q, st); }
__attribute__((visibility("default"))) hipError_t query_surface(const SceneMeshEmit& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_surface_kernel, sc, q, st); }
__attribute__((visibility("default"))) hipError_t query_surface_cut(const SceneMeshEmitCut& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_surface_cut_kernel, sc, q, st); }
__attribute__((visibility("default"))) hipError_t query_surface_nrm(const SceneMeshEmitNrm& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_surface_nrm_kernel, sc, q, st); }
__attribute__((visibility("default"))) hipError_t query_surface_nrm_cut(const SceneMeshEmitNrmCut& sc, const QueryArgs& q, hipStream_t st) { return query_launch(query_surface_nrm_cut_kernel, sc, q, st); }

__attribute__((visibility("default"))) hipError_t query_camera_rays(const DevCamera& cam, uint32_t width, uint32_t height, rpt_ray* rays, hipStream_t st)
{
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(query_camera_rays_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, cam, width, height, rays);
    return hipGetLastError();
}

}  // namespace rptlaunch
