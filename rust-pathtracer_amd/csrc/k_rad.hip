// k_rad.hip — the device side of radiance queries (include/rpt.h, "radiance queries"): the integrator's estimate along rays the caller
// brings, and the camera's sample rays.  The path-regenerating state machine of regen_body.h over a plain 1-D grid — workgroup b owns
// rays 256 b ..., a lane's "pixel" is a ray index — with a path's first segment loaded from the batch instead of made by camera_ray.
// Strict arithmetic, built like k_med.hip (-ffp-contract=off, the range tests next to every operation).
//
// The kernels are named radiance_* and live in a code object library of their own (build.py, rad_lib_of): the other libraries'
// censuses stay what they were.  The device functions are the render forms': path_trace_geom, path_shade_full, blend, the share_*
// hand-out of a wave's samples and the dev_mesh_*.h overloads, called as they are.  What is this file's own is the start of a path
// (rad_begin: path_begin with the ray loaded and the two jitter draws discarded) and the scaffolding around the loop: no tiles, no
// chunks, no unit, no timing table.
//
// Nine kernels.  The eight forms exist per combination that changes a function's body — normal map x cutout x environment — over
// the media forms' scene types, which hold every table a mesh scene can have; a feature that is absent is reached through the empty
// tables of the media's allocation or of the query's own (host_rad.h, mesh_args_rad.h).  And the camera's sample rays.
//
// Two translation units of this one file, as k_med.hip (build.py): RPT_RAD_PART 0 holds the camera's kernel and the four forms
// without a normal map, RPT_RAD_PART 1 the four with one.
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
#define RPT_MED_FN __host__ __device__ inline
#include "host_light.h"
#include "launch_rad.h"
#include "dev_mesh_smooth.h"
#include "dev_mesh_light.h"
#include "dev_mesh_tex.h"
#include "dev_mesh_env.h"
#include "dev_mesh_cut.h"
#include "dev_mesh_nrm.h"
#include "dev_mesh_mmap.h"
#include "dev_mesh_emap.h"
#include "dev_mesh_med.h"

#include "regen_body.h"

using namespace rpthost;

#ifndef RPT_RAD_PART
#error "k_rad.hip is built twice: -DRPT_RAD_PART=0 and -DRPT_RAD_PART=1 (build.py)"
#endif
#if RPT_MATH_MODE == 2
#error "k_rad.hip tests its operand ranges next to every operation (-DRPT_GUARD_PER_OP): a sample is never computed a second time"
#endif
// Waves per SIMD of the radiance forms: the media forms' four ("radiance queries").
#ifndef RPT_RAD_WAVES_PER_SIMD
#define RPT_RAD_WAVES_PER_SIMD 4
#endif

namespace {

// The start of sample `fkey` of ray `ray` (base: the workgroup's first ray): path_begin (dev_integrator.h) with the stream of the two
// hashes `h`, its two first draws made and discarded — the draws a camera sample spends on its jitter — and the ray as the caller
// gave it: two 16-byte loads, every time (the 24 bytes are not parked in LDS; a path's later starts find them in L2).
RPT_DEV void rad_begin(const rpt_ray* rays, uint64_t ray, PathRegs& p, FrameKey fkey, uint2 h)
{
    p.rng.init_hashed(fkey, h.x, h.y);
    (void)p.rng.gen();
    (void)p.rng.gen();
    const float4* r = reinterpret_cast<const float4*>(rays + ray);
    const float4 a = r[0], b = r[1];
    p.ray.o = mk3(a.x, a.y, a.z);
    p.ray.d = mk3(b.x, b.y, b.z);                                   // (not normalised; max_dist and reserved are not read)
    p.radiance = mk3(0.0f, 0.0f, 0.0f);
    p.throughput = mk3(1.0f, 1.0f, 1.0f);
    p.ps.hit_dist = -1.0f;
    p.ps.scatter_pdf = 0.0f;
    p.bounce = 0;
    p.medium = 0u;                                                  // (outside every medium, wherever the origin lies)
}

// Where this lane's ColorBuffer pixel lives, from a thread index the compiler cannot identify with the prologue's (kernel_common.h,
// pixel_address_again).
RPT_DEV float4* rad_out_again(const RadArgs& a)
{
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return reinterpret_cast<float4*>(a.out) + ((uint64_t)blockIdx.x * 256u + tid);
}

// render_regen_body_tf (regen_body.h) over rays: the same states, the same votes, the same hand-out and order of blends.
template <class S>
RPT_DEV void radiance_body(const S& sc, const RadArgs& a)
{
    __shared__ FrameKey s_fkey[kMaxSppPerLaunch];
    __shared__ float s_weight[kMaxSppPerLaunch];
    __shared__ float4 s_acc[256];
    __shared__ uint2 s_pix[256];                                    // the two hashes of the ray's stream index (Rng::init)
    __shared__ uint32_t s_count[256];                               // share_* (kernel_common.h): each ray's samples handed out and blended
    const uint32_t tid = threadIdx.x;
    share_init(s_count, false);                                     // (until the lane is known to have a ray)
    for (uint32_t i = tid; i < a.spp; i += 256u) {
        const uint64_t frames = a.frames_done + i;
        s_fkey[i] = frame_key_hd(a.seed, frames);
        s_weight[i] = 1.0f / (float)(frames + 1);                   // tracer.rs:115
    }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * 256u;              // this workgroup's first ray
    if (base + tid >= a.n) return;                                  // (no barrier below)
    if (sc.max_depth == 0) {                                        // no bounce loop at all: every sample's radiance is zero
        float4* o = reinterpret_cast<float4*>(a.out) + (base + tid);
        float4 acc = *o;
        for (uint32_t s = 0; s < a.spp; ++s) blend(acc, mk3(0.0f, 0.0f, 0.0f), s_weight[s]);
        *o = acc;
        return;
    }
    s_acc[tid] = reinterpret_cast<const float4*>(a.out)[base + tid];
    {
        const uint32_t h = pcg_hash(a.first_index + (uint32_t)(base + tid));
        s_pix[tid] = make_uint2(h, pcg_hash(h));
    }
    share_init(s_count, true);

    uint32_t s = 0;
    uint32_t q = tid;                                               // the ray this lane computes a sample of: its own while that has any
    uint32_t state = ST_TRACE;
    PathRegs p;
    GeomHit g;
    g.code = 0u;
    rad_begin(a.rays, base + tid, p, s_fkey[0], s_pix[tid]);

    for (;;) {
        const uint32_t own = share_handed_out(s_count);
        const uint64_t needy = __ballot(own < a.spp);
        if (state == ST_FINISH || state == ST_BLOCKED) {
            if (!share_my_turn(s_count, q, s)) {
                state = ST_BLOCKED;                                 // an earlier sample of the ray is still on its way: asked again every pass
            } else {
                float4 acc = s_acc[q];
                blend(acc, p.radiance, s_weight[s]);
                s_acc[q] = acc;
                share_blended(s_count, q);
                if (!share_next(s_count, a.spp, own, needy, q, s)) {
                    state = ST_DONE;
                } else {
                    rad_begin(a.rays, base + q, p, s_fkey[s], s_pix[q]);
                    state = ST_TRACE;
                }
            }
        }
        if (state == ST_TRACE) state = path_trace_geom(sc, DirectQuery{}, p, g) ? ST_SHADE : ST_FINISH;
        const uint64_t m_shade = __ballot(state == ST_SHADE);
        const uint64_t m_go = __ballot(state == ST_TRACE || state == ST_FINISH);
        if ((m_shade | m_go | __ballot(state == ST_BLOCKED)) == 0ull) break;
        if ((uint32_t)__popcll(m_shade) >= a.shade_threshold || m_go == 0ull) {
            if (state == ST_SHADE) state = path_shade_full(sc, DirectQuery{}, p, g) ? ST_FINISH : ST_TRACE;
        }
    }
    *rad_out_again(a) = s_acc[tid];
}

}  // namespace

// One radiance form over one scene type, and its launch function.  The scene is the first argument, by value, read through the
// kernarg segment (kernel_common.h, kernarg_scene).
#define RPT_RAD_FORM(kernel, launcher, Scene)                                                                                                \
    __global__ __launch_bounds__(256, RPT_RAD_WAVES_PER_SIMD) void kernel(const Scene sc, const RadArgs a) { radiance_body(kernarg_scene(sc), a); }  \
    namespace rptlaunch {                                                                                                                    \
    __attribute__((visibility("default"))) hipError_t launcher(const Scene& sc, const RadArgs& a, hipStream_t st)                            \
    {                                                                                                                                        \
        if (a.n == 0 || a.spp == 0) return hipSuccess;                                                                                       \
        const uint64_t blocks = a.n / 256u + (a.n % 256u ? 1u : 0u);     /* (no n + 255: that wraps for n near 2^64) */                      \
        if (blocks > 0x7FFFFFFFull || a.spp > kMaxSppPerLaunch) return hipErrorInvalidValue;                                                 \
        (void)hipGetLastError();                                                                                                             \
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, st, sc, a);                                                         \
        return hipGetLastError();                                                                                                            \
    }                                                                                                                                        \
    }

#if RPT_RAD_PART == 0

RPT_RAD_FORM(radiance_kernel, radiance, SceneMeshMed)
RPT_RAD_FORM(radiance_env_kernel, radiance_env, SceneMeshMedEnv)
RPT_RAD_FORM(radiance_cut_kernel, radiance_cut, SceneMeshMedCut)
RPT_RAD_FORM(radiance_cut_env_kernel, radiance_cut_env, SceneMeshMedCutEnv)

// rpt_camera_sample_rays_device: query_camera_rays_kernel (k_query.hip) with the two jitter draws taken from the pixel's stream, as
// path_begin takes them, and not replaced by 0.5f.
__global__ __launch_bounds__(256) void radiance_camera_rays_kernel(const DevCamera cam, uint32_t width, uint32_t height, FrameKey fkey, rpt_ray* rays)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)width * height) return;
    RenderParams rp = {};
    rp.width = width; rp.height = height;
    rp.tile_rows = height; rp.rank = 0u; rp.world = 1u;             // one block: local row == global row (capi.hip, launch_render)
    float px, py;
    uint32_t pixel_index;
    pixel_coords(rp, (uint32_t)(i % width), (uint32_t)(i / width), px, py, pixel_index);
    Rng rng;
    rng.init(fkey, pixel_index);
    const float offx = rng.gen();
    const float offy = rng.gen();
    const RayD ray = camera_ray(cam, px, py, offx, offy);
    float4* o = reinterpret_cast<float4*>(rays + i);
    o[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, rpt_u2f(0x7F800000u));
    o[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f);
}

// (built into librpt_hip_rad.so, build.py rad_lib_of: the launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t radiance_camera_rays(const DevCamera& cam, uint32_t width, uint32_t height, FrameKey fkey, rpt_ray* rays, hipStream_t st)
{
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(radiance_camera_rays_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, cam, width, height, fkey, rays);
    return hipGetLastError();
}

__attribute__((visibility("default"))) uint32_t radiance_max_spp() { return kMaxSppPerLaunch; }

}  // namespace rptlaunch

#else

RPT_RAD_FORM(radiance_nrm_kernel, radiance_nrm, SceneMeshMedNrm)
RPT_RAD_FORM(radiance_nrm_env_kernel, radiance_nrm_env, SceneMeshMedNrmEnv)
RPT_RAD_FORM(radiance_nrm_cut_kernel, radiance_nrm_cut, SceneMeshMedNrmCut)
RPT_RAD_FORM(radiance_nrm_cut_env_kernel, radiance_nrm_cut_env, SceneMeshMedNrmCutEnv)

#endif
