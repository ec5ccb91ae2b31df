// k_move.hip — the device side of rpt_update_meshes_device / rpt_rebuild_meshes_device (include/rpt.h, "moving meshes from device
// memory"): a mesh's new positions read from device memory, through an optional affine transform, first checked, then stored into
// the context's vertex table.  host_move.h has the statement of the transform and what the check reduces, as plain functions this
// file compiles for the device, and the same two passes on the host, which the tests hold these kernels to: plain f32 multiplies and
// adds (-ffp-contract=off: build.py).
//
// The kernels are named meshmove_* and live in a code object library of their own (build.py, move_lib_of): the other libraries'
// censuses stay what they were.  Both are one thread per vertex of one named mesh, without a loop over data, and keep everything in
// registers; the check writes nothing but two atomics per workgroup, so a rejected call has stored no position anywhere.  The host
// has checked that the source holds `n` vertices' worth of device memory by the caller's word (n == the uploaded mesh's count) and
// that `dst` + 3n floats lies inside the context's vertex table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RPT_MOVE_FN __host__ __device__ inline
#include "host_move.h"
#include "launch_move.h"

using namespace rpthost;

// One thread per vertex: host_move.h, move_check_reference.  A wave's two words by shuffles, a workgroup's through LDS, then two
// atomic max per workgroup into words the host zeroed.
__global__ __launch_bounds__(256) void meshmove_check_kernel(const float* __restrict__ src, MoveTransform xf, const uint8_t* __restrict__ referenced,
                                                             uint32_t* __restrict__ words, uint32_t n)
{
    __shared__ uint32_t part[4][kMoveWords];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    uint32_t big = 0u, bad = 0u;
    if (v < n) {
        const float* s = src + 3u * (size_t)v;
        const float in[3] = {s[0], s[1], s[2]};
        float p[3];
        move_vertex(xf, in, p);
        move_vertex_words(p, v, referenced[v] != 0, big, bad);
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t g = (uint32_t)__shfl_xor((int)big, d, 64), b = (uint32_t)__shfl_xor((int)bad, d, 64);
        big = g > big ? g : big;
        bad = b > bad ? b : bad;
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0u) { part[wave][kMoveWordBig] = big; part[wave][kMoveWordBad] = bad; }
    __syncthreads();
    if (threadIdx.x < kMoveWords) {
        uint32_t w = part[0][threadIdx.x];
        for (uint32_t k = 1; k < 4u; ++k) {
            const uint32_t x = part[k][threadIdx.x];
            w = x > w ? x : w;
        }
        if (w) atomicMax(&words[threadIdx.x], w);
    }
}

// One thread per vertex: host_move.h, move_apply_reference — the same load, the same statement, and the store.
__global__ __launch_bounds__(256) void meshmove_apply_kernel(const float* __restrict__ src, MoveTransform xf, float* __restrict__ dst, uint32_t n)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const float* s = src + 3u * (size_t)v;
    const float in[3] = {s[0], s[1], s[2]};
    float p[3];
    move_vertex(xf, in, p);
    float* o = dst + 3u * (size_t)v;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// (built into librpt_hip_move.so, build.py move_lib_of: the two launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t move_check(const float* src, const MoveTransform& xf, const uint8_t* referenced, uint32_t* words, uint32_t n,
                                                             hipStream_t st)
{
    if (n == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshmove_check_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, src, xf, referenced, words, n);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t move_apply(const float* src, const MoveTransform& xf, float* dst, uint32_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(meshmove_apply_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, src, xf, dst, n);
    return hipGetLastError();
}

}  // namespace rptlaunch
