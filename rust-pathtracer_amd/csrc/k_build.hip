// k_build.hip — a mesh scene's hierarchy built on the device (include/rpt.h, "rebuilding a moved mesh's hierarchy"): rpt_rebuild_meshes'
// new slot order and new shape.  host_build.h has the rules — the key of a triangle, where a node splits, when a child is a leaf, why
// no leaf lies deeper than the walk's stack — as plain functions this file compiles for the device, and the same topology step on the
// host, which the tests hold these kernels to.  The rows and the boxes are the refit's work (k_refit.hip), reused as it is.
//
// The kernels are named bvhbuild_* and live in a code object library of their own (build.py, build_lib_of), with the rocPRIM kernels
// of the sort and of the levels' prefix sums: the other libraries' censuses stay what they were.  Every kernel is one thread per item
// with bounded loops, waits for nothing, and keeps everything in registers; kernel boundaries on the caller's stream are the only
// ordering.  Every index a kernel writes through is below the size the host allocated: slots below n_slots (the sort's values are a
// permutation of them), node indices checked against max_nodes before they are used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#define RPT_BUILD_FN __host__ __device__ inline
#include "host_build.h"
#include "launch_build.h"

using namespace rpthost;

namespace {

// f32 -> u32 whose unsigned order is the floats' order (-0 below +0); kept for the bounds' atomics
__device__ __forceinline__ uint32_t ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// a slot's centroid: host_bvh.h, build_bvh
__device__ __forceinline__ void centroid_of(const float* slot_box, uint32_t slot, float* c)
{
    const float2* b = reinterpret_cast<const float2*>(slot_box + 6u * (size_t)slot);
    const float2 b0 = b[0], b1 = b[1], b2 = b[2];
    c[0] = b0.x * 0.5f + b1.y * 0.5f;
    c[1] = b0.y * 0.5f + b2.x * 0.5f;
    c[2] = b1.x * 0.5f + b2.y * 0.5f;
}

}  // namespace

// One workgroup: the level table (level 0 = the root over every slot), the status, the bounds' identities.
__global__ __launch_bounds__(64) void bvhbuild_init_kernel(uint32_t* __restrict__ levels, uint32_t* __restrict__ bounds, uint2* __restrict__ range, uint32_t n_slots)
{
    const uint32_t i = threadIdx.x;
    levels[i] = i == kBuildLevelCount ? 1u : 0u;                    // (kBuildLevelWords == 64 == the workgroup)
    if (i < 3u) bounds[i] = 0xFFFFFFFFu;
    else if (i < 6u) bounds[i] = 0u;
    if (i == 0u) range[0] = make_uint2(0u, n_slots);
}

// One thread per slot: the centroids' bounds, as ordered words — a wave's by shuffles, a workgroup's through LDS, then six atomics
// per workgroup (min and max commute: the result does not depend on the order).  A centroid that is not a number takes no part.
__global__ __launch_bounds__(256) void bvhbuild_bounds_kernel(const float* __restrict__ slot_box, uint32_t* __restrict__ bounds, uint32_t n_slots)
{
    __shared__ uint32_t part[4][6];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (slot < n_slots) {
        float c[3];
        centroid_of(slot_box, slot, c);
        for (int a = 0; a < 3; ++a)
            if (c[a] == c[a]) lo[a] = hi[a] = ordered(c[a]);
    }
    for (int a = 0; a < 3; ++a)
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t l = (uint32_t)__shfl_xor((int)lo[a], d, 64), h = (uint32_t)__shfl_xor((int)hi[a], d, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0u)
        for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6u) {
        uint32_t v = part[0][threadIdx.x];
        for (uint32_t w = 1; w < 4u; ++w) {
            const uint32_t x = part[w][threadIdx.x];
            v = threadIdx.x < 3u ? (x < v ? x : v) : (x > v ? x : v);
        }
        if (threadIdx.x < 3u) atomicMin(&bounds[threadIdx.x], v);
        else atomicMax(&bounds[threadIdx.x], v);
    }
}

// One thread per slot: its key (host_build.h, build_key) and itself as the value.
__global__ __launch_bounds__(256) void bvhbuild_keys_kernel(const float* __restrict__ slot_box, const float4* __restrict__ tris, const uint32_t* __restrict__ bounds,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t n_slots)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_slots) return;
    float c[3], lo[3], hi[3];
    centroid_of(slot_box, slot, c);
    for (int a = 0; a < 3; ++a) { lo[a] = unordered(bounds[a]); hi[a] = unordered(bounds[3 + a]); }
    keys[slot] = build_key(c, lo, hi, __float_as_uint(tris[3u * (size_t)slot].w));
    vals[slot] = slot;
}

// One thread per NEW slot: the .w words of the row and the three vertex indices of the slot that moves here, into `gather`
// ([6][n_slots]); then (bvhbuild_scatter_kernel, after a kernel boundary: the tables are permuted in place) into the tables.  The
// rows' float part is the refit's to write.
__global__ __launch_bounds__(256) void bvhbuild_gather_kernel(const uint32_t* __restrict__ from, const float4* __restrict__ tris,
                                                              const uint32_t* __restrict__ slot_vertex, uint32_t* __restrict__ gather, uint32_t n_slots)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_slots) return;
    const uint32_t old = from[slot];
    if (old >= n_slots) return;                                     // (a permutation: never)
    for (uint32_t k = 0; k < 3u; ++k) {
        gather[(size_t)k * n_slots + slot] = __float_as_uint(tris[3u * (size_t)old + k].w);
        gather[(size_t)(3u + k) * n_slots + slot] = slot_vertex[(size_t)k * n_slots + old];
    }
}

__global__ __launch_bounds__(256) void bvhbuild_scatter_kernel(const uint32_t* __restrict__ gather, float4* __restrict__ tris, uint32_t* __restrict__ slot_vertex,
                                                               uint32_t n_slots)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_slots) return;
    for (uint32_t k = 0; k < 3u; ++k) {
        tris[3u * (size_t)slot + k] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(gather[(size_t)k * n_slots + slot]));
        slot_vertex[(size_t)k * n_slots + slot] = gather[(size_t)(3u + k) * n_slots + slot];
    }
}

// One thread per possible node of level `depth` (`bound` of them; the level's count is in `levels`): host_build.h, build_node_split.
// Threads beyond the count write zeros: the prefix sum runs over 2 * bound flags.
__global__ __launch_bounds__(256) void bvhbuild_split_kernel(const uint64_t* __restrict__ keys, const uint2* __restrict__ range, uint32_t* __restrict__ mid,
                                                             uint32_t* __restrict__ flags, const uint32_t* __restrict__ levels, uint32_t depth, uint32_t bound,
                                                             uint32_t leaf_target, uint32_t n_slots, uint32_t max_nodes)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= bound) return;
    uint32_t interior[2] = {0u, 0u};
    const uint32_t first = levels[depth], count = levels[kBuildLevelCount + depth];
    if (j < count && first + j < max_nodes) {
        const uint32_t node = first + j;
        const uint2 r = range[node];
        uint32_t m = r.y;
        if (r.x < r.y && r.y <= n_slots) build_node_split(keys, r.x, r.y, depth, leaf_target, &m, interior);
        mid[node] = m;
    }
    reinterpret_cast<uint2*>(flags)[j] = make_uint2(interior[0], interior[1]);
}

// One thread per node of the level: host_build.h, build_node_children — the node's child words, the children's ranges, and (the
// level's last node) the next level's first node and count.
__global__ __launch_bounds__(256) void bvhbuild_emit_kernel(uint2* __restrict__ range, const uint32_t* __restrict__ mid, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ offsets, float4* __restrict__ nodes, uint32_t* __restrict__ levels,
                                                            uint32_t depth, uint32_t bound, uint32_t max_nodes)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const uint32_t first = levels[depth], count = levels[kBuildLevelCount + depth];
    if (j >= bound || j >= count || first + j >= max_nodes) return;
    const uint32_t node = first + j, next_first = first + count;
    const uint2 r = range[node];
    const uint32_t m = mid[node];
    const uint32_t interior[2] = {flags[2u * (size_t)j], flags[2u * (size_t)j + 1u]};
    const uint32_t off[2] = {offsets[2u * (size_t)j], offsets[2u * (size_t)j + 1u]};
    uint32_t status = 0u;
    if (j == count - 1u) {
        const uint32_t below = off[1] + interior[1];
        if (depth + 1u >= kBvhMaxDepth && below) status |= kBuildStatusTooDeep;
        if ((uint64_t)next_first + below > max_nodes) status |= kBuildStatusNodes;
        levels[depth + 1u] = next_first;
        levels[kBuildLevelCount + depth + 1u] = status ? 0u : below;     // (a failed build stops here: the host reads the status)
    }
    uint32_t next[2] = {next_first + off[0], next_first + off[1]}, child[2];
    for (int c = 0; c < 2; ++c)
        if (interior[c] && next[c] >= max_nodes) { status |= kBuildStatusNodes; next[c] = 0u; }
    build_node_children(r.x, m, r.y, interior, next, child, &status);
    nodes[4u * (size_t)node + 3u] = make_float4(__uint_as_float(child[0]), __uint_as_float(child[1]), 0.0f, 0.0f);
    if (!(status & kBuildStatusNodes)) {
        if (interior[0]) range[next[0]] = make_uint2(r.x, m);
        if (interior[1]) range[next[1]] = make_uint2(m, r.y);
    }
    if (status) atomicOr(&levels[kBuildStatus], status);
}

// level_nodes of a breadth-first hierarchy: every level's nodes are contiguous
__global__ __launch_bounds__(256) void bvhbuild_iota_kernel(uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = i;
}

// (built into librpt_hip_build.so, build.py build_lib_of: the launch functions are what the libraries that load it call)
namespace rptlaunch {

namespace {
hipError_t sort_bytes(uint32_t n, size_t& bytes)
{
    bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u,
                                     kBuildKeyBits, (hipStream_t) nullptr);
}
hipError_t scan_bytes(uint32_t n, size_t& bytes)
{
    bytes = 0;
    return rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
}
dim3 grid_of(uint32_t n) { return dim3((n + 255u) / 256u); }
}  // namespace

__attribute__((visibility("default"))) hipError_t build_temp_bytes(uint32_t n_slots, size_t* bytes)
{
    size_t most = 0, b = 0;
    hipError_t e = sort_bytes(n_slots, b);
    if (e != hipSuccess) return e;
    most = b;
    for (uint32_t k = 0; k < kBvhMaxDepth; ++k) {
        e = scan_bytes(2u * build_level_bound(n_slots, k), b);
        if (e != hipSuccess) return e;
        most = b > most ? b : most;
    }
    *bytes = most;
    return hipSuccess;
}

// Steps 2-5 of the build: the slots' boxes (the refit wrote them, in the present order) -> keys -> the sort -> the rows' .w words
// and the vertex indices in the new order.
__attribute__((visibility("default"))) hipError_t build_order(const BuildTables& t, hipStream_t st)
{
    if (t.n_slots == 0) return hipSuccess;
    size_t bytes = 0;
    hipError_t e = sort_bytes(t.n_slots, bytes);
    if (e != hipSuccess) return e;
    if (bytes > t.temp_bytes) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(bvhbuild_init_kernel, dim3(1), dim3(64), 0, st, t.levels, t.bounds, t.range, t.n_slots);
    hipLaunchKernelGGL(bvhbuild_bounds_kernel, grid_of(t.n_slots), dim3(256), 0, st, t.slot_box, t.bounds, t.n_slots);
    hipLaunchKernelGGL(bvhbuild_keys_kernel, grid_of(t.n_slots), dim3(256), 0, st, t.slot_box, t.tris, t.bounds, t.keys_in, t.vals_in, t.n_slots);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(t.temp, bytes, (const uint64_t*)t.keys_in, t.keys_out, (const uint32_t*)t.vals_in, t.vals_out, t.n_slots, 0u, kBuildKeyBits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bvhbuild_gather_kernel, grid_of(t.n_slots), dim3(256), 0, st, t.vals_out, t.tris, t.slot_vertex, t.gather, t.n_slots);
    hipLaunchKernelGGL(bvhbuild_scatter_kernel, grid_of(t.n_slots), dim3(256), 0, st, t.gather, t.tris, t.slot_vertex, t.n_slots);
    return hipGetLastError();
}

// Step 6: the shape over the sorted keys, level by level — every level launched for the most nodes it can have, the levels' counts
// staying on the device —, and the refit's level order.  The caller reads t.levels back afterwards.
__attribute__((visibility("default"))) hipError_t build_shape(const BuildTables& t, uint32_t leaf_target, hipStream_t st)
{
    if (t.n_slots == 0) return hipSuccess;
    if (leaf_target < 1u || leaf_target > kBvhLeafMax) return hipErrorInvalidValue;
    (void)hipGetLastError();
    for (uint32_t depth = 0; depth < kBvhMaxDepth; ++depth) {
        const uint32_t bound = build_level_bound(t.n_slots, depth);
        size_t bytes = 0;
        hipError_t e = scan_bytes(2u * bound, bytes);
        if (e != hipSuccess) return e;
        if (bytes > t.temp_bytes) return hipErrorInvalidValue;
        hipLaunchKernelGGL(bvhbuild_split_kernel, grid_of(bound), dim3(256), 0, st, (const uint64_t*)t.keys_out, (const uint2*)t.range, t.mid, t.flags,
                           (const uint32_t*)t.levels, depth, bound, leaf_target, t.n_slots, t.max_nodes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        e = rocprim::exclusive_scan(t.temp, bytes, (const uint32_t*)t.flags, t.offsets, 0u, (size_t)(2u * bound), rocprim::plus<uint32_t>(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bvhbuild_emit_kernel, grid_of(bound), dim3(256), 0, st, t.range, (const uint32_t*)t.mid, (const uint32_t*)t.flags,
                           (const uint32_t*)t.offsets, t.nodes, t.levels, depth, bound, t.max_nodes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bvhbuild_iota_kernel, grid_of(t.max_nodes), dim3(256), 0, st, t.level_nodes, t.max_nodes);
    return hipGetLastError();
}

}  // namespace rptlaunch
