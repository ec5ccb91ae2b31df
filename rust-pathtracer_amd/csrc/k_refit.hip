// k_refit.hip — the refit of a mesh scene's tables on the device (include/rpt.h, "moving meshes"): the triangle rows and the
// hierarchy's boxes recomputed from new vertex positions, the hierarchy's shape kept.  host_refit.h has the tables, why the result is
// what a fresh build would store, and the same two steps on the host (refit_slot, refit_node), which the tests hold these kernels
// to byte for byte: plain f32 subtractions and additions (-ffp-contract=off: build.py) and min / max as selections with std::min's
// and std::max's choice between equal operands (the sign of a zero bound).
//
// The kernels are named refit_* and live in a code object library of their own (build.py, refit_lib_of): the other libraries' censuses
// stay what they were.  Both are one thread per item, read through 32-bit indices the host built and checked (a slot's three vertex
// indices are below the vertex count, a leaf's slots below the slot count, a child below the node count), and keep everything in
// registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// std::min(a, b) / std::max(a, b): `a` unless b is strictly smaller / larger
__device__ __forceinline__ float sel_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float sel_max(float a, float b) { return a < b ? b : a; }

constexpr uint32_t kLeaf = 0x80000000u, kCountShift = 27u, kSlotMask = (1u << kCountShift) - 1u;      // host_bvh.h's child word
constexpr float kInf = __builtin_huge_valf();

struct Box3 {
    float lo[3], hi[3];
};
__device__ __forceinline__ void box_empty(Box3& x)
{
    for (int a = 0; a < 3; ++a) { x.lo[a] = kInf; x.hi[a] = -kInf; }
}
__device__ __forceinline__ void box_grow(Box3& x, const float* lo, const float* hi)
{
    for (int a = 0; a < 3; ++a) { x.lo[a] = sel_min(x.lo[a], lo[a]); x.hi[a] = sel_max(x.hi[a], hi[a]); }
}

}  // namespace

// One thread per slot: host_refit.h, refit_slot.  Rows are written as whole float4s, their .w words carried through.
__global__ __launch_bounds__(256) void refit_triangles_kernel(const float* __restrict__ vertices, const uint32_t* __restrict__ slot_vertex,
                                                              float4* __restrict__ tris, float* __restrict__ slot_box, uint32_t n_slots)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_slots) return;
    float v[9];
    for (uint32_t c = 0; c < 3u; ++c) {
        const float* p = vertices + 3u * (size_t)slot_vertex[(size_t)c * n_slots + slot];
        v[3 * c] = p[0]; v[3 * c + 1] = p[1]; v[3 * c + 2] = p[2];
    }
    float4* row = tris + 3u * (size_t)slot;
    const float w0 = row[0].w, w1 = row[1].w, w2 = row[2].w;
    row[0] = make_float4(v[0], v[1], v[2], w0);
    row[1] = make_float4(v[3] - v[0], v[4] - v[1], v[5] - v[2], w1);
    row[2] = make_float4(v[6] - v[0], v[7] - v[1], v[8] - v[2], w2);
    // host_bvh.h, triangle_box: the three vertices, then a + min(0, e1, e2) and a + max(0, e1, e2) per axis
    Box3 x;
    box_empty(x);
    for (int k = 0; k < 3; ++k) box_grow(x, &v[3 * k], &v[3 * k]);
    for (int a = 0; a < 3; ++a) {
        const float e1 = v[3 + a] - v[a], e2 = v[6 + a] - v[a];
        const float lo = v[a] + sel_min(sel_min(0.0f, e1), e2), hi = v[a] + sel_max(sel_max(0.0f, e1), e2);
        x.lo[a] = sel_min(x.lo[a], lo);
        x.hi[a] = sel_max(x.hi[a], hi);
    }
    float2* out = reinterpret_cast<float2*>(slot_box + 6u * (size_t)slot);      // (24 B per slot: 8-byte aligned)
    out[0] = make_float2(x.lo[0], x.lo[1]);
    out[1] = make_float2(x.lo[2], x.hi[0]);
    out[2] = make_float2(x.hi[1], x.hi[2]);
}

// One thread per interior node of one level: host_refit.h, refit_node.  A node is four float4: the left child's box lo xyz, hi xyz, the
// right child's, then the two child words (host_bvh.h, BvhNode).
__global__ __launch_bounds__(256) void refit_nodes_kernel(float4* __restrict__ nodes, const float* __restrict__ slot_box,
                                                          const uint32_t* __restrict__ level_nodes, uint32_t count)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    float4* node = nodes + 4u * (size_t)level_nodes[k];
    const float4 words = node[3];
    const uint32_t child[2] = {__float_as_uint(words.x), __float_as_uint(words.y)};
    Box3 box[2];
    for (int c = 0; c < 2; ++c) {
        Box3& x = box[c];
        box_empty(x);
        const uint32_t ch = child[c];
        if (ch & kLeaf) {
            const uint32_t cnt = (ch >> kCountShift) & 15u, first = ch & kSlotMask;
            for (uint32_t s = first; s < first + cnt; ++s) {
                const float2* b = reinterpret_cast<const float2*>(slot_box + 6u * (size_t)s);
                const float2 b0 = b[0], b1 = b[1], b2 = b[2];
                const float lo[3] = {b0.x, b0.y, b1.x}, hi[3] = {b1.y, b2.x, b2.y};
                box_grow(x, lo, hi);
            }
        } else {
            const float4* n = nodes + 4u * (size_t)ch;
            const float4 n0 = n[0], n1 = n[1], n2 = n[2];
            const float llo[3] = {n0.x, n0.y, n0.z}, lhi[3] = {n0.w, n1.x, n1.y};
            const float rlo[3] = {n1.z, n1.w, n2.x}, rhi[3] = {n2.y, n2.z, n2.w};
            box_grow(x, llo, lhi);
            box_grow(x, rlo, rhi);
        }
    }
    node[0] = make_float4(box[0].lo[0], box[0].lo[1], box[0].lo[2], box[0].hi[0]);
    node[1] = make_float4(box[0].hi[1], box[0].hi[2], box[1].lo[0], box[1].lo[1]);
    node[2] = make_float4(box[1].lo[2], box[1].hi[0], box[1].hi[1], box[1].hi[2]);
}

// (built into librpt_hip_refit.so, build.py refit_lib_of: the two launch functions are what the libraries that load it call)
namespace rptlaunch {

__attribute__((visibility("default"))) hipError_t refit_triangles(const float* vertices, const uint32_t* slot_vertex, float4* tris, float* slot_box,
                                                                  uint32_t n_slots, hipStream_t st)
{
    if (n_slots == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(refit_triangles_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, st, vertices, slot_vertex, tris, slot_box, n_slots);
    return hipGetLastError();
}

__attribute__((visibility("default"))) hipError_t refit_nodes(float4* nodes, const float* slot_box, const uint32_t* level_nodes, uint32_t count, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(refit_nodes_kernel, dim3((count + 255u) / 256u), dim3(256), 0, st, nodes, slot_box, level_nodes, count);
    return hipGetLastError();
}

}  // namespace rptlaunch
