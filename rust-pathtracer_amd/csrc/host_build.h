// host_build.h — the rules of rpt_rebuild_meshes' hierarchy build (include/rpt.h, "rebuilding a moved mesh's hierarchy"), written once:
// the sort key of a triangle, where a node splits, and when a child is a leaf.  Plain C++ with no HIP type in it, like host_bvh.h
// and host_refit.h: k_build.hip compiles these functions for the device (it defines RPT_BUILD_FN before the include), capi.hip
// uses the layout of the build's device tables, and tests/build_harness.cpp runs the same text — and build_topology, the whole
// topology step over a sorted key array on the host — under the address and undefined-behaviour sanitizers
// (tests/test_mesh_rebuild_host.py).
//
// The build: every triangle gets a 64-bit key — a 30-bit Morton code of its box's centroid, quantised within the centroids' bounds,
// above its 26-bit flattened index — so keys are unique and their order is one.  The triangle table is put into key order; the
// hierarchy is then built top-down over ranges of that order, one level per step, a node's index below its children's and every
// level's nodes contiguous (breadth-first), so the refit's level order (host_refit.h) is level k = nodes [first_k, first_k + count_k).
//
// Depth.  No leaf lies deeper than kBvhMaxDepth below the root (the walk's stack, dev_scene_mesh.h), by host_bvh.h's capacity
// rule: a node at depth k holds at most kBvhLeafMax << (kBvhMaxDepth - k) triangles.  The root does (2^27 >= 2^26 triangles); a
// node splits where the highest differing key bit changes unless a side would exceed the children's capacity, and then at the
// middle position, which halves it: ceil(n / 2) <= cap whenever n <= 2 cap.  A child at depth kBvhMaxDepth therefore holds at
// most kBvhLeafMax and is a leaf whatever the leaf target says.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "host_bvh.h"

#ifndef RPT_BUILD_FN
#define RPT_BUILD_FN inline                    // (k_build.hip: __host__ __device__ inline)
#endif

namespace rpthost {

constexpr uint32_t kBuildIndexBits = 26;       // the flattened index: below kBvhMaxTriangles = 2^26
constexpr uint32_t kBuildAxisBits = 10;        // per axis: a 30-bit Morton code
constexpr uint32_t kBuildKeyBits = 3u * kBuildAxisBits + kBuildIndexBits;
// A child of this many triangles or fewer is a leaf (at most kBvhLeafMax).  Measured, scenes.mesh_scene at 1920x1080
// (tools/mesh_bench.py --rebuild, profiles/NOTES.md): after the large move 2 / 4 / 8 render 0.418 / 0.412 / 0.381 Gsamples/s.
constexpr uint32_t kBuildLeafTarget = 2;

// A centroid coordinate within [lo, hi] -> 0 .. 2^kBuildAxisBits - 1.  Defined for every input: the arithmetic is f64 (the
// difference of two finite f32 is exact and finite there), an axis of zero, infinite or NaN extent gives 0, and so does a
// coordinate that is not a number or not within the bounds — nothing but a value in [0, 1023] reaches the conversion.
RPT_BUILD_FN uint32_t build_quantise(float c, float lo, float hi)
{
    const double ext = (double)hi - (double)lo;
    if (!(ext > 0.0) || !(ext <= 1.0e39)) return 0u;
    const double t = ((double)c - (double)lo) / ext * (double)(1u << kBuildAxisBits);
    if (!(t >= 0.0)) return 0u;
    const double top = (double)((1u << kBuildAxisBits) - 1u);
    return (uint32_t)(t < top ? t : top);
}

// bits 0 .. 9 of x spread to every third bit
RPT_BUILD_FN uint32_t build_spread3(uint32_t x)
{
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// The key of a triangle: Morton code of the quantised centroid (x in the highest bit of each triple), then the flattened index.
RPT_BUILD_FN uint64_t build_key(const float* cent, const float* lo, const float* hi, uint32_t flat_index)
{
    const uint32_t m = (build_spread3(build_quantise(cent[0], lo[0], hi[0])) << 2) | (build_spread3(build_quantise(cent[1], lo[1], hi[1])) << 1) |
                       build_spread3(build_quantise(cent[2], lo[2], hi[2]));
    return ((uint64_t)m << kBuildIndexBits) | (uint64_t)(flat_index & ((1u << kBuildIndexBits) - 1u));
}

// What the subtree of a child of a node at depth `depth` can hold (host_bvh.h's rule).  depth < kBvhMaxDepth.
RPT_BUILD_FN uint64_t build_child_capacity(uint32_t depth) { return (uint64_t)kBvhLeafMax << (kBvhMaxDepth - depth - 1u); }

// Where the node over the sorted slots [b, e) at depth `depth` splits: b < mid < e.  e - b >= 2, depth < kBvhMaxDepth, the keys
// ascend strictly.  The first slot whose key has the highest bit set in which keys[b] and keys[e - 1] differ (every key of the
// range shares the bits above it, so that bit is 0 up to the split and 1 from it on: a binary search of at most 32 steps) —
// unless a side would exceed its capacity: then the middle position.
RPT_BUILD_FN uint32_t build_split(const uint64_t* keys, uint32_t b, uint32_t e, uint32_t depth)
{
    const uint32_t middle = b + (e - b) / 2u;
    const uint64_t diff = keys[b] ^ keys[e - 1u];
    if (diff == 0u) return middle;                                  // (equal keys do not happen; the middle keeps every bound)
    const uint64_t bit = 1ull << (63 - __builtin_clzll(diff));
    uint32_t lo = b, hi = e - 1u;                                   // keys[lo] has the bit clear, keys[hi] has it set
    for (int step = 0; step < 32 && hi - lo > 1u; ++step) {
        const uint32_t m = lo + (hi - lo) / 2u;
        if (keys[m] & bit) hi = m; else lo = m;
    }
    const uint64_t cap = build_child_capacity(depth);
    if ((uint64_t)(hi - b) > cap || (uint64_t)(e - hi) > cap) return middle;
    return hi;
}

// A child of `count` triangles at depth `child_depth` is a leaf when it is small enough, and at the last depth (where the capacity
// rule has left it at most kBvhLeafMax).
RPT_BUILD_FN bool build_child_is_leaf(uint32_t count, uint32_t child_depth, uint32_t leaf_target)
{
    return count <= leaf_target || child_depth >= kBvhMaxDepth;
}

// The build's tables on a device besides the refit's (DevState::build, one allocation): the keys and their slots, in and out of the
// sort; the .w words and vertex indices of the slots on their way into the new order; per node its slot range and split; per child of
// the level being built whether it is an interior node, and the prefix sum of that; the levels' first nodes and counts, then the
// status word; the centroids' bounds; the sort's and the scan's temporary storage (sized by their query calls).
struct BuildLayout {
    size_t off_keys_in = 0, off_keys_out = 0, off_vals_in = 0, off_vals_out = 0, off_gather = 0, off_range = 0, off_mid = 0, off_flags = 0,
           off_offsets = 0, off_levels = 0, off_bounds = 0, off_temp = 0, total = 0;
    BuildLayout(uint32_t n_slots, uint32_t max_nodes, uint32_t max_level, size_t temp_bytes)
    {
        const auto round256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
        off_keys_out = round256(8 * (size_t)n_slots);
        off_vals_in = off_keys_out + round256(8 * (size_t)n_slots);
        off_vals_out = off_vals_in + round256(4 * (size_t)n_slots);
        off_gather = off_vals_out + round256(4 * (size_t)n_slots);
        off_range = off_gather + round256(24 * (size_t)n_slots);
        off_mid = off_range + round256(8 * (size_t)max_nodes);
        off_flags = off_mid + round256(4 * (size_t)max_nodes);
        off_offsets = off_flags + round256(8 * (size_t)max_level);
        off_levels = off_offsets + round256(8 * (size_t)max_level);
        off_bounds = off_levels + 256;
        off_temp = off_bounds + 256;
        total = off_temp + round256(temp_bytes);
    }
};
// off_levels: kBuildLevelWords dwords — level k's first node at [k], its node count at [32 + k] (k <= kBvhMaxDepth), the status at [63]
constexpr uint32_t kBuildLevelCount = 32, kBuildStatus = 63, kBuildLevelWords = 64;
constexpr uint32_t kBuildStatusTooDeep = 1u, kBuildStatusNodes = 2u;      // a node of the last level keeps more than a leaf holds; a node index beyond the table

// The most interior nodes a hierarchy over n_slots triangles has: every leaf holds a triangle and every interior node two children.
inline uint32_t build_max_nodes(uint32_t n_slots) { return n_slots > 1u ? n_slots - 1u : 1u; }
// ... and the most of them at depth k
inline uint32_t build_level_bound(uint32_t n_slots, uint32_t k)
{
    const uint32_t most = build_max_nodes(n_slots);
    return k < 31u && (1u << k) < most ? (1u << k) : most;
}

// ---- the topology step on the host: what k_build.hip's two kernels per level compute, statement for statement --------------------
struct BuildTopology {
    std::vector<uint32_t> child;               // 2 per interior node: host_bvh.h's child words
    std::vector<uint32_t> level_first;         // n_levels + 1 entries (host_refit.h, RefitPlan)
    uint32_t depth = 0;                        // of the deepest leaf
    uint32_t status = 0;
};

// One node of a level, first half (bvhbuild_split_kernel): its split, and which children become interior nodes.
RPT_BUILD_FN void build_node_split(const uint64_t* keys, uint32_t b, uint32_t e, uint32_t depth, uint32_t leaf_target, uint32_t* mid, uint32_t* interior)
{
    if (depth == 0u && e - b <= kBvhLeafMax) {                      // a scene of one leaf: beside an empty child (host_bvh.h)
        *mid = e;
        interior[0] = interior[1] = 0u;
        return;
    }
    const uint32_t m = build_split(keys, b, e, depth);
    *mid = m;
    interior[0] = build_child_is_leaf(m - b, depth + 1u, leaf_target) ? 0u : 1u;
    interior[1] = build_child_is_leaf(e - m, depth + 1u, leaf_target) ? 0u : 1u;
}

// ... second half (bvhbuild_emit_kernel): the child words.  `next[c]`: the node index of child c if it is an interior node.
RPT_BUILD_FN void build_node_children(uint32_t b, uint32_t mid, uint32_t e, const uint32_t* interior, const uint32_t* next, uint32_t* child, uint32_t* status)
{
    const uint32_t from[2] = {b, mid}, to[2] = {mid, e};
    for (int c = 0; c < 2; ++c) {
        const uint32_t count = to[c] - from[c];
        if (interior[c]) { child[c] = next[c]; continue; }
        if (count > kBvhLeafMax) { *status |= kBuildStatusTooDeep; child[c] = kBvhLeaf; continue; }     // (the capacity rule excludes it)
        child[c] = kBvhLeaf | (count << kBvhCountShift) | (count ? from[c] : 0u);
    }
}

// The hierarchy's shape over `n` sorted keys: 1 <= n <= kBvhMaxTriangles.  At most kBvhMaxDepth levels, as the device's host loop.
inline void build_topology(const uint64_t* keys, uint32_t n, uint32_t leaf_target, BuildTopology& out)
{
    out = BuildTopology();
    struct Range { uint32_t b, e; };
    std::vector<Range> level(1, Range{0u, n}), below;
    uint32_t first = 0;
    out.level_first.push_back(0u);
    for (uint32_t depth = 0; depth < kBvhMaxDepth && !level.empty(); ++depth) {
        const uint32_t count = (uint32_t)level.size(), next_first = first + count;
        std::vector<uint32_t> mid(count), interior(2 * (size_t)count), offset(2 * (size_t)count);
        for (uint32_t j = 0; j < count; ++j) build_node_split(keys, level[j].b, level[j].e, depth, leaf_target, &mid[j], &interior[2 * (size_t)j]);
        uint32_t sum = 0;
        for (size_t k = 0; k < interior.size(); ++k) { offset[k] = sum; sum += interior[k]; }      // the exclusive prefix sum
        below.assign(sum, Range{0u, 0u});
        out.child.resize(2 * (size_t)next_first);
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t next[2] = {next_first + offset[2 * (size_t)j], next_first + offset[2 * (size_t)j + 1]};
            build_node_children(level[j].b, mid[j], level[j].e, &interior[2 * (size_t)j], next, &out.child[2 * (size_t)(first + j)], &out.status);
            if (interior[2 * (size_t)j]) below[offset[2 * (size_t)j]] = Range{level[j].b, mid[j]};
            if (interior[2 * (size_t)j + 1]) below[offset[2 * (size_t)j + 1]] = Range{mid[j], level[j].e};
        }
        first = next_first;
        out.level_first.push_back(first);
        out.depth = depth + 1u;
        level.swap(below);
    }
    if (!level.empty()) out.status |= kBuildStatusTooDeep;         // (nodes left for a level the walk's stack does not have)
}

}  // namespace rpthost
