// host_bvh.h — the bounding volume hierarchy of mesh scenes (include/rpt.h, "triangle meshes"), built on the host at upload.  Plain
// C++ with no HIP type in it, like host_grid.h: host_upload.h includes it, and tests/test_mesh_host.py compiles it alone with
// g++ -fsanitize=address,undefined (tests/bvh_harness.cpp).  Single-threaded, so the same triangles give the same bytes.
//
// A binary tree, binned SAH (16 bins per axis over the centroids).  An interior node holds the boxes of its two children, so the
// traversal (dev_scene_mesh.h) orders them nearer first from one 64-byte record.  A child is an interior node's index or a LEAF: up
// to kBvhLeafMax triangles, contiguous in the device's triangle table (which is in leaf order).  Depth is bounded by construction:
// no leaf lies deeper than kBvhMaxDepth levels below the root — the traversal's stack has that many entries — because a node at
// depth k keeps at most kBvhLeafMax * 2^(kBvhMaxDepth - k) triangles: where the SAH split (or no split: identical centroids) would
// break that, the node is split at the median of its centroids along the widest axis (ties by triangle index), which halves it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rpthost {

constexpr uint32_t kBvhMaxDepth = 24;          // == dev_scene_mesh.h kMeshStack
constexpr uint32_t kBvhLeafMax = 8;            // triangles per leaf, at most
constexpr uint32_t kBvhLeafTarget = 2;         // ... and a node of this many or fewer is always a leaf
constexpr uint32_t kBvhBins = 16;
constexpr uint32_t kBvhMaxTriangles = 1u << 26;    // include/rpt.h RPT_MESH_MAX_TRIANGLES; kBvhLeafMax << kBvhMaxDepth = 2^27 fit
// child word: interior node index (< 2^27), or kBvhLeaf | count << kBvhCountShift | first triangle slot; kBvhLeaf alone (count 0) is
// an empty child (its box is lo = +inf, hi = -inf; the slab test lets a ray with no zero direction component into it, and the walk
// then pops the next entry: it holds no triangle)
constexpr uint32_t kBvhLeaf = 0x80000000u;
constexpr uint32_t kBvhCountShift = 27;
constexpr uint32_t kBvhSlotMask = (1u << kBvhCountShift) - 1u;

// 64 bytes: the two children's boxes, then the two child words.  (Four float4 on the device.)
struct BvhNode {
    float lbox[6];                             // lo xyz, hi xyz
    float rbox[6];
    uint32_t child[2];
    uint32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode is 64 bytes");

struct HostBvh {
    std::vector<BvhNode> nodes;                // nodes[0] is the root (always an interior node)
    std::vector<uint32_t> order;               // triangle slot -> flattened triangle index
    uint32_t depth = 0;                        // of the deepest leaf (root's children: 1)
};

namespace bvh_detail {

struct Box {
    float lo[3], hi[3];
    void empty() { for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; } }
    void grow(const Box& b) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
    void grow(const float* p) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
    double area() const
    {
        if (!(lo[0] <= hi[0])) return 0.0;
        const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }
};

// The box a node stores: the exact box of its triangles' boxes (triangle_box); the traversal widens it per ray (dev_scene_mesh.h,
// box_enter).
inline void pad_box(const Box& b, float* out)
{
    for (int a = 0; a < 3; ++a) { out[a] = b.lo[a]; out[3 + a] = b.hi[a]; }
}

// A triangle's box: its vertices, and the box of include/rpt.h's point check, a + [min(0, e1, e2), max(0, e1, e2)] in f32 with
// e1 = b - a, e2 = c - a (which can differ from the vertices' box by an ulp).
inline Box triangle_box(const float* v)
{
    Box x;
    x.empty();
    for (int k = 0; k < 3; ++k) x.grow(&v[3 * k]);
    for (int a = 0; a < 3; ++a) {
        const float e1 = v[3 + a] - v[a], e2 = v[6 + a] - v[a];
        const float lo = v[a] + std::min(std::min(0.0f, e1), e2), hi = v[a] + std::max(std::max(0.0f, e1), e2);
        x.lo[a] = std::min(x.lo[a], lo);
        x.hi[a] = std::max(x.hi[a], hi);
    }
    return x;
}

struct Builder {
    const float* tri;                          // 9 floats per flattened triangle
    std::vector<Box> tbox;
    std::vector<float> cent;                   // 3 per triangle
    std::vector<uint32_t> idx;                 // the permutation being partitioned
    HostBvh* out;

    Box range_box(uint32_t b, uint32_t e) const
    {
        Box x;
        x.empty();
        for (uint32_t i = b; i < e; ++i) x.grow(tbox[idx[i]]);
        return x;
    }

    // child word for [b, e) at depth `depth` (1 = the root's child)
    uint32_t build(uint32_t b, uint32_t e, uint32_t depth, float* box_out)
    {
        const Box bx = range_box(b, e);
        pad_box(bx, box_out);
        const uint32_t n = e - b;
        if (n <= kBvhLeafTarget || depth >= kBvhMaxDepth) return leaf(b, n, depth);     // (at kBvhMaxDepth n <= kBvhLeafMax: the capacity rule)
        uint32_t mid = 0;
        // the capacity of each child: what its subtree can hold with leaves of at most kBvhLeafMax at depth <= kBvhMaxDepth
        const uint64_t cap = (uint64_t)kBvhLeafMax << (kBvhMaxDepth - depth - 1u);
        const double leaf_cost = (double)n;
        double split_cost = 0.0;
        const bool sah = sah_split(b, e, bx, mid, split_cost);
        if (n <= kBvhLeafMax && (!sah || leaf_cost <= split_cost)) return leaf(b, n, depth);
        if (!sah || (uint64_t)(mid - b) > cap || (uint64_t)(e - mid) > cap) mid = median_split(b, e);
        const uint32_t me = (uint32_t)out->nodes.size();
        out->nodes.push_back(BvhNode{});
        BvhNode nd;
        memset(&nd, 0, sizeof(nd));
        nd.child[0] = build(b, mid, depth + 1u, nd.lbox);
        nd.child[1] = build(mid, e, depth + 1u, nd.rbox);
        out->nodes[me] = nd;
        return me;
    }

    uint32_t leaf(uint32_t b, uint32_t n, uint32_t depth)
    {
        out->depth = std::max(out->depth, depth);
        return kBvhLeaf | (n << kBvhCountShift) | b;
    }

    // Binned SAH over the centroids of [b, e): false when every centroid falls into one bin on every axis.
    bool sah_split(uint32_t b, uint32_t e, const Box& bx, uint32_t& mid, double& cost)
    {
        (void)bx;
        Box cb;
        cb.empty();
        for (uint32_t i = b; i < e; ++i) cb.grow(&cent[3 * idx[i]]);
        double best = INFINITY;
        int best_axis = -1;
        uint32_t best_bin = 0;
        float scale[3];
        for (int a = 0; a < 3; ++a) {
            const float ext = cb.hi[a] - cb.lo[a];
            scale[a] = ext > 0.0f ? (float)kBvhBins / ext : 0.0f;
            if (!(ext > 0.0f) || !std::isfinite(scale[a])) continue;
            Box bins[kBvhBins];
            uint32_t count[kBvhBins] = {};
            for (uint32_t k = 0; k < kBvhBins; ++k) bins[k].empty();
            for (uint32_t i = b; i < e; ++i) {
                const uint32_t k = bin_of(cent[3 * idx[i] + a], cb.lo[a], scale[a]);
                bins[k].grow(tbox[idx[i]]);
                count[k] += 1;
            }
            double right_area[kBvhBins];
            uint32_t right_n[kBvhBins];
            Box acc;
            acc.empty();
            uint32_t acc_n = 0;
            for (uint32_t k = kBvhBins - 1u; k > 0; --k) {
                acc.grow(bins[k]); acc_n += count[k];
                right_area[k] = acc.area(); right_n[k] = acc_n;
            }
            acc.empty();
            acc_n = 0;
            for (uint32_t k = 1; k < kBvhBins; ++k) {       // split between bin k - 1 and bin k
                acc.grow(bins[k - 1]); acc_n += count[k - 1];
                if (acc_n == 0 || right_n[k] == 0) continue;
                const double c = acc.area() * acc_n + right_area[k] * right_n[k];
                if (c < best) { best = c; best_axis = a; best_bin = k; }
            }
        }
        if (best_axis < 0) return false;
        const double parent = range_box(b, e).area();
        cost = parent > 0.0 ? 0.125 + best / parent : best;      // (traversal step : triangle test = 1 : 8)
        const int a = best_axis;
        const float lo = cb.lo[a], sc = scale[a];
        const uint32_t* first = idx.data() + b;
        std::vector<uint32_t> left, right;
        for (const uint32_t* p = first; p != idx.data() + e; ++p)
            (bin_of(cent[3 * *p + a], lo, sc) < best_bin ? left : right).push_back(*p);
        std::copy(left.begin(), left.end(), idx.begin() + b);
        std::copy(right.begin(), right.end(), idx.begin() + b + left.size());
        mid = b + (uint32_t)left.size();
        return true;
    }

    static uint32_t bin_of(float c, float lo, float scale)
    {
        const float f = (c - lo) * scale;
        const uint32_t k = f > 0.0f ? (uint32_t)f : 0u;
        return k < kBvhBins ? k : kBvhBins - 1u;
    }

    // Median of the centroids along the widest centroid axis; ties (and identical centroids) by triangle index: a total order.
    uint32_t median_split(uint32_t b, uint32_t e)
    {
        Box cb;
        cb.empty();
        for (uint32_t i = b; i < e; ++i) cb.grow(&cent[3 * idx[i]]);
        int a = 0;
        for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[a] - cb.lo[a]) a = k;
        const uint32_t mid = b + (e - b) / 2u;
        const float* c = cent.data();
        std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [c, a](uint32_t x, uint32_t y) {
            return c[3 * x + a] < c[3 * y + a] || (c[3 * x + a] == c[3 * y + a] && x < y);
        });
        // nth_element leaves each side in an order that depends on the library: sort both halves by the same key
        auto key = [c, a](uint32_t x, uint32_t y) { return c[3 * x + a] < c[3 * y + a] || (c[3 * x + a] == c[3 * y + a] && x < y); };
        std::sort(idx.begin() + b, idx.begin() + mid, key);
        std::sort(idx.begin() + mid, idx.begin() + e, key);
        return mid;
    }
};

}  // namespace bvh_detail

// Build the hierarchy over `n` triangles of 9 finite floats each (a, b, c).  1 <= n <= kBvhMaxTriangles.
inline void build_bvh(const float* tri, uint32_t n, HostBvh& out)
{
    using namespace bvh_detail;
    out.nodes.clear();
    out.order.clear();
    out.depth = 0;
    Builder bd;
    bd.tri = tri;
    bd.out = &out;
    bd.tbox.resize(n);
    bd.cent.resize(3 * (size_t)n);
    bd.idx.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        Box& x = bd.tbox[i];
        x = triangle_box(&tri[9 * (size_t)i]);
        for (int a = 0; a < 3; ++a) bd.cent[3 * (size_t)i + a] = x.lo[a] * 0.5f + x.hi[a] * 0.5f;
        bd.idx[i] = i;
    }
    out.nodes.push_back(BvhNode{});
    BvhNode root;
    memset(&root, 0, sizeof(root));
    if (n <= kBvhLeafMax) {                    // one leaf beside an empty child
        root.child[0] = bd.build(0, n, 1u, root.lbox);
        for (int a = 0; a < 3; ++a) { root.rbox[a] = INFINITY; root.rbox[3 + a] = -INFINITY; }
        root.child[1] = kBvhLeaf;
    } else {
        const uint32_t mid0 = [&]() {
            uint32_t mid = 0;
            double cost = 0.0;
            Box bx = bd.range_box(0, n);
            const uint64_t cap = (uint64_t)kBvhLeafMax << (kBvhMaxDepth - 1u);
            if (!bd.sah_split(0, n, bx, mid, cost) || (uint64_t)mid > cap || (uint64_t)(n - mid) > cap) mid = bd.median_split(0, n);
            return mid;
        }();
        root.child[0] = bd.build(0, mid0, 1u, root.lbox);
        root.child[1] = bd.build(mid0, n, 1u, root.rbox);
    }
    out.nodes[0] = root;
    out.order = bd.idx;
}

}  // namespace rpthost
