// build_harness.cpp — csrc/host_build.h on the host, for tests/test_mesh_rebuild_host.py (g++ -fsanitize=address,undefined): the split
// rule and the whole topology step the device build runs (k_build.hip compiles the same text), over sorted key arrays that press on
// the depth rule, and the key's quantisation at the edges of f32.
//
//   build_harness topology <family> <n> <leaf_target> ...   one line per case: "<family> <n> leaf <t>: nodes N levels L deepest D OK"
//   build_harness keys                                      "keys OK"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../rust-pathtracer_amd/csrc/host_build.h"

using namespace rpthost;

#define REQUIRE(cond, ...)                                                   \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);          \
            printf(__VA_ARGS__);                                             \
            printf("\n");                                                    \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint64_t key_of(uint32_t morton, uint32_t index) { return ((uint64_t)morton << kBuildIndexBits) | index; }

// sorted, unique keys of a family
static std::vector<uint64_t> family(const std::string& what, uint32_t n)
{
    std::vector<uint64_t> k;
    std::mt19937_64 rng(12345u + n);
    if (what == "random") {                    // random cells, every index once
        for (uint32_t i = 0; i < n; ++i) k.push_back(key_of((uint32_t)rng() & 0x3FFFFFFFu, i));
    } else if (what == "clustered") {          // a few thousand cells only: long runs that the index bits split
        for (uint32_t i = 0; i < n; ++i) k.push_back(key_of(((uint32_t)rng() % 3000u) * 357913u, i));
    } else if (what == "equal_morton") {       // a mesh collapsed to a point
        for (uint32_t i = 0; i < n; ++i) k.push_back(key_of(0x2AAAAAAAu, i));
    } else if (what == "diagonal_chain") {     // centroids at 2^-i (1, 1, 1): cell 2^(10 - i) per axis, several triangles each; then a dense cluster
        uint32_t index = 0;
        for (uint32_t i = 0; i <= 40u && index < n; ++i) {
            const uint32_t q = i <= 10u ? (1023u >> i) : 0u;
            const uint32_t m = (build_spread3(q) << 2) | (build_spread3(q) << 1) | build_spread3(q);
            for (uint32_t r = 0; r < 5u && index < n; ++r) k.push_back(key_of(m, index++));
        }
        while (index < n) { k.push_back(key_of(0x3FFFFFFFu - (uint32_t)(rng() % 4096u), index)); ++index; }
    } else if (what == "bit_chain") {          // one key per bit of the whole key, most chains a Morton split can make: 56 levels without the rule
        for (uint32_t b = 0; b < kBuildKeyBits && k.size() < n; ++b) k.push_back(1ull << b);
        for (uint32_t i = 0; k.size() < n; ++i) k.push_back(key_of(0x3FFFFFFFu, 3u + 5u * i));
    } else if (what == "sparse_index") {       // one cell, indices 2^b and their neighbours
        for (uint32_t b = 0; b < kBuildIndexBits && k.size() < n; ++b) k.push_back(key_of(77u, 1u << b));
        for (uint32_t i = 0; k.size() < n; ++i) k.push_back(key_of(77u, (1u << 25) + 3u + 2u * i));
    } else {
        REQUIRE(false, "unknown family %s", what.c_str());
    }
    std::sort(k.begin(), k.end());
    k.erase(std::unique(k.begin(), k.end()), k.end());
    REQUIRE(k.size() == n, "%s: %zu unique keys of %u", what.c_str(), k.size(), n);
    return k;
}

static void check_topology(const std::string& what, uint32_t n, uint32_t leaf_target)
{
    const std::vector<uint64_t> keys = family(what, n);
    BuildTopology t;
    build_topology(keys.data(), n, leaf_target, t);
    REQUIRE(t.status == 0u, "status %u", t.status);
    const uint32_t n_nodes = (uint32_t)(t.child.size() / 2u), n_levels = (uint32_t)t.level_first.size() - 1u;
    REQUIRE(n_nodes >= 1u && n_nodes <= build_max_nodes(n), "%u nodes for %u triangles", n_nodes, n);
    REQUIRE(n_levels >= 1u && n_levels <= kBvhMaxDepth && t.depth == n_levels, "%u levels, depth %u", n_levels, t.depth);
    REQUIRE(t.level_first[0] == 0u && t.level_first[n_levels] == n_nodes, "level_first ends at %u of %u", t.level_first[n_levels], n_nodes);
    for (uint32_t k = 0; k < n_levels; ++k) {
        REQUIRE(t.level_first[k] < t.level_first[k + 1u], "level %u is empty", k);
        REQUIRE(t.level_first[k + 1u] - t.level_first[k] <= build_level_bound(n, k), "level %u holds more than its bound", k);
    }
    // every node once, a parent below its children, a node's level one below its parent's; every slot in exactly one leaf, in order
    std::vector<uint32_t> depth_of(n_nodes, 0xFFFFFFFFu);
    std::vector<uint8_t> covered(n, 0);
    depth_of[0] = 0;
    uint32_t deepest = 0, n_leaves = 0;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        REQUIRE(depth_of[i] != 0xFFFFFFFFu, "node %u has no parent below it", i);
        REQUIRE(i >= t.level_first[depth_of[i]] && i < t.level_first[depth_of[i] + 1u], "node %u is not in level %u's range", i, depth_of[i]);
        for (int c = 0; c < 2; ++c) {
            const uint32_t ch = t.child[2u * (size_t)i + c];
            if (ch & kBvhLeaf) {
                const uint32_t cnt = (ch >> kBvhCountShift) & 15u, first = ch & kBvhSlotMask;
                if (cnt == 0u) { REQUIRE(n <= kBvhLeafMax && i == 0u && c == 1 && ch == kBvhLeaf, "an empty child at node %u", i); continue; }
                REQUIRE(cnt <= kBvhLeafMax && (uint64_t)first + cnt <= n, "leaf %u + %u", first, cnt);
                for (uint32_t s = first; s < first + cnt; ++s) { REQUIRE(!covered[s], "slot %u in two leaves", s); covered[s] = 1; }
                deepest = std::max(deepest, depth_of[i] + 1u);
                ++n_leaves;
            } else {
                REQUIRE(ch > i && ch < n_nodes && depth_of[ch] == 0xFFFFFFFFu, "node %u's child %u", i, ch);
                depth_of[ch] = depth_of[i] + 1u;
            }
        }
    }
    for (uint32_t s = 0; s < n; ++s) REQUIRE(covered[s], "slot %u in no leaf", s);
    REQUIRE(deepest <= kBvhMaxDepth && deepest == t.depth, "deepest leaf %u, depth %u", deepest, t.depth);
    if (n <= kBvhLeafMax) REQUIRE(n_nodes == 1u && t.child[0] == (kBvhLeaf | (n << kBvhCountShift)) && t.child[1] == kBvhLeaf, "one leaf beside an empty child");
    // the same keys once more: the same shape
    BuildTopology again;
    build_topology(keys.data(), n, leaf_target, again);
    REQUIRE(again.child == t.child && again.level_first == t.level_first, "two builds differ");
    printf("%s %u leaf %u: nodes %u levels %u deepest %u leaves %u OK\n", what.c_str(), n, leaf_target, n_nodes, n_levels, deepest, n_leaves);
}

// depth of the pure highest-differing-bit splits over [b, e) with leaves of at most kBvhLeafMax: what the rule is there against
static uint32_t morton_depth(const std::vector<uint64_t>& keys, uint32_t b, uint32_t e, uint32_t depth)
{
    if (e - b <= kBvhLeafMax) return depth;
    const uint64_t bit = 1ull << (63 - __builtin_clzll(keys[b] ^ keys[e - 1u]));
    uint32_t m = b;
    while (!(keys[m] & bit)) ++m;
    return std::max(morton_depth(keys, b, m, depth + 1u), morton_depth(keys, m, e, depth + 1u));
}

static void check_keys()
{
    const float big = 0x1p60f, inf = INFINITY, nan = NAN;
    // every finite input, and what a reduction over odd boxes could hand over, gives a cell
    const float cs[] = {0.0f, -0.0f, 1.0f, -1.0f, big, -big, FLT_MAX, -FLT_MAX, FLT_MIN, 1e-45f, inf, -inf, nan};
    for (float c : cs)
        for (float lo : cs)
            for (float hi : cs) REQUIRE(build_quantise(c, lo, hi) < 1024u, "quantise(%g, %g, %g)", c, lo, hi);
    REQUIRE(build_quantise(3.0f, 3.0f, 3.0f) == 0u, "zero extent");
    REQUIRE(build_quantise(FLT_MAX, -FLT_MAX, FLT_MAX) == 1023u && build_quantise(-FLT_MAX, -FLT_MAX, FLT_MAX) == 0u, "an extent beyond f32");
    REQUIRE(build_quantise(0.0f, -FLT_MAX, FLT_MAX) == 512u, "the middle of an extent beyond f32");
    REQUIRE(build_quantise(big, -big, big) == 1023u && build_quantise(0.0f, -big, big) == 512u && build_quantise(-big, -big, big) == 0u, "2^60");
    REQUIRE(build_quantise(1.0f, 0.0f, inf) == 0u && build_quantise(nan, 0.0f, 1.0f) == 0u && build_quantise(0.5f, nan, 1.0f) == 0u, "not numbers");
    REQUIRE(build_quantise(0.25f, 0.0f, 1.0f) == 256u && build_quantise(1.0f, 0.0f, 1.0f) == 1023u, "the unit interval");
    // the key: x in the highest bit of each triple, the index below
    const float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f};
    const float cx[3] = {1.0f, 0.0f, 0.0f}, cz[3] = {0.0f, 0.0f, 1.0f}, call[3] = {1.0f, 1.0f, 1.0f};
    REQUIRE(build_key(cx, lo, hi, 5u) == ((0x24924924ull << kBuildIndexBits) | 5u), "x");
    REQUIRE(build_key(cz, lo, hi, 0u) == (0x09249249ull << kBuildIndexBits), "z");
    REQUIRE(build_key(call, lo, hi, (1u << 26) - 1u) == (1ull << kBuildKeyBits) - 1u, "the largest key");
    REQUIRE(kBuildKeyBits == 56u && kBvhMaxTriangles == (1u << kBuildIndexBits) && kBuildLeafTarget >= 1u && kBuildLeafTarget <= kBvhLeafMax, "the constants");
    // the chain over every key bit does exceed the walk's stack without the rule (26 index bits alone cannot, with leaves of 8)
    {
        const std::vector<uint64_t> k = family("bit_chain", 5000u);
        REQUIRE(morton_depth(k, 0, 5000u, 0) > 40u, "bit_chain is not deep");
    }
    // the split: the first key with the highest differing bit set, or the middle
    const uint64_t ks[] = {1, 2, 3, 8, 9, 100, 101, 102, 103, 104};
    REQUIRE(build_split(ks, 0, 10, 0) == 5u && build_split(ks, 0, 5, 3) == 3u && build_split(ks, 5, 10, 3) == 9u, "splits");
    REQUIRE(build_split(ks, 0, 10, kBvhMaxDepth - 1u) == 5u, "the middle at the last depth");
    std::vector<uint64_t> lop(40);
    for (uint32_t i = 0; i < 40u; ++i) lop[i] = i == 39u ? (1ull << 40) : i;
    REQUIRE(build_split(lop.data(), 0, 40, 0) == 39u && build_split(lop.data(), 0, 40, 22) == 20u, "a lopsided split gives way to the middle");
    printf("keys OK\n");
}

int main(int argc, char** argv)
{
    if (argc >= 2 && std::string(argv[1]) == "keys") { check_keys(); return 0; }
    if (argc >= 5 && std::string(argv[1]) == "topology" && (argc - 2) % 3 == 0) {
        for (int i = 2; i + 2 < argc; i += 3) check_topology(argv[i], (uint32_t)strtoul(argv[i + 1], nullptr, 10), (uint32_t)strtoul(argv[i + 2], nullptr, 10));
        return 0;
    }
    fprintf(stderr, "usage: build_harness topology <family> <n> <leaf_target> ... | keys\n");
    return 2;
}
