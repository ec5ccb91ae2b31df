// The host half of rpt_update_meshes (rust-pathtracer_amd/csrc/host_refit.h) on its own, for tests/test_mesh_update_host.py, which
// builds this file with g++ -fsanitize=address,undefined -ffp-contract=off.  Modes (first argument):
//   families <kind> <n> ...  for each input (tests/bvh_harness.cpp's families, as two meshes): build the hierarchy and the tables as
//             rpt_upload_scene does; refit_reference with the SAME vertices gives the build's rows and nodes byte for byte; with moved
//             vertices (a random displacement, every vertex collapsed to one point, everything scaled by 2^61) every row is {a, b - a,
//             c - a} of its moved triangle, every box the union of its children's boxes and its leaves' triangle_box, the .w words and
//             child words are untouched, empty children keep their empty box; the level order names every interior node once, every
//             child in a strictly deeper level than its parent, in at most kBvhMaxDepth levels
//   subnormal coordinates that differ by subnormal amounts give subnormal edge components, kept
//   errors    every error case of check_mesh_update: code, a message naming mesh and vertex, and a valid update accepted after each
//   rule      the 2^60 rule turns the walk off and on again, and looks at referenced vertices only
// Prints one "... OK" line per input or mode, or what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_refit.h"

using namespace rpthost;

static int g_fail = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);           \
            printf(__VA_ARGS__);                                             \
            printf("\n");                                                    \
            g_fail = 1;                                                      \
        }                                                                    \
    } while (0)

// tests/bvh_harness.cpp's inputs
static std::vector<float> make_input(const std::string& kind, uint32_t n)
{
    std::vector<float> t(9 * (size_t)n);
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    for (uint32_t i = 0; i < n; ++i) {
        float* v = &t[9 * (size_t)i];
        if (kind == "random") {
            const float c[3] = {u(rng) * 50.0f, u(rng) * 50.0f, u(rng) * 50.0f};
            for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + u(rng) * 0.5f;
        } else if (kind == "same_centroid") {
            const float a = u(rng), b = u(rng);
            const float p[9] = {1.0f + a, 2.0f + b, 3.0f, 1.0f - a, 2.0f - b, 3.0f, 1.0f, 2.0f, 3.0f};
            memcpy(v, p, sizeof(p));
        } else if (kind == "identical") {
            const float p[9] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
            memcpy(v, p, sizeof(p));
        } else if (kind == "line") {
            const float x = (float)(i % 1000) * 0.25f;
            const float p[9] = {x, 0.0f, 0.0f, x + 0.5f, 0.0f, 0.0f, x + 1.0f, 0.0f, 0.0f};
            memcpy(v, p, sizeof(p));
        } else {                                                    // "strip"
            const float x = ldexpf(1.0f, (int)(i % 200) - 100);
            const float p[9] = {x, 0.0f, 0.0f, x, 1.0f, 0.0f, x, 0.0f, 1.0f};
            memcpy(v, p, sizeof(p));
        }
    }
    return t;
}

// A mesh scene as far as the refit knows it: the descriptor's meshes, and the two tables as prepare_scene (host_upload.h) lays them out.
struct Scene {
    std::vector<std::vector<float>> verts;
    std::vector<std::vector<uint32_t>> idx;
    std::vector<rpt_mesh> meshes;
    rpt_scene_desc d = {};
    HostBvh bvh;
    std::vector<unsigned char> rows;
    RefitPlan plan;

    // `tri`: n triangles of 9 floats, cut into two meshes (the second takes the odd half); every triangle has its own three vertices,
    // listed in reverse so that no index equals its position
    void build(const std::vector<float>& tri, uint32_t n)
    {
        const uint32_t n0 = n / 2u;
        const uint32_t count[2] = {n0, n - n0};
        uint32_t first = 0;
        for (int m = 0; m < 2; ++m) {
            const uint32_t nv = 3u * count[m];
            std::vector<float> v(3 * (size_t)nv + 3);               // (one vertex more that no triangle uses)
            std::vector<uint32_t> ix(3 * (size_t)count[m]);
            for (uint32_t t = 0; t < count[m]; ++t)
                for (uint32_t c = 0; c < 3; ++c) {
                    const uint32_t at = nv - 1u - (3u * t + c);
                    memcpy(&v[3 * (size_t)at], &tri[9 * (size_t)(first + t) + 3 * c], 12);
                    ix[3 * (size_t)t + c] = at;
                }
            v[3 * (size_t)nv] = 7.0f; v[3 * (size_t)nv + 1] = 8.0f; v[3 * (size_t)nv + 2] = 9.0f;
            verts.push_back(v);
            idx.push_back(ix);
            first += count[m];
        }
        for (int m = 0; m < 2; ++m) meshes.push_back(rpt_mesh{(uint32_t)(verts[m].size() / 3), verts[m].data(), count[m], idx[m].data(), (uint32_t)m + 5u});
        d.n_meshes = 2;
        d.meshes = meshes.data();
        build_bvh(tri.data(), n, bvh);
        rows.assign(48 * (size_t)n, 0);
        for (uint32_t slot = 0; slot < n; ++slot) {                 // host_upload.h, prepare_scene
            const uint32_t i = bvh.order[slot];
            const float* v = &tri[9 * (size_t)i];
            float r[12] = {v[0], v[1], v[2], 0.0f, v[3] - v[0], v[4] - v[1], v[5] - v[2], 0.0f, v[6] - v[0], v[7] - v[1], v[8] - v[2], 0.0f};
            const uint32_t mat = i < n0 ? 5u : 6u;
            memcpy(&r[3], &i, 4);
            memcpy(&r[11], &mat, 4);
            memcpy(&rows[48 * (size_t)slot], r, sizeof(r));
        }
        build_refit_plan(&d, bvh, plan);
    }
};

static void refit(const Scene& s, const std::vector<float>& vertices, std::vector<unsigned char>& rows, std::vector<BvhNode>& nodes)
{
    std::vector<float> slot_box(6 * (size_t)s.plan.n_slots + 1);
    refit_reference(vertices.data(), s.plan.slot_vertex.data(), s.plan.n_slots, s.plan.level_nodes.data(), s.plan.level_first.data(),
                    s.plan.n_levels(), rows.data(), nodes.data(), slot_box.data());
}

// The box a child must hold, from the moved triangles alone (not from refit_slot / refit_node): a leaf's from triangle_box of its
// slots' gathered vertices, an interior child's from that node's two stored boxes, which are checked in turn.
struct Checker {
    const Scene& s;
    const std::vector<float>& vertices;
    const std::vector<unsigned char>& rows;
    const std::vector<BvhNode>& nodes;
    uint32_t visited = 0, empties = 0;

    void gather(uint32_t slot, float* v) const
    {
        const size_t n = s.plan.n_slots;
        for (size_t c = 0; c < 3; ++c) memcpy(&v[3 * c], &vertices[3 * (size_t)s.plan.slot_vertex[c * n + slot]], 12);
    }
    void child(uint32_t ch, const float* box)
    {
        using bvh_detail::Box;
        Box want;
        want.empty();
        if (ch & kBvhLeaf) {
            const uint32_t cnt = (ch >> kBvhCountShift) & 15u, first = ch & kBvhSlotMask;
            empties += cnt == 0u;
            for (uint32_t k = first; k < first + cnt; ++k) {
                float v[9];
                gather(k, v);
                want.grow(bvh_detail::triangle_box(v));
                const float r[9] = {v[0], v[1], v[2], v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[0], v[7] - v[1], v[8] - v[2]};
                for (size_t c = 0; c < 3; ++c)
                    CHECK(memcmp(&rows[48 * (size_t)k + 16 * c], &r[3 * c], 12) == 0, "slot %u row part %zu", k, c);
            }
        } else {
            const BvhNode& n = nodes[ch];
            visited += 1;
            Box l, r;
            memcpy(l.lo, n.lbox, 12); memcpy(l.hi, n.lbox + 3, 12); memcpy(r.lo, n.rbox, 12); memcpy(r.hi, n.rbox + 3, 12);
            want.grow(l);
            want.grow(r);
            child(n.child[0], n.lbox);
            child(n.child[1], n.rbox);
        }
        float w[6];
        bvh_detail::pad_box(want, w);
        CHECK(memcmp(w, box, 24) == 0, "child word 0x%x: box {%g %g %g %g %g %g}, want {%g %g %g %g %g %g}", ch, box[0], box[1], box[2], box[3],
              box[4], box[5], w[0], w[1], w[2], w[3], w[4], w[5]);
    }
};

static void check_levels(const Scene& s)
{
    const RefitPlan& p = s.plan;
    const uint32_t n = p.n_nodes;
    CHECK(p.n_levels() >= 1 && p.n_levels() <= kBvhMaxDepth, "%u levels", p.n_levels());
    CHECK(p.level_nodes.size() == n && p.level_first.front() == 0u && p.level_first.back() == n, "level offsets");
    std::vector<uint32_t> level_of(n, 0xFFFFFFFFu);
    for (uint32_t l = 0; l < p.n_levels(); ++l) {
        CHECK(p.level_first[l] <= p.level_first[l + 1], "offsets not monotonic");
        for (uint32_t k = p.level_first[l]; k < p.level_first[l + 1]; ++k) {
            const uint32_t node = p.level_nodes[k];
            CHECK(node < n && level_of[node] == 0xFFFFFFFFu, "node %u listed twice or out of range", node);
            if (node < n) level_of[node] = l;
        }
    }
    CHECK(level_of[0] == 0u, "the root is not level 0");
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(level_of[i] != 0xFFFFFFFFu, "node %u not listed", i);
        for (int c = 0; c < 2; ++c) {
            const uint32_t ch = s.bvh.nodes[i].child[c];
            if (!(ch & kBvhLeaf)) CHECK(ch < n && level_of[ch] > level_of[i], "child %u of %u is not deeper", ch, i);
        }
    }
}

static int families(int argc, char** argv)
{
    for (int i = 2; i + 1 < argc; i += 2) {
        const int before = g_fail;
        const std::string kind = argv[i];
        const uint32_t n = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        const std::vector<float> tri = make_input(kind, n);
        Scene s;
        s.build(tri, n);
        const RefitPlan& p = s.plan;
        CHECK(p.ok && p.n_slots == n && p.n_nodes == s.bvh.nodes.size() && p.n_meshes() == 2u, "plan sizes");
        check_levels(s);
        // the same vertices: the build's bytes
        std::vector<unsigned char> rows = s.rows;
        std::vector<BvhNode> nodes = s.bvh.nodes;
        for (unsigned char& b : rows) b = (unsigned char)(b ^ ((&b - rows.data()) % 16 < 12 ? 0x5A : 0));     // (garbage in every float part ...)
        for (BvhNode& nd : nodes) for (int k = 0; k < 6; ++k) { nd.lbox[k] = -1.0f; nd.rbox[k] = -2.0f; }    // (... and in every box)
        refit(s, p.vertices, rows, nodes);
        CHECK(rows == s.rows, "same vertices: rows differ");
        CHECK(memcmp(nodes.data(), s.bvh.nodes.data(), sizeof(BvhNode) * nodes.size()) == 0, "same vertices: nodes differ");
        // moved vertices
        std::mt19937 rng(99);
        std::uniform_real_distribution<float> u(-3.0f, 3.0f);
        for (int move = 0; move < 3; ++move) {
            std::vector<float> moved = p.vertices;
            for (size_t k = 0; k < moved.size(); ++k)
                moved[k] = move == 0 ? moved[k] + u(rng) : move == 1 ? (float)(k % 3) - 0.5f : std::fabs(moved[k]) < 0x1p60f ? moved[k] * 0x1p61f : moved[k];     // (finite)
            rows = s.rows;
            nodes = s.bvh.nodes;
            refit(s, moved, rows, nodes);
            Checker ck{s, moved, rows, nodes};
            ck.visited = 1;
            ck.child(nodes[0].child[0], nodes[0].lbox);
            ck.child(nodes[0].child[1], nodes[0].rbox);
            CHECK(ck.visited == p.n_nodes, "move %d: %u of %u nodes reached", move, ck.visited, p.n_nodes);
            CHECK((n <= kBvhLeafMax) == (ck.empties == 1u), "move %d: %u empty children", move, ck.empties);
            for (uint32_t slot = 0; slot < n; ++slot)
                for (size_t c = 0; c < 3; ++c)
                    CHECK(memcmp(&rows[48 * (size_t)slot + 16 * c + 12], &s.rows[48 * (size_t)slot + 16 * c + 12], 4) == 0, "move %d: slot %u .w word %zu changed", move, slot, c);
            for (uint32_t k = 0; k < p.n_nodes; ++k)
                CHECK(memcmp(nodes[k].child, s.bvh.nodes[k].child, 16) == 0, "move %d: node %u child words changed", move, k);
            if (move == 1 && n > kBvhLeafMax) {                     // every box is the one point
                const float pt[6] = {-0.5f, 0.5f, 1.5f, -0.5f, 0.5f, 1.5f};
                for (uint32_t k = 0; k < p.n_nodes; ++k) CHECK(memcmp(nodes[k].lbox, pt, 24) == 0 && memcmp(nodes[k].rbox, pt, 24) == 0, "collapsed: node %u", k);
            }
        }
        printf("%s %u: nodes %u levels %u %s\n", kind.c_str(), n, p.n_nodes, p.n_levels(), g_fail == before ? "OK" : "FAIL");
    }
    return g_fail;
}

static int subnormal()
{
    // a at the smallest normal number, b and c one and three units of the last place away: the edges are 2^-149 and 3 * 2^-149
    const float tiny = 0x1p-126f, ulp = 0x1p-149f;
    const std::vector<float> tri = {tiny, -tiny, 0.0f, tiny + ulp, -tiny, ulp, tiny, -tiny - 3.0f * ulp, -ulp,
                                    1.0f, 1.0f, 1.0f, 2.0f, 1.0f, 1.0f, 1.0f, 2.0f, 1.0f};
    Scene s;
    s.build(tri, 2);
    std::vector<unsigned char> rows(s.rows.size(), 0);
    std::vector<BvhNode> nodes = s.bvh.nodes;
    refit(s, s.plan.vertices, rows, nodes);
    uint32_t slot = 0;
    while (slot < 2u && s.bvh.order[slot] != 0u) ++slot;
    float r[12];
    memcpy(r, &rows[48 * (size_t)slot], 48);
    CHECK(r[4] == ulp && r[5] == 0.0f && r[6] == ulp, "e1 = {%a %a %a}", r[4], r[5], r[6]);
    CHECK(r[8] == 0.0f && r[9] == -3.0f * ulp && r[10] == -ulp, "e2 = {%a %a %a}", r[8], r[9], r[10]);
    CHECK(std::fpclassify(r[4]) == FP_SUBNORMAL && std::fpclassify(r[9]) == FP_SUBNORMAL, "flushed");
    printf("subnormal %s\n", g_fail ? "FAIL" : "OK");
    return g_fail;
}

static int errors()
{
    Scene s;
    s.build(make_input("random", 40), 40);                          // two meshes of 61 vertices (60 used)
    const RefitPlan& p = s.plan;
    std::vector<float> good0(s.verts[0]), good1(s.verts[1]);
    for (float& x : good0) x += 0.25f;
    std::vector<float> max_abs;
    std::string err;
    const auto valid = [&]() {
        const rpt_mesh_vertices ok[2] = {{1u, 61u, good1.data()}, {0u, 61u, good0.data()}};
        err.clear();
        CHECK(check_mesh_update(p, true, ok, 2, max_abs, err) == RPT_OK && err.empty() && max_abs.size() == 2u, "a valid update: %s", err.c_str());
    };
    const auto expect = [&](const char* what, bool mesh_scene, const rpt_mesh_vertices* ups, uint32_t n, int code, const char* needle) {
        err.clear();
        const int rc = check_mesh_update(p, mesh_scene, ups, n, max_abs, err);
        CHECK(rc == code, "%s: rc %d, want %d (%s)", what, rc, code, err.c_str());
        CHECK(err.rfind("rpt_update_meshes: ", 0) == 0 && err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", what, err.c_str(), needle);
        valid();
    };
    valid();
    rpt_mesh_vertices one = {0u, 61u, good0.data()};
    expect("NULL updates", true, nullptr, 1, RPT_ERR_INVALID_ARG, "updates is NULL");
    expect("no mesh scene", false, &one, 1, RPT_ERR_NO_SCENE, "scene with meshes");
    RefitPlan none;
    err.clear();
    CHECK(check_mesh_update(none, false, &one, 1, max_abs, err) == RPT_ERR_NO_SCENE, "an empty plan");
    one.mesh = 2u;
    expect("mesh out of range", true, &one, 1, RPT_ERR_INVALID_ARG, "mesh 2 out of range");
    const rpt_mesh_vertices twice[3] = {{1u, 61u, good1.data()}, {0u, 61u, good0.data()}, {1u, 61u, good1.data()}};
    expect("named twice", true, twice, 3, RPT_ERR_INVALID_ARG, "mesh 1 is named twice");
    one = {1u, 60u, good1.data()};
    expect("count", true, &one, 1, RPT_ERR_INVALID_ARG, "mesh 1: n_vertices 60 != the uploaded mesh's 61");
    one = {1u, 61u, nullptr};
    expect("NULL vertices", true, &one, 1, RPT_ERR_INVALID_ARG, "mesh 1: vertices is NULL");
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    for (float b : bad) {
        std::vector<float> v(good1);
        v[3 * 17 + 2] = b;
        one = {1u, 61u, v.data()};
        expect("non-finite", true, &one, 1, RPT_ERR_INVALID_ARG, "mesh 1 vertex 17 is not finite");
    }
    {   // an unreferenced vertex must be finite too: upload checks every vertex
        std::vector<float> v(good0);
        v[3 * 60] = NAN;
        one = {0u, 61u, v.data()};
        expect("non-finite, unused vertex", true, &one, 1, RPT_ERR_INVALID_ARG, "mesh 0 vertex 60 is not finite");
    }
    {   // the first fault answers
        std::vector<float> v(good0);
        v[0] = NAN;
        const rpt_mesh_vertices two[2] = {{0u, 61u, v.data()}, {9u, 61u, good1.data()}};
        expect("first fault", true, two, 2, RPT_ERR_INVALID_ARG, "mesh 0 vertex 0 is not finite");
    }
    printf("errors %s\n", g_fail ? "FAIL" : "OK");
    return g_fail;
}

static int rule()
{
    Scene s;
    s.build(make_input("random", 40), 40);
    const RefitPlan& p = s.plan;
    CHECK(refit_use_bvh(p.mesh_max_abs) && p.mesh_max_abs[0] > 1.0f && p.mesh_max_abs[0] < 60.0f, "the uploaded scene walks");
    std::vector<float> max_abs;
    std::string err;
    std::vector<float> v(s.verts[1]);
    v[3 * 5 + 1] = -0x1p61f;
    rpt_mesh_vertices one = {1u, 61u, v.data()};
    CHECK(check_mesh_update(p, true, &one, 1, max_abs, err) == RPT_OK, "%s", err.c_str());
    CHECK(max_abs[1] == 0x1p61f && max_abs[0] == p.mesh_max_abs[0] && !refit_use_bvh(max_abs), "beyond 2^60: the loop");
    RefitPlan q = p;
    q.mesh_max_abs = max_abs;                                       // (what rpt_update_meshes keeps)
    v[3 * 5 + 1] = 0x1p60f;
    CHECK(check_mesh_update(q, true, &one, 1, max_abs, err) == RPT_OK && max_abs[1] == 0x1p60f && refit_use_bvh(max_abs), "2^60 itself walks");
    rpt_mesh_vertices other = {0u, 61u, s.verts[0].data()};
    CHECK(check_mesh_update(q, true, &other, 1, max_abs, err) == RPT_OK && !refit_use_bvh(max_abs), "another mesh's update does not bring mesh 1 back");
    v = s.verts[1];
    v[3 * 60] = 0x1p100f;                                           // the vertex no triangle uses
    CHECK(check_mesh_update(q, true, &one, 1, max_abs, err) == RPT_OK && refit_use_bvh(max_abs) && max_abs[1] == p.mesh_max_abs[1], "an unused vertex does not count");
    printf("rule %s\n", g_fail ? "FAIL" : "OK");
    return g_fail;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "families") return families(argc, argv) ? 1 : 0;
    if (mode == "subnormal") return subnormal() ? 1 : 0;
    if (mode == "errors") return errors() ? 1 : 0;
    if (mode == "rule") return rule() ? 1 : 0;
    printf("usage: refit_harness families <kind> <n> ... | subnormal | errors | rule\n");
    return 2;
}
