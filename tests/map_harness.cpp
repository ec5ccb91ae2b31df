// map_harness.cpp — csrc/host_map.h's recipe, executed on the host (tests/test_mesh_map_host.py); a stand-alone program, so it may be
// built with -fsanitize=address,undefined and run as it is.
//
//   map_harness cut | nrm | mmap | emap    the feature's setter as capi.hip's set_mesh_maps and map_device run it, on host buffers:
//                                          memset and memcpy for the HIP calls, the header's plain-loop reference for the decode
//                                          launch.  After each call of a sequence, the tables equal, byte for byte, those one call
//                                          that names every ON mesh builds from nothing.
//   map_harness recipe                     the recipe's own rules: the stage's rounding and prefix, the error of a kept mesh that
//                                          the device holds nothing for.
//
// The scene: three meshes of 2, 1 and 3 triangles, all textured (mesh 2 CLAMP).  The calls:
//   1  meshes 0 (3 x 5) and 2 (1 x 1)     2  mesh 0 again, 2 x 9: mesh 2 moves down and is not named
//   3  mesh 0 OFF: mesh 2 moves to the front     4  mesh 1 only (a cutout: 33 x 1, a mask that ends inside a word; a map: 3 x 5)
//   5  meshes 1 and 2 OFF: no tables
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rust-pathtracer_amd/csrc/host_cut.h"
#include "../rust-pathtracer_amd/csrc/host_emap.h"
#include "../rust-pathtracer_amd/csrc/host_map.h"
#include "../rust-pathtracer_amd/csrc/host_mmap.h"
#include "../rust-pathtracer_amd/csrc/host_nrm.h"

using namespace rpthost;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

struct Scene {
    RefitPlan plan;
    TexPlan tex;
    LightPlan light;                  // no mesh is a light
    Scene()
    {
        plan.ok = true;
        plan.mesh_first = {0u, 4u, 7u, 12u};
        plan.tri_first = {0u, 2u, 3u, 6u};
        plan.mesh_material = {0u, 1u, 2u};
        plan.n_slots = 6;
        std::vector<TexImage> image(3);
        for (uint32_t m = 0; m < 3; ++m) { image[m].width = m + 1u; image[m].height = 2; image[m].wrap = m == 2 ? RPT_TEX_WRAP_CLAMP : RPT_TEX_WRAP_REPEAT; }
        build_tex_plan(plan, image, std::vector<float>(), tex);
    }
};

struct Spec {                         // one item of a call; width == 0: OFF
    uint32_t mesh, width, height;
};

// `bytes` bytes that differ from mesh to mesh and from size to size.
static std::vector<uint8_t> image_bytes(uint32_t mesh, size_t bytes)
{
    std::vector<uint8_t> v(bytes);
    uint32_t x = 2463534242u + 977u * mesh + (uint32_t)bytes;
    for (uint8_t& b : v) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; b = (uint8_t)(x >> 11); }
    return v;
}

// ---- the four features: the item, the checks, the plan, the constants, the reference of the decode, the descriptors -----------------
struct Cut {
    using Item = rpt_mesh_cutout;
    using Entry = CutMask;
    using Plan = CutPlan;
    static constexpr MapConsts k = {4, 1, 0};
    static constexpr uint32_t odd_w = 33, odd_h = 1;
    static std::vector<Entry>& entries(Plan& p) { return p.mask; }
    static Item item(const Spec& s, const uint8_t* src)
    {
        Item it;
        memset(&it, 0, sizeof(it));
        it.mesh = s.mesh; it.mode = s.width ? RPT_MESH_CUTOUT_ON : RPT_MESH_CUTOUT_OFF; it.width = s.width; it.height = s.height; it.alpha = src;
        it.threshold = s.width ? 100u + s.mesh : 0u;
        return it;
    }
    static int check(const Scene& sc, const Item* items, uint32_t n, const Plan& p, std::vector<Entry>& out, std::string& err)
    {
        return check_mesh_cutouts(sc.plan, true, sc.tex, sc.light, items, n, p.mask, out, err);
    }
    static void build(const Scene& sc, std::vector<Entry> e, Plan& p) { build_cut_plan(sc.plan, std::move(e), p); }
    static std::vector<MapNamed> named(const std::vector<Item>& items) { return map_named(items.data(), (uint32_t)items.size(), &Item::alpha); }
    static void decode(const Plan& p, uint32_t mesh, const uint8_t* staged, uint8_t* dst, uint32_t)
    {
        const Entry& c = p.mask[mesh];
        cut_mask_reference(staged, c.width, c.height, c.threshold, reinterpret_cast<uint32_t*>(dst));
    }
    static void descriptors(const Scene& sc, const Plan& p, uint8_t* base)
    {
        const std::vector<uint32_t> d = cut_desc_table(p, sc.tex);
        memcpy(base + p.layout().off_desc, d.data(), 4 * d.size());
    }
};

struct Nrm {
    using Item = rpt_mesh_normal_map;
    using Entry = NrmMap;
    using Plan = NrmPlan;
    static constexpr MapConsts k = {16, 4, 0};
    static constexpr uint32_t odd_w = 3, odd_h = 5;
    static std::vector<Entry>& entries(Plan& p) { return p.map; }
    static Item item(const Spec& s, const uint8_t* src)
    {
        Item it;
        memset(&it, 0, sizeof(it));
        it.mesh = s.mesh; it.mode = s.width ? RPT_MESH_NORMAL_MAP_ON : RPT_MESH_NORMAL_MAP_OFF; it.width = s.width; it.height = s.height; it.texels = src;
        it.filter = s.mesh & 1u ? RPT_TEX_FILTER_NEAREST : RPT_TEX_FILTER_BILINEAR;
        it.flags = s.mesh == 2u ? (uint32_t)RPT_NORMAL_MAP_FLIP_GREEN : 0u;
        it.strength = 0.5f + (float)s.mesh;
        return it;
    }
    static int check(const Scene& sc, const Item* items, uint32_t n, const Plan& p, std::vector<Entry>& out, std::string& err)
    {
        return check_mesh_normal_maps(sc.plan, true, sc.tex, items, n, p.map, out, err);
    }
    static void build(const Scene& sc, std::vector<Entry> e, Plan& p) { build_nrm_plan(sc.plan, std::move(e), p); }
    static std::vector<MapNamed> named(const std::vector<Item>& items) { return map_named(items.data(), (uint32_t)items.size(), &Item::texels); }
    static void decode(const Plan& p, uint32_t mesh, const uint8_t* staged, uint8_t* dst, uint32_t n)
    {
        nrm_decode_reference(staged, n, p.map[mesh].strength, p.map[mesh].flags, reinterpret_cast<TexTexel*>(dst));
    }
    static void descriptors(const Scene& sc, const Plan& p, uint8_t* base)
    {
        const std::vector<uint32_t> d = nrm_desc_table(p, sc.tex);
        memcpy(base + p.layout().off_desc, d.data(), 4 * d.size());
    }
};

struct Mmap {
    using Item = rpt_mesh_material_map;
    using Entry = MmapMap;
    using Plan = MmapPlan;
    static constexpr MapConsts k = {16, 4, 0};
    static constexpr uint32_t odd_w = 3, odd_h = 5;
    static std::vector<Entry>& entries(Plan& p) { return p.map; }
    static Item item(const Spec& s, const uint8_t* src)
    {
        Item it;
        memset(&it, 0, sizeof(it));
        it.mesh = s.mesh; it.mode = s.width ? RPT_MESH_MATERIAL_MAP_ON : RPT_MESH_MATERIAL_MAP_OFF; it.width = s.width; it.height = s.height; it.texels = src;
        it.filter = s.mesh & 1u ? RPT_TEX_FILTER_NEAREST : RPT_TEX_FILTER_BILINEAR;
        it.roughness_channel = s.mesh; it.metallic_channel = s.mesh == 1u ? RPT_MATERIAL_MAP_CHANNEL_NONE : 3u - s.mesh;
        return it;
    }
    static int check(const Scene& sc, const Item* items, uint32_t n, const Plan& p, std::vector<Entry>& out, std::string& err)
    {
        return check_mesh_material_maps(sc.plan, true, sc.tex, items, n, p.map, out, err);
    }
    static void build(const Scene& sc, std::vector<Entry> e, Plan& p) { build_mmap_plan(sc.plan, std::move(e), p); }
    static std::vector<MapNamed> named(const std::vector<Item>& items) { return map_named(items.data(), (uint32_t)items.size(), &Item::texels); }
    static void decode(const Plan& p, uint32_t mesh, const uint8_t* staged, uint8_t* dst, uint32_t n)
    {
        mmap_decode_reference(staged, n, p.map[mesh].roughness_channel, p.map[mesh].metallic_channel, reinterpret_cast<TexTexel*>(dst));
    }
    static void descriptors(const Scene& sc, const Plan& p, uint8_t* base)
    {
        const std::vector<uint32_t> d = mmap_desc_table(p, sc.tex);
        memcpy(base + p.layout().off_desc, d.data(), 4 * d.size());
    }
};

struct Emap {
    using Item = rpt_mesh_emission_map;
    using Entry = EmapMap;
    using Plan = EmapPlan;
    static constexpr MapConsts k = {16, 4, 1024};
    static constexpr uint32_t odd_w = 3, odd_h = 5;
    static std::vector<Entry>& entries(Plan& p) { return p.map; }
    static Item item(const Spec& s, const uint8_t* src)
    {
        Item it;
        memset(&it, 0, sizeof(it));
        it.mesh = s.mesh; it.mode = s.width ? RPT_MESH_EMISSION_MAP_ON : RPT_MESH_EMISSION_MAP_OFF; it.width = s.width; it.height = s.height; it.texels = src;
        it.filter = s.mesh & 1u ? RPT_TEX_FILTER_NEAREST : RPT_TEX_FILTER_BILINEAR;
        it.gamma = s.mesh == 0u ? 1.0f : 2.2f;
        return it;
    }
    static int check(const Scene& sc, const Item* items, uint32_t n, const Plan& p, std::vector<Entry>& out, std::string& err)
    {
        return check_mesh_emission_maps(sc.plan, true, sc.tex, items, n, p.map, out, err);
    }
    static void build(const Scene& sc, std::vector<Entry> e, Plan& p) { build_emap_plan(sc.plan, std::move(e), p); }
    static std::vector<MapNamed> named(const std::vector<Item>& items) { return map_named(items.data(), (uint32_t)items.size(), &Item::texels); }
    static void decode(const Plan& p, uint32_t mesh, const uint8_t* staged, uint8_t* dst, uint32_t n)
    {
        tex_decode_reference(staged + 1024, n, p.map[mesh].gamma, reinterpret_cast<TexTexel*>(dst));      // (the kernel's L table lies at `staged`)
    }
    static void descriptors(const Scene& sc, const Plan& p, uint8_t* base)
    {
        const EmapLayout el = p.layout();
        const std::vector<uint32_t> d = emap_desc_table(p, sc.tex), l = emap_light_desc_table(p, sc.tex, sc.light);
        memcpy(base + el.off_desc, d.data(), 4 * d.size());
        memcpy(base + el.off_light_desc, l.data(), 4 * l.size());
    }
};

constexpr MapConsts Cut::k, Nrm::k, Mmap::k, Emap::k;

// The emission tables' zero block: all-zero descriptors and an all-0xFFFFFFFF triangle table, whatever the call.
static int zero_block(const EmapPlan& p, const std::vector<uint8_t>& tables)
{
    const EmapLayout el = p.layout();
    const MmapLayout zl = p.zero.layout();
    REQUIRE(zl.total == el.zero.total && zl.off_texels == zl.total && el.off_zero + zl.total <= el.off_texels);
    const uint8_t* z = tables.data() + el.off_zero;
    for (size_t i = 0; i < zl.off_none; ++i) REQUIRE(z[i] == 0u);
    REQUIRE(zl.off_texels - zl.off_none >= 4u * p.n_tris);
    for (size_t i = zl.off_none; i < zl.off_texels; ++i) REQUIRE(z[i] == 0xFFu);
    return 0;
}
template <class Plan> static int zero_block(const Plan&, const std::vector<uint8_t>&) { return 0; }

// One "device" and the "context's" plan of one feature.
template <class F>
struct Sim {
    typename F::Plan plan;
    std::vector<uint8_t> tables;                                     // empty: the device holds none
    std::vector<std::vector<uint8_t>> source = std::vector<std::vector<uint8_t>>(3);      // mesh -> the bytes its image was last set from
};

// capi.hip's map_device with memset and memcpy: every buffer is exactly as large as the call would allocate it, so an offset that is
// off is the sanitizer's to find.
template <class F>
static int device(const Scene& sc, std::vector<uint8_t>& tables, const typename F::Plan& now, const typename F::Plan& old, const std::vector<MapNamed>& named)
{
    const auto nl = now.layout();
    const auto ol = old.layout();
    const MapRecipe r = map_recipe(now.slots(), old.slots(), !tables.empty(), named, F::k);
    REQUIRE(r.missing == kMapNoMesh);
    REQUIRE(r.stage_bytes % 16 == 0);
    std::vector<uint8_t> fresh(nl.total, 0x5A), stage(r.stage_bytes, 0xA5);
    uint8_t* elems = fresh.data() + nl.off_elems();
    for (const MapFill& fl : nl.fills()) {
        REQUIRE(fl.off + fl.bytes <= fresh.size());
        if (fl.bytes) memset(fresh.data() + fl.off, fl.value, fl.bytes);
    }
    size_t next = 0;
    for (const MapRecipe::Item& it : r.items) {
        const MapNamed& nm = named[it.index];
        REQUIRE(nm.on && it.count == (uint64_t)nm.width * nm.height && it.stage % 16 == 0 && it.stage == next);
        next = it.stage + F::k.prefix + map_round16(F::k.src_bytes * (size_t)it.count);
        REQUIRE(next <= stage.size());
        uint8_t* staged = stage.data() + it.stage;
        memcpy(staged + F::k.prefix, nm.src, F::k.src_bytes * (size_t)it.count);
        for (uint32_t b = 0; b < F::k.prefix; ++b) REQUIRE(staged[b] == 0xA5u);      // the image's bytes lie `prefix` past the part's start, and no other part reaches into it
        REQUIRE(F::k.prefix == 0u || F::k.prefix == 1024u);
        F::decode(now, nm.mesh, staged, elems + F::k.elem_bytes * (size_t)it.dst, (uint32_t)it.count);
    }
    REQUIRE(next == stage.size());
    for (const MapRecipe::Keep& kp : r.keeps) {
        REQUIRE(ol.off_elems() + F::k.elem_bytes * (size_t)kp.src + kp.bytes <= tables.size());
        memcpy(elems + F::k.elem_bytes * (size_t)kp.dst, tables.data() + ol.off_elems() + F::k.elem_bytes * (size_t)kp.src, kp.bytes);
    }
    F::descriptors(sc, now, fresh.data());
    tables = std::move(fresh);
    return 0;
}

// capi.hip's set_mesh_maps after the NULL check: the checks, the early returns, the way back to no tables, the plan swap, the device.
template <class F>
static int call(const Scene& sc, Sim<F>& s, const std::vector<Spec>& specs)
{
    std::vector<typename F::Item> items;
    std::vector<std::vector<uint8_t>> fresh_source(3);
    for (const Spec& sp : specs) {
        if (sp.width) fresh_source[sp.mesh] = image_bytes(sp.mesh, F::k.src_bytes * (size_t)sp.width * sp.height);
        items.push_back(F::item(sp, sp.width ? fresh_source[sp.mesh].data() : nullptr));
    }
    std::vector<typename F::Entry> entries;
    std::string err;
    const int rc = F::check(sc, items.data(), (uint32_t)items.size(), s.plan, entries, err);
    if (rc != RPT_OK) { printf("FAILED check: %s\n", err.c_str()); return 1; }
    for (const Spec& sp : specs) s.source[sp.mesh] = fresh_source[sp.mesh];
    bool any = false;
    for (const typename F::Entry& c : entries) any = any || c.width != 0u;
    if (!any && !s.plan.any()) return 0;
    if (!any) {
        s.tables.clear();
        s.plan = typename F::Plan();
        return 0;
    }
    typename F::Plan old = std::move(s.plan);
    F::build(sc, std::move(entries), s.plan);
    return device<F>(sc, s.tables, s.plan, old, F::named(items));
}

// The tables one call that names every ON mesh of `s` builds from nothing equal s's, byte for byte.
template <class F>
static int same_as_from_scratch(const Scene& sc, Sim<F>& s)
{
    Sim<F> t;
    std::vector<Spec> specs;
    for (uint32_t m = 0; m < 3; ++m)
        if (s.plan.on(m)) specs.push_back(Spec{m, F::entries(s.plan)[m].width, F::entries(s.plan)[m].height});
    if (!specs.empty()) REQUIRE(call(sc, t, specs) == 0);
    REQUIRE(t.tables.size() == s.tables.size() && s.tables.size() == (s.plan.any() ? s.plan.layout().total : 0u));
    REQUIRE(t.tables.empty() || memcmp(t.tables.data(), s.tables.data(), s.tables.size()) == 0);
    for (uint32_t m = 0; m < 3; ++m) REQUIRE(t.source[m] == (s.plan.on(m) ? s.source[m] : std::vector<uint8_t>()));
    if (s.plan.any()) REQUIRE(zero_block(s.plan, s.tables) == 0);
    return 0;
}

template <class F>
static int sequence(const char* name)
{
    const Scene sc;
    Sim<F> s;
    const std::vector<std::vector<Spec>> calls = {
        {{0, 3, 5}, {2, 1, 1}}, {{0, 2, 9}}, {{0, 0, 0}}, {{1, F::odd_w, F::odd_h}}, {{1, 0, 0}, {2, 0, 0}},
    };
    const bool on_after[5][3] = {{true, false, true}, {true, false, true}, {false, false, true}, {false, true, true}, {false, false, false}};
    for (size_t c = 0; c < calls.size(); ++c) {
        REQUIRE(call(sc, s, calls[c]) == 0);
        for (uint32_t m = 0; m < 3; ++m) REQUIRE(s.plan.on(m) == on_after[c][m]);
        REQUIRE(same_as_from_scratch(sc, s) == 0);
        const std::vector<MapSlot> slots = s.plan.slots();
        uint64_t at = 0;                                             // the ON meshes' parts lie one after the other in mesh order
        for (const MapSlot& sl : slots) { REQUIRE(!sl.count || sl.first == at); at += sl.count; }
        printf("call %zu: %zu bytes\n", c + 1, s.tables.size());
    }
    REQUIRE(s.tables.empty() && !s.plan.any());
    REQUIRE(call(sc, s, {{0, 0, 0}}) == 0 && s.tables.empty());      // every map OFF, as before
    printf("%s OK\n", name);
    return 0;
}

static int recipe()
{
    const MapConsts plain = {16, 4, 0}, table = {16, 4, 1024}, alpha = {4, 1, 0};
    const uint8_t px[4] = {0, 0, 0, 0};
    const std::vector<MapSlot> now = {{0, 15}, {15, 18}, {33, 1}}, old = {{0, 0}, {0, 18}, {18, 1}};
    const std::vector<MapNamed> named = {{0, true, 3, 5, px}};       // mesh 0: 15 texels, 60 B -> 64; meshes 1 and 2 are kept
    {
        const MapRecipe r = map_recipe(now, old, true, named, plain);
        REQUIRE(r.missing == kMapNoMesh && r.stage_bytes == 64 && r.items.size() == 1 && r.keeps.size() == 2);
        REQUIRE(r.items[0].index == 0 && r.items[0].stage == 0 && r.items[0].dst == 0 && r.items[0].count == 15);
        REQUIRE(r.keeps[0].mesh == 1 && r.keeps[0].src == 0 && r.keeps[0].dst == 15 && r.keeps[0].bytes == 16 * 18);
        REQUIRE(r.keeps[1].mesh == 2 && r.keeps[1].src == 18 && r.keeps[1].dst == 33 && r.keeps[1].bytes == 16);
    }
    {
        const std::vector<MapNamed> two = {{2, true, 1, 1, px}, {1, false, 0, 0, nullptr}, {0, true, 3, 5, px}};      // in the call's order
        const MapRecipe r = map_recipe({{0, 15}, {0, 0}, {15, 1}}, old, true, two, table);
        REQUIRE(r.items.size() == 2 && r.keeps.empty() && r.stage_bytes == (1024 + 16) + (1024 + 64));
        REQUIRE(r.items[0].index == 0 && r.items[0].stage == 0 && r.items[0].dst == 15 && r.items[0].count == 1);
        REQUIRE(r.items[1].index == 2 && r.items[1].stage == 1024 + 16 && r.items[1].dst == 0 && r.items[1].count == 15);
        const MapRecipe a = map_recipe({{0, 8}, {0, 0}, {8, 4}}, old, true, {{2, true, 33, 1, px}, {0, true, 17, 15, px}}, alpha);
        REQUIRE(a.stage_bytes == 48 + 256 && a.items[1].stage == 48 && a.items[1].count == 255 && a.items[0].dst == 8);
    }
    for (int held = 0; held < 2; ++held) {                           // a kept mesh the device holds nothing for: the error, and no step
        const MapRecipe r = map_recipe(now, held ? std::vector<MapSlot>{{0, 0}, {0, 18}} : old, held != 0, named, plain);
        REQUIRE(r.missing == (held ? 2u : 1u) && r.items.empty() && r.keeps.empty() && r.stage_bytes == 0);
    }
    REQUIRE(map_recipe(now, {}, true, named, plain).missing == 1u);
    REQUIRE(map_round16(0) == 0 && map_round16(1) == 16 && map_round16(16) == 16 && map_round16(17) == 32);
    printf("recipe OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "cut") return sequence<Cut>("cut");
    if (what == "nrm") return sequence<Nrm>("nrm");
    if (what == "mmap") return sequence<Mmap>("mmap");
    if (what == "emap") return sequence<Emap>("emap");
    if (what == "recipe") return recipe();
    printf("usage: map_harness cut | nrm | mmap | emap | recipe\n");
    return 2;
}
