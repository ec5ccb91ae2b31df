// host_upload.h — the host half of rpt_upload_scene (include/rpt.h): every check of a scene descriptor, and the image of the scene a
// device holds — a small scene's kernel argument and class map, a large or mesh scene's tables.  No HIP runtime call: capi.hip copies
// SceneImage::bytes to every device and then commits (rpt_upload_scene), and tests/upload_harness.cpp runs this file under the
// address and undefined-behaviour sanitizers (tests/test_upload_host.py).
#pragma once

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"
#include "host_bvh.h"
#include "host_map.h"
#include "host_refit.h"
#include "host_scene.h"
#include "launch.h"

namespace rpthost {

using rptdev::DevBackground;
using rptdev::DevLight;
using rptdev::DevMaterial;
using rptdev::DevPlane;
using rptdev::SceneLarge;
using rptdev::SceneMesh;
using rptdev::SceneSmall;
using rptdev::SceneSmallSdf;

enum class SceneKind : uint32_t {
    none,         // no scene uploaded yet
    small,        // the tables are the kernel argument (SceneSmallSdf); a class map, if any, is the device's tables
    large,        // the tables are in device memory (dev_scene_large.h): beyond the kernel argument's sizes
    mesh,         // ... with triangles and their hierarchy (dev_scene_mesh.h, include/rpt.h "triangle meshes")
};

// What a context keeps of its scene besides the device tables (rpt_ctx::scene).
struct SceneState {
    SceneKind kind = SceneKind::none;
    bool media = false;               // RPT_SCENE_MEDIA and some material carries a medium: the media kernels (dev_media.h)
    rpt_camera camera = {};
    SceneSmallSdf small = {};         // small scenes; the camera part is filled per launch (depends on width/height); sdf.n_prims == 0: plain
    bool class_map_ok = false;        // small scenes of 5-12 primitives: their accepted sets fall into at most 16 classes of equal material
    MatClassMap class_map = {};       // (launch.h; `cls` is filled at launch: the 4 096-byte map is the device's tables)
    uint32_t mesh_nodes = 0, mesh_depth = 0;    // a mesh scene's hierarchy (include/rpt_test.h, rpt_debug_mesh_stats)
    float mesh_build_ms = 0.0f;
};

// Everything a device needs of a scene.  Large and mesh scenes' tables, in `bytes` (every table addressed with 32-bit byte offsets
// from its own base: dev_scene_large.h, gather32): spheres, their materials, lights, materials, the spherical lights' records for
// Scene::sample_lights and their indices, the grid; then, 16-byte aligned, a mesh scene's triangles (48 B) and hierarchy nodes (64 B).
struct SceneImage {
    SceneState state;
    std::vector<unsigned char> bytes; // what every device holds (DevState::tables); empty: nothing (a small scene without a class map)
    SceneMesh tables = {};            // large and mesh scenes: the kernel argument but for its device pointers (bind_scene)
    HostAccel accel;
    RefitPlan refit;                  // mesh scenes: what rpt_update_meshes needs beyond `bytes` (host_refit.h); the context keeps it
    size_t off_smat = 0, off_lights = 0, off_mats = 0, off_lsph = 0, off_lids = 0, off_accel = 0, off_tris = 0, off_nodes = 0;
};

inline DevPlane dev_plane(const rpt_plane& a) { return DevPlane{a.normal[0], a.normal[1], a.normal[2], a.point[0], a.point[1], a.point[2], a.min_denom, a.material, a.max_t}; }
inline DevLight dev_light(const rpt_light& a)
{
    return DevLight{a.type, a.position[0], a.position[1], a.position[2], a.emission[0], a.emission[1], a.emission[2], a.radius, a.area,
                    a.u[0], a.u[1], a.u[2], a.v[0], a.v[1], a.v[2]};
}
inline DevMaterial dev_material(const rpt_material& a)
{
    DevMaterial m;
    m.mask = a.mask; m.proc_kind = a.proc_kind;
    for (int k = 0; k < 3; ++k) { m.rgb[k] = a.rgb[k]; m.emission[k] = a.emission[k]; }
    m.anisotropic = a.anisotropic; m.metallic = a.metallic; m.roughness = a.roughness; m.subsurface = a.subsurface;
    m.specular_tint = a.specular_tint; m.sheen = a.sheen; m.sheen_tint = a.sheen_tint; m.clearcoat = a.clearcoat;
    m.clearcoat_gloss = a.clearcoat_gloss; m.spec_trans = a.spec_trans; m.ior = a.ior;
    for (int k = 0; k < 4; ++k) m.proc_params[k] = a.proc_params[k];
    m.medium_type = a.medium_type; m.medium_density = a.medium_density; m.medium_anisotropy = a.medium_anisotropy;
    for (int k = 0; k < 3; ++k) m.medium_color[k] = a.medium_color[k];
    return m;
}
inline DevBackground dev_background(const rpt_background& b)
{
    return DevBackground{b.kind, b.colour_a[0], b.colour_a[1], b.colour_a[2], b.colour_b[0], b.colour_b[1], b.colour_b[2], b.gamma, b.scale};
}

// The classes of accepted sets of a small scene of 5-12 primitives (launch.h, MatClassMap).  The material of a hit is Material::new()
// overwritten field by field by the accepted primitives in order (apply_patch_fields; a procedural patch writes rgb whatever its
// mask says: apply_patch_row), so two sets give the same material when every field has the same last writer in both.  False: the
// scene is not one the mapped table serves (fewer than 5 primitives, two procedural materials, more than 16 classes).
inline bool material_class_map(const SceneSmall& sc, MatClassMap& map, std::vector<uint8_t>& cls)
{
    using rptdev::kMaxSpheres;
    const uint32_t ns = sc.n_spheres, np = sc.n_planes, nb = ns + np;
    if (nb < 5u || nb > 12u) return false;
    uint32_t n_procedural = 0;
    uint32_t mask_of[rptdev::kMaxSpheres + rptdev::kMaxPlanes];
    for (uint32_t i = 0; i < nb; ++i) {
        const DevMaterial& m = sc.materials[i < ns ? sc.spheres[i].material : sc.planes[i - ns].material];
        n_procedural += m.proc_kind != 0u;
        mask_of[i] = (m.mask & (uint32_t)RPT_MAT_ALL) | (m.proc_kind == RPT_PROC_CHECKER_DIR ? (uint32_t)RPT_MAT_RGB : 0u);
    }
    if (n_procedural > 1u) return false;
    memset(&map, 0, sizeof(map));
    cls.assign(4096, 0);
    struct Signature { uint8_t last[13]; bool operator==(const Signature& o) const { return memcmp(last, o.last, sizeof(last)) == 0; } };
    std::vector<Signature> classes;
    for (uint32_t set = 0; set < (1u << nb); ++set) {
        Signature sig;
        memset(sig.last, 0xFF, sizeof(sig.last));
        for (uint32_t i = 0; i < nb; ++i)
            if ((set >> i) & 1u)
                for (uint32_t f = 0; f < 13u; ++f) if ((mask_of[i] >> f) & 1u) sig.last[f] = (uint8_t)i;
        size_t c = 0;
        while (c < classes.size() && !(classes[c] == sig)) ++c;
        if (c == classes.size()) {
            if (classes.size() == kMatClasses) return false;
            classes.push_back(sig);
            map.class_set[c] = (uint16_t)((set & ((1u << ns) - 1u)) | ((set >> ns) << kMaxSpheres));      // (GeomHit.code's layout: planes from bit 8)
        }
        cls[set] = (uint8_t)c;
    }
    map.n_classes = (uint32_t)classes.size();
    return true;
}

// `err` = "rpt_upload_scene: " + the message (at most 511 characters, as capi.hip's set_err keeps); returns `code` (host_map.h's call_error, under this call's name).
template <class... A>
inline int upload_error(std::string& err, int code, const char* fmt, A... a) { return call_error(err, "rpt_upload_scene", code, fmt, a...); }

// Checks `s` (every RPT_ERR_INVALID_ARG and RPT_ERR_UNSUPPORTED case of include/rpt.h, in one fixed order: a descriptor with several
// faults always answers the first), classifies it and builds `img`.  RPT_OK, or the code with `err` set.  `s` is not NULL.
inline int prepare_scene(const rpt_scene_desc* s, SceneImage& img, std::string& err)
{
    using rptdev::kMaxLights;
    using rptdev::kMaxMaterials;
    using rptdev::kMaxPlanes;
    using rptdev::kMaxSdfPrims;
    using rptdev::kMaxSpheres;
    using rptdev::kNoSphere;
    const int INVALID = RPT_ERR_INVALID_ARG, UNSUPPORTED = RPT_ERR_UNSUPPORTED;
    img = SceneImage();
    if (s->abi_version != RPT_ABI_VERSION) return upload_error(err, INVALID, "abi_version %u != %u", s->abi_version, RPT_ABI_VERSION);
    if ((s->n_spheres && !s->spheres) || (s->n_planes && !s->planes) || (s->n_lights && !s->lights) || (s->n_materials && !s->materials))
        return upload_error(err, INVALID, "a table pointer is NULL");
    // bounded loop counts: a wave must always reach the end of its kernel
    if (s->max_depth > 4096u) return upload_error(err, INVALID, "max_depth %u exceeds the supported 4096", s->max_depth);
    if (s->sdf.n_prims && s->sdf.max_steps > 65536u) return upload_error(err, INVALID, "sdf.max_steps %u exceeds the supported 65536", s->sdf.max_steps);
    const bool large = s->n_spheres > (uint32_t)kMaxSpheres || s->n_lights > (uint32_t)kMaxLights || s->n_materials > (uint32_t)kMaxMaterials;
    if (s->n_planes > (uint32_t)kMaxPlanes) return upload_error(err, UNSUPPORTED, "at most %d planes are supported", kMaxPlanes);
    for (uint32_t i = 0; i < s->n_spheres; ++i)
        if (s->spheres[i].material >= s->n_materials) return upload_error(err, INVALID, "sphere %u material out of range", i);
    for (uint32_t i = 0; i < s->n_planes; ++i)
        if (s->planes[i].material >= s->n_materials) return upload_error(err, INVALID, "plane %u material out of range", i);
    for (uint32_t i = 0; i < s->n_lights; ++i)
        if (s->lights[i].type > RPT_LIGHT_DISTANT) return upload_error(err, INVALID, "light %u has an unknown type", i);
    // participating media (include/rpt.h): used only under RPT_SCENE_MEDIA, and then only when some material carries one
    bool media = false;
    if (s->flags & RPT_SCENE_MEDIA) {
        for (uint32_t i = 0; i < s->n_materials; ++i) {
            const rpt_material& m = s->materials[i];
            if (!(m.mask & RPT_MAT_MEDIUM)) continue;
            if (m.medium_type > RPT_MEDIUM_EMISSIVE) return upload_error(err, INVALID, "material %u has an unknown medium type", i);
            if (!(m.medium_density >= 0.0f) || !std::isfinite(m.medium_density))
                return upload_error(err, INVALID, "material %u: the medium's density must be finite and >= 0", i);
            media = media || m.medium_type != RPT_MEDIUM_NONE;
        }
        if (media && s->n_materials > rptdev::kMaxMediaMaterials)
            return upload_error(err, UNSUPPORTED, "scenes with media can have at most %u materials", rptdev::kMaxMediaMaterials);
    }
    if (s->sdf.n_prims) {
        if (s->sdf.n_prims > (uint32_t)kMaxSdfPrims || !s->sdf.prims || s->sdf.material >= s->n_materials || !(s->sdf.smooth_k > 0.0f))
            return upload_error(err, INVALID, "bad SDF object (1..%d prims, material in range, smooth_k > 0)", kMaxSdfPrims);
        for (uint32_t i = 0; i < s->sdf.n_prims; ++i)
            if (s->sdf.prims[i].kind > RPT_SDF_TORUS_Y) return upload_error(err, INVALID, "unknown SDF primitive kind");
        if (large) return upload_error(err, UNSUPPORTED, "the SDF object is only supported in small scenes");
    }
    // the checks that hold for every scene's meshes (also an empty one's)
    if (s->n_meshes && !s->meshes) return upload_error(err, INVALID, "meshes is NULL");
    uint64_t n_tris = 0;
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const rpt_mesh& me = s->meshes[m];
        if ((me.n_vertices && !me.vertices) || (me.n_triangles && !me.indices)) return upload_error(err, INVALID, "mesh %u: a table pointer is NULL", m);
        if (me.material >= s->n_materials) return upload_error(err, INVALID, "mesh %u material out of range", m);
        for (uint64_t k = 0; k < 3ull * me.n_vertices; ++k)
            if (!std::isfinite(me.vertices[k])) return upload_error(err, INVALID, "mesh %u vertex %llu is not finite", m, (unsigned long long)(k / 3));
        for (uint64_t k = 0; k < 3ull * me.n_triangles; ++k)
            if (me.indices[k] >= me.n_vertices)
                return upload_error(err, INVALID, "mesh %u triangle %llu: vertex index out of range", m, (unsigned long long)(k / 3));
        n_tris += me.n_triangles;
    }
    SceneState& st = img.state;
    st.camera = s->camera;
    st.media = media;

    if (!large && n_tris == 0) {
        // ---- small: the tables are the kernel argument
        st.kind = SceneKind::small;
        SceneSmallSdf& d = st.small;
        d.n_spheres = s->n_spheres; d.n_planes = s->n_planes; d.n_lights = s->n_lights; d.n_materials = s->n_materials;
        d.flags = s->flags;
        d.max_depth = s->max_depth;
        d.eps = s->eps;
        d.n_lights_f = (float)s->n_lights;
        d.bg = dev_background(s->background);
        for (uint32_t i = 0; i < s->n_spheres; ++i) {
            const rpt_sphere& a = s->spheres[i];
            d.spheres[i] = rptdev::DevSphere{a.center[0], a.center[1], a.center[2], a.radius, a.material};
        }
        for (uint32_t i = 0; i < s->n_planes; ++i) d.planes[i] = dev_plane(s->planes[i]);
        for (uint32_t i = 0; i < s->n_lights; ++i) d.lights[i] = dev_light(s->lights[i]);
        for (uint32_t i = 0; i < s->n_materials; ++i) d.materials[i] = dev_material(s->materials[i]);
        d.sdf.n_prims = s->sdf.n_prims; d.sdf.max_steps = s->sdf.max_steps; d.sdf.material = s->sdf.material;
        d.sdf.smooth_k = s->sdf.smooth_k; d.sdf.hit_eps = s->sdf.hit_eps; d.sdf.max_t = s->sdf.max_t; d.sdf.normal_eps = s->sdf.normal_eps;
        d.sdf.inv_smooth_k = s->sdf.n_prims ? 1.0f / s->sdf.smooth_k : 0.0f;
        for (uint32_t i = 0; i < s->sdf.n_prims; ++i) {
            const rpt_sdf_prim& a = s->sdf.prims[i];
            d.sdf.prims[i] = rptdev::DevSdfPrim{a.center[0], a.center[1], a.center[2], a.params[0], a.params[1], a.kind, {0u, 0u}};
        }
        // five to twelve primitives: the classes of accepted sets the material table is indexed by (launch.h, MatClassMap), once per scene
        std::vector<uint8_t> cls;
        st.class_map_ok = s->sdf.n_prims == 0 && !media && material_class_map(static_cast<const SceneSmall&>(d), st.class_map, cls);
        if (st.class_map_ok) img.bytes.assign(cls.begin(), cls.end());
        return RPT_OK;
    }

    // ---- large and mesh scenes: the tables in device memory
    if (n_tris) {
        if (n_tris > RPT_MESH_MAX_TRIANGLES) return upload_error(err, UNSUPPORTED, "at most %u triangles", RPT_MESH_MAX_TRIANGLES);
        if (s->flags & RPT_SCENE_MEDIA) return upload_error(err, UNSUPPORTED, "meshes and participating media (RPT_SCENE_MEDIA) do not go together");
        if (s->sdf.n_prims) return upload_error(err, UNSUPPORTED, "meshes and the SDF object do not go together");
    }
    if ((uint64_t)s->n_spheres + n_tris >= kNoSphere)
        return upload_error(err, UNSUPPORTED, n_tris ? "spheres + triangles must stay below 2^28 - 1" : "at most 2^28 - 2 spheres");
    // Layered patches need a bit per primitive: these scenes must use full sphere (and mesh) materials.
    const auto full_patch = [&](uint32_t mi) { const rpt_material& m = s->materials[mi]; return (m.mask & RPT_MAT_ALL) == RPT_MAT_ALL && m.proc_kind == RPT_PROC_NONE; };
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const rpt_sphere& sp = s->spheres[i];
        if (media && !(s->materials[sp.material].mask & RPT_MAT_MEDIUM))
            // (with patches a nearer sphere WITHOUT a medium would inherit the medium of a farther one accepted before it)
            return upload_error(err, UNSUPPORTED, "in a large scene with media every sphere material must set RPT_MAT_MEDIUM "
                                                  "(medium_type RPT_MEDIUM_NONE for none); sphere %u does not", i);
        if (!full_patch(sp.material)) {
            if (n_tris) return upload_error(err, UNSUPPORTED, "a scene with meshes needs full sphere materials; sphere %u's is not", i);
            return upload_error(err, UNSUPPORTED, "scenes beyond %d spheres / %d lights / %d materials need full sphere materials "
                                                  "(mask == RPT_MAT_ALL, no procedural part); sphere %u does not", kMaxSpheres, kMaxLights, kMaxMaterials, i);
        }
        // the acceleration structures are built from these numbers: they must be numbers
        if (!std::isfinite(sp.center[0]) || !std::isfinite(sp.center[1]) || !std::isfinite(sp.center[2]) || !std::isfinite(sp.radius) || sp.radius < 0.0f)
            return upload_error(err, INVALID, "sphere %u has a non-finite centre or a negative / non-finite radius", i);
    }
    for (uint32_t m = 0; m < s->n_meshes; ++m)
        if (!full_patch(s->meshes[m].material))
            return upload_error(err, UNSUPPORTED, "mesh %u's material is not a full patch (mask == RPT_MAT_ALL, no procedural part)", m);
    st.kind = n_tris ? SceneKind::mesh : SceneKind::large;

    // flatten: meshes in order, each mesh's triangles in order; the hierarchy over them (host_bvh.h)
    const uint32_t n = (uint32_t)n_tris;
    std::vector<float> tv(9 * (size_t)n);
    std::vector<uint32_t> tmat(n);
    for (uint32_t m = 0, k = 0; m < s->n_meshes; ++m) {
        const rpt_mesh& me = s->meshes[m];
        for (uint32_t t = 0; t < me.n_triangles; ++t, ++k) {
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) tv[9 * (size_t)k + 3 * v + a] = me.vertices[3 * (size_t)me.indices[3 * (size_t)t + v] + a];
            tmat[k] = me.material;
        }
    }
    HostBvh bvh;
    if (n) {
        const auto t_build = std::chrono::steady_clock::now();
        build_bvh(tv.data(), n, bvh);
        st.mesh_build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build).count();
        st.mesh_nodes = (uint32_t)bvh.nodes.size();
        st.mesh_depth = bvh.depth;
        build_refit_plan(s, bvh, img.refit);
    }
    const size_t sz_tris = 48 * (size_t)n, sz_nodes = sizeof(BvhNode) * bvh.nodes.size();

    // the layout of `bytes`
    const bool use_accel = s->n_spheres >= 64 && !knobs().no_grid;
    if (use_accel) {
        std::string why;
        if (!build_accel(s->spheres, s->n_spheres, img.accel, why)) return upload_error(err, UNSUPPORTED, "%s", why.c_str());
    }
    // The spherical lights once more as {centre, radius * radius} records with their indices, padded to whole groups of four: what
    // Scene::sample_lights' loop streams (dev_scene_large.h, closest_geom_finish).  Only when every light that DOES something
    // in sample_lights is spherical: always, unless the scene samples the other light types and has a rectangular one.
    std::vector<float> lsph;
    std::vector<uint32_t> lids;
    bool lights_fast = true;
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        const rpt_light& l = s->lights[i];
        if (l.type == RPT_LIGHT_SPHERICAL) { lsph.insert(lsph.end(), {l.position[0], l.position[1], l.position[2], l.radius * l.radius}); lids.push_back(i); }
        else if (l.type == RPT_LIGHT_RECTANGULAR && (s->flags & RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES)) lights_fast = false;
    }
    const uint32_t n_light_spheres = (uint32_t)lids.size();
    while (lids.size() % 4u) { lsph.insert(lsph.end(), {0.0f, 0.0f, 0.0f, 0.0f}); lids.push_back(0u); }
    const auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    img.off_smat = sizeof(float4) * s->n_spheres;
    img.off_lights = img.off_smat + round16(sizeof(uint32_t) * s->n_spheres);
    img.off_mats = img.off_lights + round16(sizeof(DevLight) * (s->n_lights ? s->n_lights : 1));
    img.off_lsph = img.off_mats + round16(sizeof(DevMaterial) * (s->n_materials ? s->n_materials : 1));
    img.off_lids = img.off_lsph + sizeof(float) * lsph.size();
    img.off_accel = img.off_lids + round16(sizeof(uint32_t) * lids.size());
    img.off_tris = round16(img.off_accel + img.accel.bytes());
    img.off_nodes = img.off_tris + sz_tris;
    // every table is addressed with 32-bit byte offsets from its own base (dev_scene_large.h, gather32)
    if ((uint64_t)img.off_nodes + sz_nodes >= (1ull << 32)) return upload_error(err, UNSUPPORTED, "the scene's tables exceed 4 GiB");

    std::vector<unsigned char>& h = img.bytes;
    h.assign(n ? img.off_nodes + sz_nodes : img.off_accel + img.accel.bytes(), 0);
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const rpt_sphere& sp = s->spheres[i];
        const float c[4] = {sp.center[0], sp.center[1], sp.center[2], sp.radius};
        memcpy(h.data() + sizeof(float4) * i, c, sizeof(c));
        memcpy(h.data() + img.off_smat + sizeof(uint32_t) * i, &sp.material, sizeof(uint32_t));
    }
    for (uint32_t i = 0; i < s->n_lights; ++i) { const DevLight l = dev_light(s->lights[i]); memcpy(h.data() + img.off_lights + sizeof(DevLight) * i, &l, sizeof(l)); }
    for (uint32_t i = 0; i < s->n_materials; ++i) { const DevMaterial m = dev_material(s->materials[i]); memcpy(h.data() + img.off_mats + sizeof(DevMaterial) * i, &m, sizeof(m)); }
    if (!lsph.empty()) memcpy(h.data() + img.off_lsph, lsph.data(), sizeof(float) * lsph.size());
    if (!lids.empty()) memcpy(h.data() + img.off_lids, lids.data(), sizeof(uint32_t) * lids.size());
    if (use_accel) img.accel.write(h.data() + img.off_accel);
    // triangles in leaf order: {a, flattened index}, {b - a, -}, {c - a, material} (dev_scene_mesh.h, tri_at)
    for (uint32_t slot = 0; slot < n; ++slot) {
        const uint32_t i = bvh.order[slot];
        const float* v = &tv[9 * (size_t)i];
        float r[12] = {v[0], v[1], v[2], 0.0f, v[3] - v[0], v[4] - v[1], v[5] - v[2], 0.0f, v[6] - v[0], v[7] - v[1], v[8] - v[2], 0.0f};
        memcpy(&r[3], &i, 4);
        memcpy(&r[11], &tmat[i], 4);
        memcpy(h.data() + img.off_tris + sizeof(r) * slot, r, sizeof(r));
    }
    if (sz_nodes) memcpy(h.data() + img.off_nodes, bvh.nodes.data(), sz_nodes);

    // the kernel argument but for its device pointers
    SceneMesh& M = img.tables;
    M.n_spheres = s->n_spheres; M.n_planes = s->n_planes; M.n_lights = s->n_lights; M.n_materials = s->n_materials;
    M.flags = s->flags; M.max_depth = s->max_depth; M.eps = s->eps; M.n_lights_f = (float)s->n_lights;
    M.bg = dev_background(s->background);
    for (uint32_t i = 0; i < s->n_planes; ++i) M.planes[i] = dev_plane(s->planes[i]);
    M.n_light_spheres = lights_fast ? n_light_spheres : 0xFFFFFFFFu;
    M.use_accel = use_accel ? 1u : 0u;
    M.n_tris = n;
    // the walk's exactness argument needs finite widened slab bounds (dev_scene_mesh.h): beyond 2^60 the ordered loop serves every ray
    bool coords_ok = true;
    for (float x : tv) coords_ok = coords_ok && std::fabs(x) <= 0x1p60f;
    M.use_bvh = (n && coords_ok) ? 1u : 0u;
    return RPT_OK;
}

// The kernel argument of a large or mesh scene over a copy of img.bytes at `base` (on a device, or on the host in the tests); for
// a small scene, img.tables as it is (zero: its kernel argument is SceneState::small).
inline void bind_scene(const SceneImage& img, unsigned char* base, SceneMesh& M)
{
    M = img.tables;
    if (img.state.kind != SceneKind::large && img.state.kind != SceneKind::mesh) return;
    M.spheres = reinterpret_cast<const float4*>(base);
    M.sphere_material = reinterpret_cast<const uint32_t*>(base + img.off_smat);
    M.lights = reinterpret_cast<const DevLight*>(base + img.off_lights);
    M.materials = reinterpret_cast<const DevMaterial*>(base + img.off_mats);
    M.light_spheres = reinterpret_cast<const float4*>(base + img.off_lsph);
    M.light_sphere_ids = reinterpret_cast<const uint32_t*>(base + img.off_lids);
    if (M.use_accel) img.accel.bind(M, base + img.off_accel);
    if (M.n_tris) {
        M.tris = reinterpret_cast<const float4*>(base + img.off_tris);
        M.nodes = reinterpret_cast<const float4*>(base + img.off_nodes);
    }
}

}  // namespace rpthost
