// rpt.hpp — C++ host-side mirror of the reference's render API over the C ABI (rpt.h).
//
// The reference is compiled code (Rust) and this image has no Rust toolchain, so the host side
// above the C ABI is written in C++ with the reference's names, argument meaning and behaviour:
//
//   reference                                              here
//   ColorBuffer::new(w, h)            buffer.rs:18         rpt::ColorBuffer(w, h)
//   ColorBuffer::at / convert_to_u8   buffer.rs:29, :55    .at(x, y) / tracer.convert_to_u8(buffer, frame)
//   Pinhole::new/set/set_fov          pinhole.rs:14-34     rpt::Pinhole
//   AnalyticalLight::spherical        light.rs:13          rpt::AnalyticalLight::spherical
//   AnalyticalScene::new              analytical.rs:13     rpt::AnalyticalScene
//   Tracer::new / render / scene      tracer.rs:13,22,629  rpt::Tracer
//
// Errors: the reference's render() cannot fail; here a failing C-ABI call throws rpt::Error
// (status + rpt_last_error text).  Header-only; link with -lrpt_hip.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "rpt.h"

namespace rpt {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& msg) : std::runtime_error("rpt status " + std::to_string(s) + ": " + msg), status(s) {}
};

struct F3 { float x, y, z; };

// buffer.rs:6-32
struct ColorBuffer {
    size_t width, height;
    std::vector<float> pixels;      // RGBA f32, row 0 = top
    size_t frames;
    ColorBuffer(size_t w, size_t h) : width(w), height(h), pixels(w * h * 4, 0.0f), frames(0) {}
    void at(size_t x, size_t y, float out[4]) const {
        size_t i = y * width * 4 + x * 4;
        for (int c = 0; c < 4; ++c) out[c] = pixels[i + c];
    }
};

// camera/pinhole.rs:6-34
struct Pinhole {
    F3 origin{0.0f, 0.0f, 3.0f}, center{0.0f, 0.0f, 0.0f};
    float fov = 80.0f;
    void set(F3 o, F3 c) { origin = o; center = c; }
    void set_fov(float f) { fov = f; }
};

// light.rs:6-28
struct AnalyticalLight {
    rpt_light light{};
    static AnalyticalLight spherical(F3 position, float radius, F3 emission) {
        AnalyticalLight l;
        l.light.type = RPT_LIGHT_SPHERICAL;
        l.light.position[0] = position.x; l.light.position[1] = position.y; l.light.position[2] = position.z;
        l.light.emission[0] = emission.x; l.light.emission[1] = emission.y; l.light.emission[2] = emission.z;
        l.light.radius = radius;
        l.light.area = 4.0f * 3.14159265358979323846f * radius * radius;      // light.rs:22
        return l;
    }
    // LightType::Rectangular / Distant (globals.rs:69-73): declared by the reference, sampled only in scenes with
    // sample_all_light_types (project-defined, see rpt.h)
    static AnalyticalLight rectangular(F3 position, F3 u, F3 v, F3 emission) {
        AnalyticalLight l;
        l.light.type = RPT_LIGHT_RECTANGULAR;
        l.light.position[0] = position.x; l.light.position[1] = position.y; l.light.position[2] = position.z;
        l.light.emission[0] = emission.x; l.light.emission[1] = emission.y; l.light.emission[2] = emission.z;
        l.light.u[0] = u.x; l.light.u[1] = u.y; l.light.u[2] = u.z;
        l.light.v[0] = v.x; l.light.v[1] = v.y; l.light.v[2] = v.z;
        const double cx = (double)u.y * v.z - (double)u.z * v.y, cy = (double)u.z * v.x - (double)u.x * v.z, cz = (double)u.x * v.y - (double)u.y * v.x;
        l.light.area = (float)std::sqrt(cx * cx + cy * cy + cz * cz);
        return l;
    }
    static AnalyticalLight distant(F3 position, F3 emission) {
        AnalyticalLight l;
        l.light.type = RPT_LIGHT_DISTANT;
        l.light.position[0] = position.x; l.light.position[1] = position.y; l.light.position[2] = position.z;
        l.light.emission[0] = emission.x; l.light.emission[1] = emission.y; l.light.emission[2] = emission.z;
        return l;
    }
};

// Data-driven counterpart of trait Scene (scene.rs:5-90): the scene describes itself.
struct Scene {
    Pinhole camera;
    std::vector<rpt_sphere> spheres;
    std::vector<rpt_plane> planes;
    std::vector<AnalyticalLight> lights;
    std::vector<rpt_material> materials;      // patches over Material::new()
    rpt_background background{RPT_BG_CONSTANT, {0, 0, 0}, {0, 0, 0}, 2.2f, 1.0f};
    float eps = 0.005f;                        // tracer.rs:16
    uint32_t max_depth = 4;                    // scene.rs:28-30
    bool any_hit_uses_max_dist = false;
    bool sample_all_light_types = false;       // rectangular / distant lights do something (off = the reference)
    // triangle meshes (include/rpt.h, "triangle meshes"): each points at vertex / index arrays the caller keeps alive
    std::vector<rpt_mesh> meshes;
    virtual ~Scene() = default;

    size_t number_of_lights() const { return lights.size(); }
    const AnalyticalLight& light_at(size_t i) const { return lights.at(i); }
    uint16_t recursion_depth() const { return (uint16_t)max_depth; }

    // keeps `lights_flat_` alive; the descriptor points into this object
    rpt_scene_desc describe() {
        lights_flat_.clear();
        for (const auto& l : lights) lights_flat_.push_back(l.light);
        rpt_scene_desc d{};
        d.abi_version = RPT_ABI_VERSION;
        d.flags = (any_hit_uses_max_dist ? RPT_SCENE_ANYHIT_USES_MAX_DIST : 0u) | (sample_all_light_types ? RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES : 0u);
        d.camera.origin[0] = camera.origin.x; d.camera.origin[1] = camera.origin.y; d.camera.origin[2] = camera.origin.z;
        d.camera.center[0] = camera.center.x; d.camera.center[1] = camera.center.y; d.camera.center[2] = camera.center.z;
        d.camera.fov_deg = camera.fov;
        d.background = background;
        d.eps = eps;
        d.max_depth = max_depth;
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_planes = (uint32_t)planes.size(); d.planes = planes.data();
        d.n_lights = (uint32_t)lights_flat_.size(); d.lights = lights_flat_.data();
        d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.n_meshes = (uint32_t)meshes.size(); d.meshes = meshes.data();
        return d;
    }

private:
    std::vector<rpt_light> lights_flat_;
};

// renderer/src/analytical.rs:4-205
struct AnalyticalScene : Scene {
    AnalyticalScene() {
        rpt_scene_desc d{};
        rpt_scene_analytical(&d);
        spheres.assign(d.spheres, d.spheres + d.n_spheres);
        planes.assign(d.planes, d.planes + d.n_planes);
        materials.assign(d.materials, d.materials + d.n_materials);
        for (uint32_t i = 0; i < d.n_lights; ++i) { AnalyticalLight l; l.light = d.lights[i]; lights.push_back(l); }
        background = d.background;
        eps = d.eps;
        max_depth = d.max_depth;
        camera.origin = F3{d.camera.origin[0], d.camera.origin[1], d.camera.origin[2]};
        camera.center = F3{d.camera.center[0], d.camera.center[1], d.camera.center[2]};
        camera.fov = d.camera.fov_deg;
    }
};

// tracer.rs:5-19, :22, :629
class Tracer {
public:
    explicit Tracer(Scene* scene, int device = 0, uint64_t seed = 1) : scene_(scene), seed_(seed) {
        check(rpt_create(&ctx_, device), nullptr);
        sync_scene();
    }
    /// The GPUs of a node driven by this process: render() fans the rows out over them inside the call, where the
    /// reference fans out over rayon's threads (tracer.rs:29-32).
    Tracer(Scene* scene, const std::vector<int>& devices, uint64_t seed = 1) : scene_(scene), seed_(seed) {
        check(rpt_create_multi(&ctx_, devices.data(), (int)devices.size()), nullptr);
        sync_scene();
    }
    void set_tile_rows(uint32_t tile_rows) { check(rpt_set_tile_rows(ctx_, tile_rows), ctx_); }
    // scheduling of the launches (rpt.h, rpt_set_dispatch): changes when a sample is computed, never its value
    void set_dispatch(uint32_t cost_order = 1, uint32_t unit_rounds = 12, uint32_t unit_min_spp = 64, uint32_t unit_slots = 0)
    {
        check(rpt_set_dispatch(ctx_, cost_order, unit_rounds, unit_min_spp, unit_slots), ctx_);
    }
    ~Tracer() { rpt_destroy(ctx_); }
    Tracer(const Tracer&) = delete;
    Tracer& operator=(const Tracer&) = delete;

    /// Render one frame and accumulate into the pixels buffer (tracer.rs:21-123).
    void render(ColorBuffer& buffer) { render_n(buffer, 1); }

    /// `spp` consecutive frames in one launch; bit-identical to `spp` render() calls.
    void render_n(ColorBuffer& buffer, uint32_t spp) {
        check(rpt_render(ctx_, buffer.pixels.data(), (uint32_t)buffer.width, (uint32_t)buffer.height, buffer.frames, spp, seed_, 0), ctx_);
        buffer.frames += spp;                                           // tracer.rs:121
    }

    /// ColorBuffer::convert_to_u8 (buffer.rs:55-64) on the device.
    void convert_to_u8(const ColorBuffer& buffer, uint8_t* frame) {
        check(rpt_convert_to_u8(ctx_, buffer.pixels.data(), frame, (uint32_t)buffer.width, (uint32_t)buffer.height), ctx_);
    }

    /// The interactive loop of renderer/src/main.rs:113-124 with the ColorBuffer kept in HBM: render `spp` more
    /// frames into the context's resident buffer, then fetch the gamma-encoded u8 frame (4 B per pixel).
    void render_resident(size_t width, size_t height, uint32_t spp = 1) { check(rpt_resident_render(ctx_, (uint32_t)width, (uint32_t)height, spp, seed_, 0), ctx_); }
    void resident_to_u8(uint8_t* frame) { check(rpt_resident_download_u8(ctx_, frame), ctx_); }
    void resident_to(ColorBuffer& buffer) {
        check(rpt_resident_download(ctx_, buffer.pixels.data()), ctx_);
        uint64_t f = 0; rpt_resident_frames(ctx_, &f); buffer.frames = (size_t)f;
    }
    void resident_reset() { check(rpt_resident_reset(ctx_), ctx_); }

    /// Return the scene (tracer.rs:629); call sync_scene() after mutating it.
    Scene* scene() { return scene_; }
    void sync_scene() { rpt_scene_desc d = scene_->describe(); check(rpt_upload_scene(ctx_, &d), ctx_); }
    /// New vertex positions for meshes of the uploaded scene without the upload (rpt.h, "moving meshes"): the frames of a fresh
    /// sync_scene() of the moved scene, from a refit of the hierarchy on the device.  The caller's Scene keeps its own arrays:
    /// point its rpt_mesh entries at the new positions before the next sync_scene().
    void update_meshes(const std::vector<rpt_mesh_vertices>& updates) {
        check(rpt_update_meshes(ctx_, updates.data(), (uint32_t)updates.size()), ctx_);
    }
    /// ... and a new hierarchy over all triangles, built on the device (rpt.h, "rebuilding a moved mesh's hierarchy"): for a mesh
    /// whose shape has changed.  No updates: a rebuild over the positions the context holds.
    void rebuild_meshes(const std::vector<rpt_mesh_vertices>& updates = {}) {
        check(rpt_rebuild_meshes(ctx_, updates.data(), (uint32_t)updates.size()), ctx_);
    }
    /// The two calls for positions in DEVICE memory, each mesh through an optional 3x4 transform applied on the device (rpt.h,
    /// "moving meshes from device memory").  They block and have consumed the sources when they return.
    void update_meshes_device(const std::vector<rpt_mesh_source>& sources) {
        check(rpt_update_meshes_device(ctx_, sources.data(), (uint32_t)sources.size()), ctx_);
    }
    void rebuild_meshes_device(const std::vector<rpt_mesh_source>& sources = {}) {
        check(rpt_rebuild_meshes_device(ctx_, sources.data(), (uint32_t)sources.size()), ctx_);
    }
    /// The positions the context holds for one mesh of the uploaded scene (xyz per vertex).
    std::vector<float> mesh_vertices(uint32_t mesh, uint32_t n_vertices) {
        std::vector<float> out(3 * (size_t)n_vertices);
        check(rpt_download_mesh_vertices(ctx_, mesh, out.data(), n_vertices), ctx_);
        return out;
    }
    /// Per-mesh shading (rpt.h, "smooth mesh shading"): RPT_MESH_SHADING_SMOOTH interpolates vertex normals the library computes
    /// on the device and keeps current through every call above; sync_scene() leaves every mesh flat again.
    void set_mesh_shading(const std::vector<rpt_mesh_shading>& items) {
        check(rpt_set_mesh_shading(ctx_, items.data(), (uint32_t)items.size()), ctx_);
    }
    /// The vertex normals the context holds for one SMOOTH mesh (xyz per vertex).
    std::vector<float> mesh_normals(uint32_t mesh, uint32_t n_vertices) {
        std::vector<float> out(3 * (size_t)n_vertices);
        check(rpt_download_mesh_normals(ctx_, mesh, out.data(), n_vertices), ctx_);
        return out;
    }
    /// Mesh lights (rpt.h, "mesh lights"): next-event estimation samples the surface of every mesh that is RPT_MESH_LIGHT_ON, through
    /// a table the library computes on the device and keeps current through every call above; sync_scene() leaves every mesh off.
    void set_mesh_lights(const std::vector<rpt_mesh_light>& items) {
        check(rpt_set_mesh_lights(ctx_, items.data(), (uint32_t)items.size()), ctx_);
    }
    /// The table the context holds for one ON mesh: the running sums C_k (one per triangle), the exponent E and the area A_tot.
    struct MeshLightTable { std::vector<uint64_t> cdf; int32_t exponent = 0; float area = 0.0f; };
    MeshLightTable mesh_light_table(uint32_t mesh, uint32_t n_triangles) {
        MeshLightTable t;
        t.cdf.resize(n_triangles);
        check(rpt_download_mesh_light_table(ctx_, mesh, t.cdf.data(), n_triangles, &t.exponent, &t.area), ctx_);
        return t;
    }
    /// Mesh textures (rpt.h, "mesh textures"): a UV-mapped RGBA8 base colour per mesh, decoded on the device and multiplied into the
    /// mesh material's rgb at every hit; an item without an image removes its mesh's texture; sync_scene() leaves every mesh untextured.
    void set_mesh_textures(const std::vector<rpt_mesh_texture>& items) {
        check(rpt_set_mesh_textures(ctx_, items.data(), (uint32_t)items.size()), ctx_);
    }
    /// The decoded texels the context holds for one textured mesh: width * height * 4 floats, row 0 first.
    std::vector<float> mesh_texture(uint32_t mesh, uint32_t width, uint32_t height) {
        std::vector<float> out(4 * (size_t)width * height);
        check(rpt_download_mesh_texture(ctx_, mesh, out.data(), width, height), ctx_);
        return out;
    }
    /// Environment lighting (rpt.h, "environment lighting"): a square f32 RGB image in the octahedral layout replaces the background
    /// of the uploaded mesh scene and, with RPT_ENV_SAMPLED, is importance-sampled by direct_light; sync_scene() drops it.
    void set_environment(const rpt_environment& env) { check(rpt_set_environment(ctx_, &env), ctx_); }
    void remove_environment() { check(rpt_set_environment(ctx_, nullptr), ctx_); }
    /// The running sums C_k of a SAMPLED environment's table (size * size of them) and its exponent E.
    std::vector<uint64_t> environment_table(uint32_t size, int32_t* exponent) {
        std::vector<uint64_t> out((size_t)size * size);
        check(rpt_download_environment_table(ctx_, out.data(), size * size, exponent), ctx_);
        return out;
    }
    /// Mesh cutouts (rpt.h, "mesh cutouts"): an A8 mask per named mesh, tested inside the walks through the mesh's texture UVs; an item
    /// with RPT_MESH_CUTOUT_OFF removes its mesh's.  sync_scene() drops them all.
    void set_mesh_cutouts(const std::vector<rpt_mesh_cutout>& items) { check(rpt_set_mesh_cutouts(ctx_, items.data(), (uint32_t)items.size()), ctx_); }
    /// The mask bits the context holds for one cutout mesh: ceil(width * height / 32) words, texel k in bit k % 32 of word k / 32.
    std::vector<uint32_t> mesh_cutout(uint32_t mesh, uint32_t width, uint32_t height) {
        std::vector<uint32_t> out(((size_t)width * height + 31) / 32);
        check(rpt_download_mesh_cutout(ctx_, mesh, out.data(), (uint32_t)out.size()), ctx_);
        return out;
    }
    /// Mesh normal maps (rpt.h, "mesh normal maps"): an RGBA8 tangent-space map per named mesh, looked up through the mesh's texture UVs
    /// at the hit, bends the shading normal; an item with RPT_MESH_NORMAL_MAP_OFF removes its mesh's.  sync_scene() drops them all.
    void set_mesh_normal_maps(const std::vector<rpt_mesh_normal_map>& items) { check(rpt_set_mesh_normal_maps(ctx_, items.data(), (uint32_t)items.size()), ctx_); }
    /// The decoded texels the context holds for one normal-mapped mesh: width * height * 4 floats {x, y, z, 0}.
    std::vector<float> mesh_normal_map(uint32_t mesh, uint32_t width, uint32_t height) {
        std::vector<float> out((size_t)width * height * 4);
        check(rpt_download_mesh_normal_map(ctx_, mesh, out.data(), width, height), ctx_);
        return out;
    }
    /// Mesh material maps (rpt.h, "mesh material maps"): an RGBA8 map per named mesh, looked up through the mesh's texture UVs at the
    /// hit, scales the material's roughness and metallic; an item with RPT_MESH_MATERIAL_MAP_OFF removes its mesh's.  sync_scene() drops them all.
    void set_mesh_material_maps(const std::vector<rpt_mesh_material_map>& items) { check(rpt_set_mesh_material_maps(ctx_, items.data(), (uint32_t)items.size()), ctx_); }
    /// The decoded texels the context holds for one material-mapped mesh: width * height * 4 floats {fr, fm, 0, 0}.
    std::vector<float> mesh_material_map(uint32_t mesh, uint32_t width, uint32_t height) {
        std::vector<float> out((size_t)width * height * 4);
        check(rpt_download_mesh_material_map(ctx_, mesh, out.data(), width, height), ctx_);
        return out;
    }
    /// Mesh emission maps (rpt.h, "mesh emission maps"): an RGBA8 map per named mesh, looked up through the mesh's texture UVs, scales the
    /// material's emission at the hit, in the mesh-light sampler and at the emitter exit; an item with RPT_MESH_EMISSION_MAP_OFF removes its
    /// mesh's.  sync_scene() drops them all.
    void set_mesh_emission_maps(const std::vector<rpt_mesh_emission_map>& items) { check(rpt_set_mesh_emission_maps(ctx_, items.data(), (uint32_t)items.size()), ctx_); }
    /// The decoded texels the context holds for one emission-mapped mesh: width * height * 4 floats {r, g, b, 0}.
    std::vector<float> mesh_emission_map(uint32_t mesh, uint32_t width, uint32_t height) {
        std::vector<float> out((size_t)width * height * 4);
        check(rpt_download_mesh_emission_map(ctx_, mesh, out.data(), width, height), ctx_);
        return out;
    }
    /// Mesh media (rpt.h, "mesh media"): a homogeneous medium bounded by each named mesh — coloured absorption, a glow or fog; an item of
    /// type RPT_MEDIUM_NONE removes its mesh's.  sync_scene() drops them all.
    void set_mesh_media(const std::vector<rpt_mesh_medium>& items) { check(rpt_set_mesh_media(ctx_, items.data(), (uint32_t)items.size()), ctx_); }
    /// Ray queries (rpt.h, "ray queries") on device arrays, enqueued on `stream`: the closest hit of every ray (and, with `surfaces`,
    /// the surface there), whether anything lies along it before its max_dist, and the camera's rays through the pixel centres.
    void trace_rays_device(const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces = nullptr, void* stream = nullptr)
    {
        check(rpt_trace_rays_device(ctx_, rays, n, hits, surfaces, 0u, stream), ctx_);
    }
    void occluded_device(const rpt_ray* rays, uint64_t n, uint8_t* occluded, void* stream = nullptr) { check(rpt_occluded_device(ctx_, rays, n, occluded, 0u, stream), ctx_); }
    void camera_rays_device(uint32_t width, uint32_t height, rpt_ray* rays, void* stream = nullptr) { check(rpt_camera_rays_device(ctx_, width, height, rays, stream), ctx_); }
    /// The same on host arrays; they block.
    std::vector<rpt_hit> trace_rays(const std::vector<rpt_ray>& rays, std::vector<rpt_surface>* surfaces = nullptr)
    {
        std::vector<rpt_hit> hits(rays.size());
        if (surfaces) surfaces->resize(rays.size());
        check(rpt_trace_rays(ctx_, rays.data(), rays.size(), hits.data(), surfaces ? surfaces->data() : nullptr, 0u), ctx_);
        return hits;
    }
    std::vector<uint8_t> occluded(const std::vector<rpt_ray>& rays)
    {
        std::vector<uint8_t> out(rays.size());
        check(rpt_occluded(ctx_, rays.data(), rays.size(), out.data(), 0u), ctx_);
        return out;
    }
    /// Radiance queries (rpt.h, "radiance queries"): `spp` samples of the integrator's estimate along every ray, blended into `out`
    /// (a ColorBuffer pixel per ray, in/out) as frames `frames_done` ..., with the tracer's seed; and the rays a render of `frame` sends.
    void radiance_device(const rpt_ray* rays, uint64_t n, float* out, uint64_t frames_done = 0, uint32_t spp = 1, uint32_t first_index = 0, void* stream = nullptr)
    {
        check(rpt_radiance_device(ctx_, rays, n, out, frames_done, spp, seed_, first_index, 0u, stream), ctx_);
    }
    void camera_sample_rays_device(uint32_t width, uint32_t height, uint64_t frame, rpt_ray* rays, void* stream = nullptr)
    {
        check(rpt_camera_sample_rays_device(ctx_, width, height, frame, seed_, rays, stream), ctx_);
    }
    /// The same on host arrays; it blocks.  Returns n x 4 floats, accumulated from zeros.
    std::vector<float> radiance(const std::vector<rpt_ray>& rays, uint32_t spp = 1, uint64_t frames_done = 0, uint32_t first_index = 0)
    {
        std::vector<float> out(rays.size() * 4, 0.0f);
        check(rpt_radiance(ctx_, rays.data(), rays.size(), out.data(), frames_done, spp, seed_, first_index, 0u), ctx_);
        return out;
    }

private:
    static void check(int rc, const rpt_ctx* ctx) { if (rc != RPT_OK) throw Error(rc, rpt_last_error(ctx)); }
    rpt_ctx* ctx_ = nullptr;
    Scene* scene_;
    uint64_t seed_;
};

}  // namespace rpt
