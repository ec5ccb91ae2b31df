/* rpt.h — C ABI of the MI355X-native path-tracing integrator.
 *
 * This is the drop-in boundary for ONE hot path of markusmoenig/rust-pathtracer:
 *     Tracer::render(&mut self, buffer: &mut ColorBuffer)
 *         rust-pathtracer/src/tracer.rs:22-123   (rayon scanline loop + bounce loop)
 * and its callees (direct_light :126, sample_light :173, Disney BSDF :223-626,
 * Scene::sample_lights scene.rs:36-86, Pinhole::gen_ray camera/pinhole.rs:38-60,
 * State/Material finalize globals.rs:50-62 / material.rs:117-131) plus the workload
 * scene renderer/src/analytical.rs:13-204.
 *
 * The reference has no FFI of its own (the path is a plain Rust method), so these
 * entry points are what a Rust `extern "C"` block for that method binds; the
 * binding is shown in INTEGRATION.md and rust/gpu_tracer.rs.
 *
 * Conventions
 *   - every function returns 0 on success or a negative rpt_status; nothing unwinds
 *     across the boundary (the reference's render() cannot fail: tracer.rs:22);
 *   - plain pointers and sizes only; a context is used by one thread at a time
 *     (render takes &mut self in the reference: tracer.rs:22);
 *   - all arithmetic is f32 (rust-pathtracer/src/lib.rs:6).
 */
#ifndef RPT_H
#define RPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPT_ABI_VERSION 5u            /* 5: triangle meshes (rpt_mesh, rpt_scene_desc.meshes); 4: the A/B-only render flags and the test hooks left this header (include/rpt_test.h) */

typedef enum rpt_status {
    RPT_OK              =  0,
    RPT_ERR_INVALID_ARG = -1,
    RPT_ERR_NO_DEVICE   = -2,   /* no usable gfx950 device: the product has no CPU fallback */
    RPT_ERR_HIP         = -3,   /* a HIP runtime call failed; see rpt_last_error */
    RPT_ERR_NO_SCENE    = -4,
    RPT_ERR_UNSUPPORTED = -5,
    RPT_ERR_RCCL        = -6    /* an RCCL call failed (or librccl.so.1 could not be loaded); see rpt_last_error */
} rpt_status;

/* ---- scene as data ---------------------------------------------------------
 * The reference's Scene is code (trait callbacks, scene.rs:5-90) and cannot run
 * on the device, so the scene crosses the boundary as plain data.  The closed set
 * below covers renderer/src/analytical.rs exactly, including its material
 * layering: closest_hit overwrites fields of state.material each time a primitive
 * is accepted (analytical.rs:56-58, 82-85, 115-116), so a material is a PATCH —
 * a field mask plus values — applied over Material::new() (material.rs:82-114) in
 * primitive order.                                                             */

enum {                                /* rpt_material.mask bits */
    RPT_MAT_RGB             = 1u << 0,
    RPT_MAT_EMISSION        = 1u << 1,
    RPT_MAT_ANISOTROPIC     = 1u << 2,
    RPT_MAT_METALLIC        = 1u << 3,
    RPT_MAT_ROUGHNESS       = 1u << 4,
    RPT_MAT_SUBSURFACE      = 1u << 5,
    RPT_MAT_SPECULAR_TINT   = 1u << 6,
    RPT_MAT_SHEEN           = 1u << 7,
    RPT_MAT_SHEEN_TINT      = 1u << 8,
    RPT_MAT_CLEARCOAT       = 1u << 9,
    RPT_MAT_CLEARCOAT_GLOSS = 1u << 10,
    RPT_MAT_SPEC_TRANS      = 1u << 11,
    RPT_MAT_IOR             = 1u << 12,
    RPT_MAT_ALL             = (1u << 13) - 1u,   /* every BSDF field */
    RPT_MAT_MEDIUM          = 1u << 13           /* Material.medium (all four fields at once); only read under RPT_SCENE_MEDIA */
};

enum { RPT_MEDIUM_NONE = 0, RPT_MEDIUM_ABSORB = 1, RPT_MEDIUM_SCATTER = 2, RPT_MEDIUM_EMISSIVE = 3 };   /* MediumType, material.rs:8-13 */

enum {                                /* rpt_material.proc_kind */
    RPT_PROC_NONE        = 0,
    /* rgb = checker(dir.x/dir.y*s + o, dir.z/dir.y*s + o) ? a : b   (analytical.rs:107-115);
     * proc_params = {s, o, a, b}.  Sets rgb regardless of RPT_MAT_RGB.          */
    RPT_PROC_CHECKER_DIR = 1
};

typedef struct rpt_material {         /* user-set fields of material.rs:48-78 that the tracer reads */
    uint32_t mask;
    uint32_t proc_kind;
    float rgb[3];
    float emission[3];
    float anisotropic;
    float metallic;
    float roughness;
    float subsurface;
    float specular_tint;
    float sheen;
    float sheen_tint;
    float clearcoat;
    float clearcoat_gloss;
    float spec_trans;
    float ior;
    float proc_params[4];
    /* Material.medium (material.rs:16-21, 75, 107): see "participating media" below */
    uint32_t medium_type;
    float medium_density;
    float medium_color[3];
    float medium_anisotropy;
} rpt_material;

typedef struct rpt_sphere {           /* analytical.rs:166-190 */
    float    center[3];
    float    radius;
    uint32_t material;                /* index into rpt_scene_desc.materials */
} rpt_sphere;

typedef struct rpt_plane {            /* analytical.rs:193-204 generalised: dot(point - o, n) / dot(n, d) */
    float    normal[3];
    float    point[3];
    float    min_denom;               /* reject |dot(n,d)| <= min_denom (1e-4 in the reference) */
    uint32_t material;
    float    max_t;                   /* > 0: also reject t > max_t (a floor of finite reach); 0 = the reference's infinite plane */
} rpt_plane;

enum { RPT_LIGHT_RECTANGULAR = 0, RPT_LIGHT_SPHERICAL = 1, RPT_LIGHT_DISTANT = 2 };  /* globals.rs:69-73 */

/* globals.rs:76-84.  The reference samples and intersects only SPHERICAL lights (tracer.rs:175-217, scene.rs:68).
 * With RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES the other two declared types work too — project-defined, after the
 * renderer tracer.rs is a port of (its comments "Required for quad lights with single sided emission",
 * tracer.rs:148, and "No MIS for distant light", tracer.rs:158, are that renderer's), in the operation order
 * written in oracle/rpt_oracle.hpp:
 *   RECTANGULAR  the parallelogram position + a*u + b*v, a,b in [0,1]; area = |u x v| (the caller supplies it);
 *                sampled uniformly (2 draws), pdf = dist^2 / (area * |n.dir|), n = normalize(u x v); emits from the
 *                side n points to; a ray reaching it from that side ends the path like a spherical light does.
 *   DISTANT      direction = normalize(position), no draws, dist = +inf, pdf = 1, area = 0 (so no MIS weight);
 *                never intersected. */
typedef struct rpt_light {
    uint32_t type;
    float    position[3];
    float    emission[3];
    float    u[3];
    float    v[3];
    float    radius;
    float    area;                    /* 4*pi*r*r for a spherical light (light.rs:22) */
} rpt_light;

typedef struct rpt_camera {           /* camera/pinhole.rs:6-25 */
    float origin[3];
    float center[3];
    float fov_deg;
} rpt_camera;

enum {
    RPT_BG_CONSTANT   = 0,            /* colour_a * scale */
    /* t = 0.5*(dir.y+1); to_linear((1-t)*colour_a + t*colour_b) * scale
     * (analytical.rs:28-32, to_linear = powf(gamma) per channel, scene.rs:32-34) */
    RPT_BG_GRADIENT_Y = 1
};

typedef struct rpt_background {
    uint32_t kind;
    float    colour_a[3];
    float    colour_b[3];
    float    gamma;
    float    scale;
} rpt_background;

/* ---- procedural SDF object (BASELINE.json configs[3]; the reference has no SDF scene, Readme.md:18) ----
 * One implicit surface per scene: the polynomial smooth union of a list of primitives,
 *     d = fold(smin_k) over prims,   smin_k(a,b) = min(a,b) - h*h*k*0.25,  h = max(k - |a-b|, 0) * (1/k)
 * (1/k is the f32 quotient 1.0f / k, computed once)
 * found by sphere marching from t = 0:  p = o + t*d;  hit when sdf(p) < hit_eps * t;  t += sdf(p);
 * miss after max_steps steps or when t > max_t.  Normal = normalised tetrahedral gradient with step
 * normal_eps.  The object is tested AFTER the spheres and planes (accepted when nearer) and counts as
 * an occluder in any_hit.  All arithmetic is f32, in exactly this order (tests/media_sdf_f64.py restates it from this text):
 *   Primitives, with q = p - center:
 *     sphere        length(q) - r                                  (length = sqrt(q.x*q.x + q.y*q.y + q.z*q.z), fx.rs)
 *     torus about y sqrt(qx*qx + q.y*q.y) - r_minor,   qx = sqrt(q.x*q.x + q.z*q.z) - R
 *   Fold, left to right from primitive 0 (a = the running value, b = the next primitive's; one primitive: no fold):
 *     h = max(k - |a - b|, 0) * (1/k);   m = a < b ? a : b;   a = m - h*h*k*0.25       (products left to right)
 *   March:  t = 0;  at most max_steps times:
 *     1. dist = sdf(o + t*d)                                       (o + t*d = origin + direction * t, ray.rs)
 *     2. if dist < hit_eps * t: a hit at t        (at t = 0 that is dist < 0: an origin inside the object hits at t = 0)
 *     3. t = t + dist
 *     4. if t > max_t: a miss
 *     and a miss when the steps run out.
 *   Normal at p:  n = sdf(p + e*k0)*k0 + sdf(p + e*k1)*k1 + sdf(p + e*k2)*k2 + sdf(p + e*k3)*k3, summed in that order, with
 *     e = normal_eps and k0..k3 = (1,-1,-1), (-1,-1,1), (-1,1,-1), (1,1,1);  then n / length(n).
 *   closest_hit:  after the last plane, with `first` and `dist` as the spheres and planes left them (first: no primitive was tested yet,
 *     whether or not one was hit): a hit of the march at t is accepted when first || t < dist; then state.hit_dist = t, state.normal =
 *     the normal at o + t*d, the material patch `material` is applied, dist = t.  After it come Scene::sample_lights.
 *   any_hit:  the object goes last; a hit of the march at t occludes under the scene's rule (RPT_SCENE_ANYHIT_USES_MAX_DIST: only when
 *     t < max_dist). */
enum { RPT_SDF_SPHERE = 0, RPT_SDF_TORUS_Y = 1 };

typedef struct rpt_sdf_prim {
    uint32_t kind;
    float    center[3];
    float    params[2];               /* sphere: {radius, -}; torus around the y axis: {major R, minor r} */
} rpt_sdf_prim;

typedef struct rpt_sdf {
    uint32_t n_prims;                 /* 0 = no SDF object; at most 8 */
    uint32_t max_steps;               /* at most 65536 */
    uint32_t material;
    float    smooth_k;
    float    hit_eps;
    float    max_t;
    float    normal_eps;
    const rpt_sdf_prim* prims;
} rpt_sdf;

enum {                                /* rpt_scene_desc.flags */
    /* Scene::any_hit honours max_dist.  OFF reproduces analytical.rs:130, which
     * ignores it (anything along the shadow ray occludes). */
    RPT_SCENE_ANYHIT_USES_MAX_DIST = 1u << 0,
    /* Sample and intersect RECTANGULAR and DISTANT lights (project-defined, see rpt_light).  OFF reproduces the
     * reference, whose sample_light and Scene::sample_lights only know LightType::Spherical (tracer.rs:175-217,
     * scene.rs:68): such lights are still picked by the light-index draw but contribute nothing. */
    RPT_SCENE_SAMPLE_ALL_LIGHT_TYPES = 1u << 1,
    /* Participating media (project-defined, see below).  OFF reproduces the reference, which never reads a Medium. */
    RPT_SCENE_MEDIA = 1u << 2
};

/* ---- participating media — PROJECT-DEFINED: THERE IS NO REFERENCE BEHAVIOUR TO MATCH ----------------
 * The reference declares Medium {medium_type, density, color, anisotropy} (material.rs:8-34), carries one in every Material
 * (material.rs:75,107) and one in State (globals.rs:19,37), clamps the anisotropy in Material::finalize (material.rs:126) —
 * and tracer.rs never reads any of it ("Support of mediums / volumetric objects" is a Todo, Readme.md:13).  With
 * RPT_SCENE_MEDIA the fields mean what they mean in the renderer tracer.rs is a port of (its default build: homogeneous
 * media bounded by surfaces, no nesting, binary shadow rays), made consistent in two places (marked *): the medium acts on
 * a segment BEFORE what lies at its end is looked at, and a light sample taken inside a medium is attenuated by it.  The
 * arithmetic (f32, operation order) is the one written in oracle/rpt_oracle.hpp, Tracer::sample_pixel; exp and ln are
 * rpt_expf / rpt_logf of include/rpt_strict_math.h.
 *
 * A path carries `in_medium` (false at the camera) and a copy of the medium it is in (State.medium).  One iteration of
 * the bounce loop (tracer.rs:61-103) becomes:
 *   1. state.is_emitter = false (the reference never clears it, which is harmless only because an emitter hit ends the
 *      path there; here a path can go on after one).  closest_hit; a miss adds the background and ends the path as always
 *      (also inside a medium: a medium acts only on segments that end on something).
 *   2.* if in_medium, over seg = state.hit_dist:
 *        ABSORB    throughput.c *= exp(-(((1 - color.c) * seg) * density))            per channel (Beer-Lambert)
 *        EMISSIVE  radiance += ((color * seg) * density) * throughput
 *        SCATTER   one draw r;  d = min(-ln(r) / density, seg)  (f32::min);  if d < seg the path SCATTERS at p = ray.at(d):
 *                    throughput *= color;
 *                    next-event estimation from p exactly as direct_light (tracer.rs:126-170) with scatter_pos = p (no
 *                    offset) and the phase function in place of the BSDF: f = pdf = phase_hg(dot(-ray.direction,
 *                    light.direction), g), same MIS weight, same `pdf > 0` guard;  * the unoccluded light's `li` is
 *                    attenuated over light_sample.dist exactly as in step 3 (the scatter point lies inside the medium: the medium is
 *                    both the phase function and what the light crosses), the max_dist of the shadow ray is dist - eps as always;
 *                    two draws r1, r2;  dir = sample_hg(-ray.direction, g, r1, r2);  scatter_sample.pdf =
 *                    phase_hg(dot(-ray.direction, dir), g);  scatter_sample.l = dir;  ray = Ray(p, dir)  (no eps offset);
 *                    then Russian roulette as after a surface bounce, and the next iteration.  The iteration counts
 *                    against max_depth like a surface bounce; in_medium stays as it is.
 *      g = the medium's anisotropy, clamped to [-0.9, 0.9] by Material::finalize (material.rs:126).
 *   3. (no scatter event) the reference's iteration as it is: State::finalize, emission, the emitter exit — its MIS weight
 *      reads scatter_sample.pdf, which after a medium scatter is the phase pdf —, direct_light, disney_sample, next ray.
 *      * In direct_light, when in_medium and light_sample.dist is finite, the unoccluded light's `li` is multiplied by the
 *      medium's transmittance over light_sample.dist: ABSORB exp(-(((1 - color.c) * dist) * density)) per channel,
 *      SCATTER exp(-(dist * density)), EMISSIVE 1.  (Shadow rays are the scene's binary any_hit, so this matters for lights
 *      INSIDE a medium — use RPT_SCENE_ANYHIT_USES_MAX_DIST there; a medium's own boundary occludes lights outside it.)
 *   4. after the next ray is set (tracer.rs:100-101), if state.material.medium.medium_type != NONE:
 *        in_medium = dot(ray.direction, state.normal) < 0      (the NEW direction against the geometric normal: entering)
 *        and when that is true state.medium = state.material.medium.
 *      Media are entered and left through their boundary surface (a refraction into it, spec_trans > 0, or any scatter
 *      that ends up on the inner side); there is no stack: media do not nest.
 *   phase_hg(c, g)  = INV_4_PI * (1 - g*g) / (d * sqrt(d)),  d = 1 + g*g + 2*g*c,  INV_4_PI = 1 / (4 * PI)  (f32)
 *   sample_hg(v, g, r1, r2):  cos = |g| < 0.001 ? 1 - 2*r2 : -(1 + g*g - q*q) / (2*g),  q = (1 - g*g) / (1 + g - 2*g*r2);
 *                             phi = r1 * TWO_PI;  sin = clamp(sqrt(1 - cos*cos), 0, 1);  (t, b) = onb(v)  (tracer.rs:184-189);
 *                             dir = (sin * cos(phi)) * t + (sin * sin(phi)) * b + cos * v
 * Draw order of an iteration inside a SCATTER medium: the distance draw; then, on a scatter event, light index, light r1,
 * r2 (if the scene has lights), r1, r2 of sample_hg, [roulette]; otherwise the surface bounce's draws as always.
 * Materials of small scenes are patches: RPT_MAT_MEDIUM writes all four medium fields.  rpt_upload_scene rejects a
 * negative or non-finite density.  Kernel forms: every scene class's kernel renders media (megakernel, the compacting
 * kernel, the SDF march kernel, large scenes' megakernel); RPT_RENDER_FAST_MATH and RPT_RENDER_NESTED_LOOPS do not
 * (RPT_ERR_UNSUPPORTED). */

/* ---- triangle meshes (the reference's Todo "Implement a mesh based example scene", Readme.md) — PROJECT-DEFINED -------------
 * A mesh is a list of triangles over a vertex array, with ONE material.  The triangles of all meshes form one flattened list:
 * meshes in order, each mesh's triangles in order; a triangle's index below is its position in that list.
 *
 * Triangle test (two-sided Moller-Trumbore), f32 in exactly this operation order; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x) (fx.rs:335-344), the divide is the library's
 * correctly rounded one.  For a ray (o, d) and a triangle (a, b, c):
 *     e1 = b - a;  e2 = c - a;  p = cross(d, e2);  det = dot(e1, p)
 *     !(det < 0 || det > 0)          -> miss   (also a NaN det)
 *     inv = 1 / det;  s = o - a;  u = dot(s, p) * inv
 *     !(u >= 0 && u <= 1)            -> miss
 *     q = cross(s, e1);  v = dot(d, q) * inv
 *     !(v >= 0 && u + v <= 1)        -> miss
 *     t = dot(e2, q) * inv
 *     !(t >= 0 && t < F::MAX)        -> miss   (F::MAX = 3.40282347e38: so a hit always has t < the running distance's start value,
 *                                              and the "first primitive is accepted whenever hit" rule never changes a triangle's result)
 *     point check, per axis i = x, y, z (min / max of finite numbers):
 *       lo = a.i + min(min(0, e1.i), e2.i);  hi = a.i + max(max(0, e1.i), e2.i);  w = (max(|lo|, |hi|) + |o.i|) * 2^-16;
 *       p = o.i + t * d.i;  !(lo - w <= p && p <= hi + w) -> miss
 *     (A hit whose point lies outside the triangle's box by more than the rounding of the test can produce: what a ray lying in
 *     the triangle's plane to f32 precision gets, whose det is rounding noise.  The check makes every hit lie near its triangle,
 *     which is what lets the library's hierarchy give exactly the loop's answer: DESIGN.md 4c.)
 * Normal: normalize(cross(e1, e2)), NOT turned toward the ray; State::finalize computes ffnormal from it as for planes.
 *
 * closest_hit: spheres, then planes, then the triangles in flattened order, then Scene::sample_lights.  A triangle is accepted
 * when t < dist (dist = the running closest distance), so the result is the nearest triangle nearer than everything before it,
 * the lowest flattened index on equal t.  any_hit: any triangle hit with (!use_max || t < max_dist).
 *
 * Materials: a scene with meshes follows the large scenes' rule — every sphere and mesh material must be a full patch
 * ((mask & RPT_MAT_ALL) == RPT_MAT_ALL, proc_kind == RPT_PROC_NONE); planes may carry any patch (at most 4 planes).  A triangle
 * that wins therefore leaves its own material.  A mesh's emission counts when a path hits it, as for spheres; a mesh is a
 * light for next-event estimation only while rpt_set_mesh_lights has turned it ON (below, "mesh lights").
 *
 * Limits: at most RPT_MESH_MAX_TRIANGLES triangles in all, n_spheres + triangles below 2^28 - 1, and the scene's device tables
 * (spheres, lights, materials, triangles at 48 B, BVH nodes at 64 B: at most one per triangle) below 4 GiB (RPT_ERR_UNSUPPORTED).
 * rpt_upload_scene answers
 *   RPT_ERR_INVALID_ARG  a vertex index >= n_vertices, a non-finite vertex, a NULL array with a non-zero count (vertices,
 *                        indices, or meshes), a material index out of range;
 *   RPT_ERR_UNSUPPORTED  meshes together with RPT_SCENE_MEDIA or an SDF object, a sphere or mesh material that is not a full patch,
 *                        more than the limits above;
 * and rpt_render* answer RPT_ERR_UNSUPPORTED for RPT_RENDER_FAST_MATH, RPT_RENDER_NESTED_LOOPS and RPT_RENDER_SMALL_COMPACT on a
 * scene with meshes (the scene class has one, strict kernel: like media).  A scene whose meshes hold no triangle at all is not
 * a mesh scene.  The library builds a bounding volume hierarchy over the triangles at upload; it returns exactly
 * what the ordered loop above returns, for every ray (a ray with a NaN component hits no triangle; one with an infinite component,
 * and every ray of a scene with a vertex coordinate beyond 2^60, is served by the loop itself). */
#define RPT_MESH_MAX_TRIANGLES (1u << 26)

typedef struct rpt_mesh {
    uint32_t n_vertices;  const float*    vertices;   /* xyz, 3 floats per vertex */
    uint32_t n_triangles; const uint32_t* indices;    /* 3 vertex indices per triangle */
    uint32_t material;                                /* index into rpt_scene_desc.materials */
} rpt_mesh;

typedef struct rpt_scene_desc {
    uint32_t abi_version;             /* RPT_ABI_VERSION */
    uint32_t flags;
    rpt_camera     camera;
    rpt_background background;
    float    eps;                     /* Tracer.eps = 0.005 (tracer.rs:16) */
    uint32_t max_depth;               /* Scene::recursion_depth() = 4 (scene.rs:28-30); at most 4096 */
    uint32_t n_spheres;   const rpt_sphere*   spheres;    /* tested first, in order */
    uint32_t n_planes;    const rpt_plane*    planes;     /* then planes, in order  */
    uint32_t n_lights;    const rpt_light*    lights;     /* then Scene::sample_lights */
    uint32_t n_materials; const rpt_material* materials;
    rpt_sdf  sdf;                     /* then the SDF object, if any */
    uint32_t n_meshes;    const rpt_mesh*     meshes;     /* then the meshes' triangles (after the planes: see "triangle meshes") */
} rpt_scene_desc;

/* Fill `out` with renderer/src/analytical.rs's AnalyticalScene (2 spheres, plane,
 * 1 spherical light, Pinhole defaults).  The arrays it points to are static.  */
int rpt_scene_analytical(rpt_scene_desc* out);

/* ---- render flags ----------------------------------------------------------
 * Bits 2-4, 6-7 and 9-10 named measured-slower kernel forms kept for A/B runs until ABI 3 (inline / three-room / pool / compacting SDF
 * marches, the resumable grid walk, the wavefront form of large scenes and its counterpart flag).  Those forms are gone from the
 * library (profiles/NOTES.md has their numbers, the history their code); the bits are reserved and rpt_render* answer them with
 * RPT_ERR_INVALID_ARG. */
enum {
    RPT_RENDER_DEFAULT      = 0u,
    /* Small scenes without an SDF object or media: the nested-loop kernel (sample loop outside, bounce loop inside) instead of
     * the path-regenerating one.  Same image bit for bit; the differential baseline of the reference's own scene class. */
    RPT_RENDER_NESTED_LOOPS = 1u << 0,
    /* Relaxed arithmetic: the same kernels built with hipcc's fast f32 divide/sqrt and FMA contraction.
     * Not bit-identical to the reference arithmetic (statistically equivalent: SURVEY.md 8c tier T1); off by default; bench.py
     * reports it beside the headline, never as the headline.  Its device arithmetic against float64 (tests/test_gpu_relaxed.py,
     * measured on an MI355X): divide <= 2.5 ulp (largest seen 1.91), square root <= 2.5 ulp (0.92), over every finite operand —
     * hipcc's sequences scale by the operands' exponents, so denormal operands and results and huge denominators stay within
     * that; zeros, infinities and NaNs give IEEE's answers — and include/rpt_strict_math.h's functions keep their bounds under
     * contraction (sin / cos 1.41 ulp, log2 / log / pow / exp 0.50).  Every relaxed kernel's frame is held to the f64 oracle's
     * with bounds taken from the strict frame's distance to it (flipped pixels <= 2.5x + 6, median <= 4x; measured 0.25-2x and
     * 0.7-2x).  The relaxed build has no range guards and needs none: the stock scene scaled by 2^-31, 2^-20, 2^30 and 2^31 stays
     * finite and within those bounds (from 2^23 up, of the f32 oracle's frame: the reference's f32 camera quantises its rays there). */
    RPT_RENDER_FAST_MATH    = 1u << 1,
    /* Russian roulette (project-defined; the reference's bounce loop is a fixed `for _ in 0..depth` with three
     * early exits, tracer.rs:61-103).  After the throughput update and the next-ray set-up of bounce b (0-based),
     * when b + 1 >= 2 and b + 1 < depth:  q = clamp(max(throughput.x, throughput.y, throughput.z), 0.05, 1)
     * (f32::max, so a NaN component is ignored);  one more draw r (after the bounce's other draws);  r >= q ends
     * the path, otherwise throughput = throughput / q.  Same expectation, different samples: OFF (the default) is
     * the reference.  Worth it for deep paths (max_depth > 4). */
    RPT_RENDER_RUSSIAN_ROULETTE = 1u << 5,
    /* Small scenes without an SDF object: use the kernel that keeps the workgroup's 256 paths in LDS and re-deals them to its
     * threads before every stage.  It is what a launch of ONE sample per pixel takes by default — the reference's
     * own usage, one render() per redraw, where the megakernel has nothing to regenerate over and its waves drain (+4 % at 1080p,
     * more on small frames) — and slower than the megakernel from two samples per launch up; the flag forces it at any sample
     * count (tests).  Same image bit for bit. */
    RPT_RENDER_SMALL_COMPACT = 1u << 8,
    RPT_RENDER_ALL_FLAGS = RPT_RENDER_NESTED_LOOPS | RPT_RENDER_FAST_MATH | RPT_RENDER_RUSSIAN_ROULETTE | RPT_RENDER_SMALL_COMPACT
};

/* ---- context --------------------------------------------------------------- */
typedef struct rpt_ctx rpt_ctx;

/* Create a context on HIP device `device_id` (must be gfx950).  Replaces
 * Tracer::new (tracer.rs:13-19) together with rpt_upload_scene. */
int rpt_create(rpt_ctx** out, int device_id);
void rpt_destroy(rpt_ctx* ctx);
const char* rpt_last_error(const rpt_ctx* ctx);   /* valid until the next call on ctx; ctx may be NULL */
uint32_t rpt_abi_version(void);
/* sizeof(rpt_scene_desc) as this library was built: a binding in another language asserts it against its own
 * mirror of the struct before the first rpt_upload_scene (rust/gpu_tracer.rs does). */
uint32_t rpt_sizeof_scene_desc(void);
/* 0 for the shipped library (librpt_hip.so: exactly this header).  1 for the test build (librpt_hip_test.so): the same objects
 * linked with the hooks of include/rpt_test.h — per-function probes, grid-query probes, dispatch read-outs — which the parity
 * tests use to localise a mismatch. */
uint32_t rpt_build_has_test_hooks(void);

/* ---- the GPUs of one node (what replaces rayon's fan-out, tracer.rs:29-32) -----------------------------
 * The reference's only parallel construct is INSIDE render(): one rayon task per scanline.  Here the image is
 * row-tiled over the GPUs: rows are dealt cyclically in blocks of `tile_rows` rows (default 2; block b -> rank
 * b % world; sky rows are ~10x cheaper than floor rows, so contiguous slabs would not balance), each GPU keeps
 * its rows as a compact tile in its own HBM, ranks exchange nothing while rendering, and one RCCL gather over
 * xGMI brings the tiles to the root (rank 0), where a small kernel scatters them into the top-down image.
 * The RNG is keyed by the global pixel, so the image does not depend on the number of GPUs.
 *
 * Two ways to get there, same entry points afterwards:
 *   rpt_create_multi   ONE process drives n devices (one host thread, one stream + tile per device,
 *                      ncclCommInitAll): rpt_render / rpt_resident_* on such a context fan out over the
 *                      devices inside the call, exactly where the reference fans out over threads.
 *   rpt_create_rank    one process per GPU (torch.distributed.run, MPI, ...): rank 0 calls
 *                      rpt_comm_unique_id, the host distributes those 128 bytes over any channel it has, every
 *                      rank calls rpt_create_rank (ncclCommInitRank: collective).  rpt_resident_render,
 *                      rpt_resident_gather_device, rpt_resident_download[_u8] are then collective calls: every
 *                      rank makes them in the same order; destinations are only written on rank 0.
 * A context from rpt_create is world = 1.
 * rpt_create_multi accepts a device more than once: each entry is a rank of its own (own stream, own tile), and the launches of
 * one GPU's ranks run side by side, so that in a progressive render (rpt_resident_render called again and again) one rank's
 * launch fills the tail of the other's: +5 % on a resident 1920x1080 frame with the device listed twice, +22 % on 3840x270.
 * Such contexts gather their tiles with peer / device copies instead of RCCL (which needs one device per rank).             */
#define RPT_UNIQUE_ID_BYTES 128
typedef struct rpt_unique_id { char bytes[RPT_UNIQUE_ID_BYTES]; } rpt_unique_id;

int rpt_create_multi(rpt_ctx** out, const int* device_ids, int n_devices);
int rpt_comm_unique_id(rpt_unique_id* out);
int rpt_create_rank(rpt_ctx** out, int device_id, int rank, int world, const rpt_unique_id* id);
/* rank of this context's first device, number of ranks in all, number of devices this context drives */
int rpt_world(const rpt_ctx* ctx, int* rank, int* world, int* n_local);
/* Rows per cyclic block for the NEXT resident buffer / rpt_render call (0 < tile_rows). */
int rpt_set_tile_rows(rpt_ctx* ctx, uint32_t tile_rows);

/* How the context's launches are dispatched.  None of this changes a pixel: it decides when and where a sample is computed.
 * A workgroup of the render kernels computes a UNIT: one 16x16 tile x one chunk of the launch's samples.
 *   cost_order     1 (default): within a chunk the tiles are dispatched most expensive first, as timed by the context's previous
 *                  launch of the same shape, so that the cheap ones fill the launch's tail; 0: bottom rows first, always
 *   unit_rounds    a launch whose tiles are fewer than this many rounds of workgroups on the device (default 12) is cut into
 *                  chunks of samples until they are — a tile's chunks are handed from workgroup to workgroup through HBM, in
 *                  order —; 0: one unit per tile (and launches of more samples than the kernel's sample tables hold — 512, 192 for
 *                  scenes with the SDF object — are still one launch: chunks of that many)
 *   unit_min_spp   ... but no chunk shorter than this many samples (default 64)
 *   unit_slots     workgroups the device holds at once; 0 (default): 5 per compute unit
 * Environment defaults: RPT_DISPATCH_ORDER, RPT_UNIT_ROUNDS, RPT_UNIT_MIN_SPP.                                               */
int rpt_set_dispatch(rpt_ctx* ctx, uint32_t cost_order, uint32_t unit_rounds, uint32_t unit_min_spp, uint32_t unit_slots);

/* Copy the scene into the context (Tracer owns its scene: tracer.rs:8). */
int rpt_upload_scene(rpt_ctx* ctx, const rpt_scene_desc* scene);

/* ---- moving meshes — PROJECT-DEFINED ------------------------------------------------------------------------------------------
 * New vertex positions for meshes of the uploaded scene, without the upload: the scene's meshes keep their indices, materials
 * and triangle order, and each mesh named in `updates` gets the positions given — all of its vertices.  Afterwards the context
 * renders exactly what it would render after rpt_upload_scene of the same descriptor with those vertex arrays: the same frames
 * bit for bit, the same errors from rpt_render*.
 *
 * The hierarchy keeps its shape and gets new boxes, computed on the device (a refit: DESIGN.md 4c).  No result depends on that;
 * speed can: the shape was chosen for the uploaded positions, and after a large deformation a fresh rpt_upload_scene walks
 * faster.  Measured on an MI355X, scenes.mesh_scene (393 216 triangles) at 1920x1080 (tools/mesh_bench.py --update,
 * profiles/NOTES.md): an update takes 0.62-0.65 ms (the context's first one 2.2 ms: it allocates) where the upload of the same
 * moved scene takes 184-191 ms; and after a ripple of 1.25 % of the icosphere's radius with the torus turned by 0.05 rad a fresh
 * upload rendered 1.4 % faster than the refitted hierarchy, after 12.5 % and 0.5 rad 35 % faster, after 25 % and 2 rad 74 % faster.
 * Update while a mesh only moves; upload again once its shape has changed.
 *
 * The call blocks until every device of the context has finished its earlier work and holds the new tables (like
 * rpt_upload_scene, whose hipFree waits for the device); launches the caller has put on streams of its own through
 * rpt_render_device must be ordered by the caller, as for an upload.  The resident ColorBuffer is left alone, as rpt_upload_scene
 * leaves it: the caller resets it.  The learned dispatch order is kept (it never changes a pixel, and a small move leaves the
 * tile costs good predictors).  A context of several devices (rpt_create_multi) updates every one; with one process per GPU
 * (rpt_create_rank) every rank makes the call itself, as for an upload.
 *
 * n_updates == 0 is RPT_OK and does nothing.  A mesh without triangles may be named: its count is checked and nothing else
 * happens.  Everything below but RPT_ERR_HIP is checked on the host before any device is touched, in this order, so that a
 * rejected call leaves the context exactly as it was:
 *   RPT_ERR_INVALID_ARG  ctx is NULL; updates is NULL with a non-zero count;
 *   RPT_ERR_NO_SCENE     no scene is uploaded, or the uploaded scene is not a mesh scene (it holds no triangle);
 *   RPT_ERR_UNSUPPORTED  the scene's meshes hold 2^32 vertices or more in all;
 *   RPT_ERR_INVALID_ARG  per update, in order: mesh >= the scene's n_meshes; a mesh named twice; n_vertices different from the
 *                        uploaded mesh's; vertices NULL with a non-zero count; a non-finite coordinate (rpt_last_error names the
 *                        mesh and the vertex);
 *   RPT_ERR_HIP          a runtime call failed part-way.  The tables may then be half written, so the context is left with NO
 *                        scene (its tables freed; rpt_render* answer RPT_ERR_NO_SCENE until the next rpt_upload_scene).
 * As at upload, while a coordinate some triangle uses lies beyond 2^60 the ordered loop serves every ray; an update that brings
 * all of them back turns the hierarchy's walk on again.
 *
 * Memory.  On the host a mesh scene keeps, from its upload to the context's first update, a copy of its vertices and indices
 * (12 B per vertex + 12 B per triangle + 4 B per hierarchy node), and for its whole life 1 B per vertex.  The first update
 * allocates on every device, until the next rpt_upload_scene, 12 B per vertex + 36 B per triangle + 4 B per hierarchy node (the
 * vertices, each triangle's vertex indices and box, the refit order) — about half of the scene's own triangle and node tables —
 * and releases the host copy.  A context that is never updated allocates nothing on a device. */
typedef struct rpt_mesh_vertices {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t n_vertices;              /* must equal that mesh's n_vertices */
    const float* vertices;            /* xyz, 3 floats per vertex: the mesh's new positions, all of them */
} rpt_mesh_vertices;

int rpt_update_meshes(rpt_ctx* ctx, const rpt_mesh_vertices* updates, uint32_t n_updates);

/* ---- rebuilding a moved mesh's hierarchy — PROJECT-DEFINED ---------------------------------------------------------------------
 * rpt_update_meshes, and then a NEW hierarchy: the meshes named in `updates` get the positions given, and every device of the
 * context builds a hierarchy over all triangles of the scene on the device — new shape, new leaf order, new boxes (DESIGN.md 4c:
 * the triangles sorted by a Morton code of their centroids, split top-down where the code's highest differing bit changes, under
 * the upload's depth rule).  Afterwards the context renders exactly what it would render after rpt_upload_scene of the same
 * descriptor with those vertex arrays: the same frames bit for bit, the same errors from rpt_render*.
 *
 * Arguments and checks are rpt_update_meshes', in its order, all on the host before any device is touched, so that a rejected
 * call leaves the context exactly as it was; rpt_last_error names this call.  One difference: n_updates == 0 is not a no-op — it
 * rebuilds over the positions the context holds (`updates` may then be NULL), and only RPT_ERR_NO_SCENE and RPT_ERR_UNSUPPORTED
 * (2^32 vertices) can reject it.  RPT_ERR_HIP: a runtime call failed part-way, an allocation among them, or the build did not end
 * within the walk's 24 levels (the depth rule excludes it; such a table is never bound): the context is left with NO scene.
 * The 2^60 rule is unchanged: whether the walk or the ordered loop serves the rays follows the positions, and the tables a
 * rebuild leaves are valid either way.
 *
 * A later rpt_update_meshes refits the rebuilt shape; a later rebuild starts from whatever is there; rpt_upload_scene drops
 * everything a rebuild allocated.  Blocking, streams, the resident ColorBuffer, the learned dispatch order, contexts of several
 * devices and one process per GPU: all as for rpt_update_meshes.  The same positions give the same tables, byte for byte, on every
 * device and at every call.
 *
 * Memory.  The context's first rebuild allocates on every device, until the next rpt_upload_scene: the refit's tables with room
 * for any hierarchy (12 B per vertex + 40 B per triangle), a node table of its own (64 B per triangle; the upload's stays where
 * it is, unused), and the build's work area (76 B per triangle and the sort's temporary storage) — for scenes.mesh_scene
 * about 80 MB beside the scene's own 34 MB.
 *
 * When to use which.  Measured on an MI355X, scenes.mesh_scene (393 216 triangles) at 1920x1080 x 16 spp (tools/mesh_bench.py
 * --rebuild, profiles/NOTES.md; medians of 5, alternating): a rebuild takes 1.10-1.11 ms (the context's first one 8.6 ms: it
 * allocates) where an update takes 0.62 ms and the upload of the same moved scene 188-192 ms.  Render rates afterwards, in
 * Gsamples/s, refit / rebuilt / fresh upload: after a ripple of 1.25 % of the icosphere's radius with the torus turned by 0.05 rad
 * 0.803 / 0.705 / 0.814; after 12.5 % and 0.5 rad 0.460 / 0.537 / 0.623; after 25 % and 2 rad 0.278 / 0.418 / 0.483.  A rebuilt
 * (Morton-order) hierarchy walks at 86-87 % of the upload's binned-SAH one whatever the move, a refitted one at 99 % down to 58 %:
 * update while a mesh only moves or ripples; rebuild once its shape has changed — somewhere before the medium move here —, every
 * frame if need be; and upload again only where the scene then stays put for long, since the host build's extra 190 ms buy 15 %
 * of the render rate (here: from about twenty such frames on). */
int rpt_rebuild_meshes(rpt_ctx* ctx, const rpt_mesh_vertices* updates, uint32_t n_updates);

/* ---- moving meshes from device memory — PROJECT-DEFINED -------------------------------------------------------------------------
 * rpt_update_meshes and rpt_rebuild_meshes for positions that already live in device memory (a skinning, cloth or simulation
 * step's output), with an optional affine transform per mesh applied on the device while they are read: a caller who keeps a
 * rest pose in device memory moves a mesh rigidly with that array and twelve floats per frame — the library keeps no rest pose of
 * its own, and nothing drifts.
 *
 * Meaning.  Let P(m) be, for each mesh m named in `sources`, the positions computed from vertices_dev and transform as written
 * below.  The two calls leave the context in the state rpt_update_meshes / rpt_rebuild_meshes would leave it in, given P as host
 * arrays: the same frames bit for bit, the same triangle and node tables byte for byte, the same errors from rpt_render* — and so
 * the frames of a fresh rpt_upload_scene of the descriptor with P.
 *
 * The transform: 12 floats in HOST memory, the rows of a 3x4 matrix t; f32 in exactly this operation order, nothing contracted:
 *     out[c] = ((t[4c]*x + t[4c+1]*y) + t[4c+2]*z) + t[4c+3]        c = 0, 1, 2
 * transform == NULL copies a vertex's three words unchanged, so a -0 stays -0.  An identity matrix is NOT the same thing: it
 * turns -0 into +0 (-0*1 + 0*0 = +0).  The statement is written once, csrc/host_move.h, for the kernel and the host reference.
 *
 * Checks, in this order.  On the host first:
 *   RPT_ERR_INVALID_ARG  ctx is NULL; sources is NULL with a non-zero count;
 *   RPT_ERR_NO_SCENE     no scene is uploaded, or the uploaded scene is not a mesh scene;
 *   RPT_ERR_UNSUPPORTED  the scene's meshes hold 2^32 vertices or more in all;
 *   RPT_ERR_INVALID_ARG  per source, in order: mesh >= the scene's n_meshes; a mesh named twice; n_vertices different from the
 *                        uploaded mesh's; vertices_dev NULL with a non-zero count; vertices_dev not device memory — whatever
 *                        hipPointerGetAttributes does not report as hipMemoryTypeDevice: an error from the query, host memory
 *                        whether page-locked or not, managed memory —, before any kernel is launched; vertices_dev's allocation
 *                        ending before 12 * n_vertices bytes from the pointer on (hipMemGetAddressRange; where the runtime
 *                        reports no range for the memory, and inside a larger allocation such as a pooling allocator's block,
 *                        the extent is the caller's responsibility: the kernels read 3 * n_vertices floats); a non-finite
 *                        entry in transform (rpt_last_error names the mesh and the entry).
 * Then on the device: every coordinate of every named mesh's P must be finite.  A NaN or infinity in the source, or an overflow
 * through the transform, answers RPT_ERR_INVALID_ARG; rpt_last_error names the mesh (the first such source in `sources`) and its
 * lowest offending vertex.  A vertex no triangle references is checked too, as on the host path.
 * A rejected call leaves the context exactly as it was: the check pass transforms in registers and stores no position; only when
 * every source has passed does a second pass compute the same positions again and store them.  A later
 * rpt_rebuild_meshes(ctx, NULL, 0) after a rejection sees the old positions.
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for rpt_update_meshes.
 * The 2^60 rule is unchanged; the per-mesh largest |coordinate| over referenced vertices now comes from the device check.
 *
 * Where the source lives.  vertices_dev may lie on any device of the process.  The check runs on the context's first device; each
 * device of the context reads a source that lies on itself in place, and one that lies elsewhere from a copy into its own memory
 * (hipMemcpyAsync, hipMemcpyDefault).  A context of several devices (rpt_create_multi, also with a device listed twice) brings
 * every one to the same state; with one process per GPU every rank makes the call itself, as for an update.  (The copy of a source
 * from another device is unverified on hardware: the tests run on one GPU, where a context with the device listed twice is what
 * exercises the several-devices loop.)
 *
 * Ordering.  The calls block, like their host forms.  Before a source is read, all earlier work on the device that holds it has
 * finished (hipDeviceSynchronize there): a producer kernel enqueued on any stream before the call is complete.  When the call
 * returns the source has been consumed: the caller may overwrite it at once.  There is no stream argument.
 *
 * n_sources == 0: rpt_update_meshes_device answers RPT_OK and does nothing; rpt_rebuild_meshes_device is
 * rpt_rebuild_meshes(ctx, NULL, 0).  Streams of the caller's own, the resident ColorBuffer, the learned dispatch order: as for
 * rpt_update_meshes.
 *
 * rpt_download_mesh_vertices copies the positions the context holds for one mesh — all its vertices — to host memory: before the
 * context's first update of any kind from the host's copy of the upload, afterwards from its first device's vertex table.  It
 * answers RPT_ERR_INVALID_ARG for a NULL ctx, NULL vertices with a non-zero count, mesh >= n_meshes or n_vertices different from
 * the mesh's, RPT_ERR_NO_SCENE without a mesh scene, RPT_ERR_UNSUPPORTED for 2^32 vertices, and never changes anything.
 *
 * Memory.  The context's first device-source call allocates on its first device, until the next rpt_upload_scene, 1 B per vertex
 * (which vertices a triangle references) + 8 B per mesh (the check's words); a device that reads a source lying on another device
 * keeps 12 B per vertex for the copies.  The refit's and the rebuild's tables are those of rpt_update_meshes /
 * rpt_rebuild_meshes, allocated as there.  No staging copy of the positions exists: the check stores nothing.
 *
 * Timings: tools/mesh_bench.py --device times both forms on scenes.mesh_scene (393 216 triangles, 196 610 vertices) next to
 * the host forms (medians of 5, alternating); no figures are recorded here yet.  What the device forms leave out of the host forms'
 * 0.62 ms and 1.10 ms is the host's scan of 2.4 MB of coordinates and one pageable copy per mesh; what they add is two kernel
 * launches per named mesh, one 8-byte-per-mesh read-back and one more wait. */
typedef struct rpt_mesh_source {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t n_vertices;              /* must equal that mesh's n_vertices */
    const float* vertices_dev;        /* DEVICE memory, xyz, 3 floats per vertex: all of the mesh's vertices */
    const float* transform;           /* HOST memory, 12 floats, rows of a 3x4 matrix; NULL = take the positions as they are */
} rpt_mesh_source;

int rpt_update_meshes_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources);
int rpt_rebuild_meshes_device(rpt_ctx* ctx, const rpt_mesh_source* sources, uint32_t n_sources);
int rpt_download_mesh_vertices(rpt_ctx* ctx, uint32_t mesh, float* vertices /* host */, uint32_t n_vertices);

/* ---- smooth mesh shading — PROJECT-DEFINED --------------------------------------------------------------------------------------
 * Per mesh, a winning triangle is shaded with the interpolated normals of its three vertices instead of normalize(cross(e1, e2)).
 * The library computes the vertex normals on the device from the f32 positions the context holds, and computes them again inside
 * every call that moves a mesh; nothing crosses the host.  Every operation order is stated, so that normals and frames stay
 * checkable bit for bit (tests/test_gpu_mesh_smooth.py holds both to a numpy float32 restatement).  dot, cross and F::MAX are those
 * of "triangle meshes"; the square root and the divides are the library's correctly rounded ones.
 *
 * Vertex normals of a SMOOTH mesh.  Let the mesh's triangles be k = 0, 1, ... in the mesh's own order, (a, b, c) the positions of
 * triangle k's corners.
 *     face vector      g_k = cross(b - a, c - a)      (the e1, e2 and cross of the triangle test; not normalised: area-weighted)
 *     vertex vector    s_j = the sum of g_k over the triangles that name vertex j at one or more corners, each such triangle
 *                      counted ONCE, in ascending k; per component, f32, left to right, starting with the first term.
 *                      No triangle names j: s_j = (0, 0, 0).
 *     l2 = dot(s_j, s_j);  !(l2 > 0 && l2 <= F::MAX)  ->  n_j = (0, 0, 0)     (also a NaN from overflowing edges)
 *     otherwise        n_j = s_j / sqrt(l2), per component: one root, three divides (the reference's normalize)
 * The order is by triangle index within the mesh, never by slot of the hierarchy: rpt_rebuild_meshes reorders slots and leaves
 * every normal bit for bit where it was.
 *
 * Normal of a winning triangle of a SMOOTH mesh.  u and v are the values the triangle test computed for this ray and triangle
 * (the library recomputes them from the unchanged ray and row: the same operations, the same bits); na, nb, nc the vertex
 * normals of its corners a, b, c.
 *     w = (1 - u) - v
 *     m.i = (w * na.i + u * nb.i) + v * nc.i          i = x, y, z
 *     l2 = dot(m, m);  !(l2 > 0 && l2 <= F::MAX)  ->  the flat normal normalize(cross(e1, e2))
 *     otherwise        m / sqrt(l2): one root, three divides
 * Like the flat normal it is NOT turned toward the ray, and everything downstream treats it as today's normal: ffnormal, eta's
 * side, the offset of the next-event ray.  The known cost of that choice: near silhouettes and near the terminator an
 * interpolated normal can face away from the ray that hit the front of its triangle, or lean over a neighbouring facet — the
 * hit is then shaded from the other side, or a shadow ray starts below the neighbour.  The library does not bend the normal.
 * Triangle test, acceptance order, any_hit and materials are unchanged.
 *
 * rpt_set_mesh_shading sets the mode of the named meshes of the uploaded scene, before or after any number of moves or rebuilds;
 * meshes not named keep theirs, and rpt_upload_scene leaves every mesh RPT_MESH_SHADING_FLAT.  On return every SMOOTH mesh's
 * normals are current on every device of the context (rpt_create_multi: all of them; one process per GPU: every rank makes the
 * call itself, as for rpt_update_meshes).  A mesh without triangles may be named.  The checks, in this order, all on the host
 * before any device is touched — a rejected call changes nothing, and rpt_last_error names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_UNSUPPORTED  the scene's meshes hold 2^32 vertices or more;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item: mesh >= n_meshes, a mesh named twice, a mode that is
 *                        neither constant;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for rpt_update_meshes.
 * While some mesh is SMOOTH the scene renders through a kernel of its own (the mesh kernel's body with the normal above); when
 * the last SMOOTH mesh goes back to FLAT the context renders exactly as if the call had never been made — the same kernel, the
 * same tables.  A scene on which the call was never made is untouched by all of this.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms recompute the normals of every SMOOTH mesh on the device
 * before they return RPT_OK (two more kernel launches per device, whatever the number of meshes); a rejected move leaves them as
 * they were.
 *
 * rpt_download_mesh_normals copies the normals the context holds for one SMOOTH mesh — all its vertices, xyz — to host memory from
 * its first device.  It takes rpt_download_mesh_vertices' arguments and gives its answers; a FLAT mesh answers
 * RPT_ERR_INVALID_ARG and says so.  It never changes anything.
 *
 * Memory.  The call brings the refit's tables to every device as the context's first rpt_update_meshes does (and reads the
 * triangles' corners back from the first device once per call: 60 B per triangle over the link; the call is rare).  While a mesh
 * is SMOOTH every device holds, until the last mesh is FLAT again or the next rpt_upload_scene: 20 B per vertex of the SCENE
 * (a 16-byte normal and a 4-byte list offset), per triangle of the SMOOTH meshes 28 B (its face vector, 16 B, and its corners,
 * 12 B) + 4 B per distinct corner (the vertices' lists: 12 B for a proper triangle), and one bit per triangle of the scene.
 *
 * Timings: not measured yet.  tools/mesh_bench.py --smooth alternates, in one process, flat and smooth frames of
 * scenes.mesh_scene and the four move calls with both meshes smooth against flat.  What the normals add to a move is two
 * launches per device over the tables above (scenes.mesh_scene: about 25 MB read and written). */
enum { RPT_MESH_SHADING_FLAT = 0, RPT_MESH_SHADING_SMOOTH = 1 };

typedef struct rpt_mesh_shading {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_SHADING_FLAT or RPT_MESH_SHADING_SMOOTH */
} rpt_mesh_shading;

int rpt_set_mesh_shading(rpt_ctx* ctx, const rpt_mesh_shading* items, uint32_t n_items);
int rpt_download_mesh_normals(rpt_ctx* ctx, uint32_t mesh, float* normals /* host, xyz per vertex */, uint32_t n_vertices);

/* ---- mesh lights — PROJECT-DEFINED ------------------------------------------------------------------------------------------------
 * Per mesh, next-event estimation samples the mesh's surface: an emissive mesh that is ON is a light like an rpt_light, picked by
 * direct_light's index draw, sampled over its area, and weighed against BSDF sampling by the power heuristic on both sides.  The
 * library computes the table the sampler reads on the device from the f32 positions the context holds, and computes it again inside
 * every call that moves a mesh; nothing crosses the host.  Every operation is stated, so that tables, samples and frames stay
 * checkable bit for bit (tests/test_gpu_mesh_light.py holds them to a numpy restatement).  dot, cross and F::MAX are those of
 * "triangle meshes"; the square roots and the divides are the library's correctly rounded ones.
 *
 * The table of an ON mesh.  Its triangles are k = 0 .. n-1 in the mesh's own order, never in slot order: rpt_rebuild_meshes leaves
 * the table bit for bit where it was.  (a, b, c) are the f32 corner positions the context holds.
 *     g = cross(b - a, c - a);  l2 = dot(g, g);  A_k = !(l2 > 0 && l2 <= F::MAX) ? 0 : 0.5f * sqrt(l2)
 *     A_max = max over k of A_k.  The mesh is DARK if A_max == 0, if it has no triangle, or if A_tot below is not finite; a dark
 *             mesh has E = 0, every C_k = 0 and A_tot = 0.  Otherwise E is the integer with A_max = f * 2^E, f in [0.5, 1).
 *     q_k   = floor(A_k * 2^(36 - E)) as a uint64 (A_k is an f32 and the scale a power of two: the product is exact in float64;
 *             q_k < 2^36)
 *     C_k   = q_0 + ... + q_k as a uint64 (below 2^62 for 2^26 triangles);  Q = C_(n-1)
 *     A_tot = f32(Q) * 2^(E - 36): the integer rounded to the nearest f32, ties to even, then an exact scaling; an overflow gives
 *             +inf, which makes the mesh dark.
 * The sums are fixed-point integers on purpose: integer addition is associative, so any parallel scan and any maximum give the
 * same bits, no summation order needs a promise, and the CDF is monotone by construction.
 *
 * Pickable lights.  N = n_lights + the number of ON meshes, and N_f = (float)N takes the place of `n_lights as F` everywhere the
 * integrator uses it: the index draw and the emission factor of every light, the rpt_lights included.  Index i < n_lights is the
 * i-th rpt_light as before; index n_lights + j is the j-th ON mesh in ascending mesh index.  Next-event estimation is skipped when
 * N == 0 (not when n_lights == 0).
 *
 * Sampling an ON mesh from scatter_pos.  The draws, in this order after the light-index draw: r0a, r0b, r1, r2 — all four are always
 * taken.  A dark mesh leaves LightSampleRec::new()'s zeros, so the facing test fails.  Otherwise
 *     J = (uint64)(r0a * 2^24) << 24 | (uint64)(r0b * 2^24)       (draws are multiples of 2^-24: exact)
 *     T = (J * Q) >> 48, the high part of the 64 x 64 product of (J << 16) and Q;  T < Q
 *     k = the first index with C_k > T, by binary search (q_k > 0 there)
 *     e1 = b - a;  e2 = c - a;  su = sqrt(r1);  bu = 1 - su;  bv = r2 * su
 *     P.i = (a.i + bu * e1.i) + bv * e2.i                           i = x, y, z
 *     direction = P - scatter_pos;  dist = length(direction);  dist_sq = dist * dist;  direction = direction / dist, per component
 *     n = normalize(cross(e1, e2));  c = dot(n, direction);  normal = (c > 0) ? -n : n
 *     emission = N_f * (the mesh material's emission);  pdf = dist_sq / (A_tot * |c|)
 * The mesh is two-sided like its emission, so the integrator's dot(direction, normal) < 0 passes from either side and fails for
 * c == 0 or NaN.  The light.area that gates the MIS weight is A_tot (> 0).  The shadow ray, disney_eval, the MIS weight and the
 * contribution are direct_light's as they stand.
 *
 * Hit side.  Where a hit's emission is added (tracer.rs:74) — `radiance += emission * throughput` — a path whose ray won a
 * triangle of an ON, not dark, mesh adds `(w * emission) * throughput` instead:
 *     w = 1 at bounce 0;  otherwise c = |dot(ray.d, n_flat)|, n_flat = normalize(cross(e1, e2)) of the winning triangle's row;
 *     !(c > 0) -> w = 1;  else lp = (hit_dist * hit_dist) / (A_tot * c) and w = power_heuristic(scatter_pdf, lp)
 * with the previous bounce's scatter_pdf and the state's hit_dist — exactly how the emitter exit weighs an rpt_light.  (Where
 * Scene::sample_lights found an rpt_light in front of that triangle, hit_dist is the light's distance, as the state holds it.)  The
 * path goes on as for any surface: a mesh light is not an emitter exit.  A SMOOTH mesh may be ON: sampling and lp use the flat
 * normal, shading the normal the mesh's mode says.  Triangle test, acceptance order, any_hit, Scene::sample_lights and the materials
 * are unchanged.
 *
 * rpt_set_mesh_lights sets the mode of the named meshes of the uploaded scene, before or after any number of moves, rebuilds or
 * shading changes; meshes not named keep theirs, and rpt_upload_scene leaves every mesh RPT_MESH_LIGHT_OFF.  On return every ON
 * mesh's table is current on every device of the context (rpt_create_multi: all of them; one process per GPU: every rank makes the
 * call itself, as for rpt_update_meshes).  A mesh without triangles may be named (it is dark).  The checks, in this order, all on
 * the host before any device is touched — a rejected call changes nothing, and rpt_last_error names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_UNSUPPORTED  the scene lacks RPT_SCENE_ANYHIT_USES_MAX_DIST: without it a mesh light's own triangles occlude every
 *                        shadow ray aimed at them; the scene's meshes hold 2^32 vertices or more;
 *   RPT_ERR_UNSUPPORTED  n_lights plus the number of ON meshes would reach 2^24 (the index draw has 24 bits).  This comes before the
 *                        items' own checks, so it counts what the well-formed items would leave ON: an item whose mesh or mode
 *                        is out of range counts as absent, a mesh named twice with its last mode;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item: mesh >= n_meshes, a mesh named twice, a mode that is
 *                        neither constant;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for rpt_update_meshes.
 * While some mesh is ON the scene renders through a kernel of its own (the mesh kernel's body with the sampler and the weight
 * above; it serves FLAT and SMOOTH meshes alike); when the last ON mesh goes OFF the context renders exactly as if the call had
 * never been made — the same kernel, the same tables.  A scene on which the call was never made is untouched by all of this.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms recompute the table of every ON mesh on the device before
 * they return RPT_OK (five more kernel launches per device, whatever the number of meshes: reset, areas and maxima, quantise and
 * scan within 256 triangles, scan of the block sums, CDF and A_tot); a rejected move leaves the tables as they were.
 *
 * rpt_download_mesh_light_table copies the table the context holds for one ON mesh to host memory from its first device: C_k for
 * all its triangles, E and A_tot.  It follows rpt_download_mesh_normals: a mesh out of range, an n_triangles that is not the
 * uploaded mesh's, a NULL destination or an OFF mesh answer RPT_ERR_INVALID_ARG (the last says so).  It never changes anything.
 *
 * Memory.  The call brings the refit's tables to every device as the context's first rpt_update_meshes does (and reads the
 * triangles' corners back from the first device once per call, like rpt_set_mesh_shading).  While a mesh is ON every device holds,
 * until the last mesh is OFF again or the next rpt_upload_scene: per ON mesh 32 B; per triangle of the ON meshes 36 B (C_k and the
 * scan's partial sum, 8 B each, A_k, 4 B, its corners, 12 B, its mesh's ordinal, 4 B) and 8 B per 256 of them; per triangle of the
 * SCENE 4 B (the hit side's lookup) and one bit.
 *
 * Timings: not measured yet — neither what the binary search and the extra tables cost a frame nor what the five launches add to a
 * move.  tools/mesh_bench.py --lights alternates, in one process, frames of scenes.mesh_scene with its torus emissive and OFF / ON,
 * and the four move calls with the mesh ON against OFF. */
enum { RPT_MESH_LIGHT_OFF = 0, RPT_MESH_LIGHT_ON = 1 };

typedef struct rpt_mesh_light {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_LIGHT_OFF or RPT_MESH_LIGHT_ON */
} rpt_mesh_light;

int rpt_set_mesh_lights(rpt_ctx* ctx, const rpt_mesh_light* items, uint32_t n_items);
int rpt_download_mesh_light_table(rpt_ctx* ctx, uint32_t mesh, uint64_t* cdf /* host, one per triangle of the mesh */,
                                  uint32_t n_triangles, int32_t* exponent, float* area);

/* ---- mesh textures — PROJECT-DEFINED ----------------------------------------------------------------------------------------------
 * Per mesh, a UV-mapped base colour: one RGBA8 image and one UV per vertex, sampled at the winning triangle and multiplied into the
 * mesh material's rgb.  Every operation is stated, so that texels, lookups and frames stay checkable bit for bit
 * (tests/test_gpu_mesh_texture.py holds them to a numpy restatement).  All arithmetic is f32, one rounding per operation, nothing
 * contracted; the divide is the library's correctly rounded one, the power is rpt_powf of include/rpt_strict_math.h.
 *
 * Scope.  A textured mesh keeps its full-patch material.  At a winning triangle of that mesh only mat.rgb changes:
 *     rgb.c = m.rgb[c] * tex.c                                       c = r, g, b; one product each
 * A texture never touches emission (an emission map does: "mesh emission maps" below).  hit_emission, the sampler of mesh lights and
 * its hit weight, the triangle test, the acceptance order, any_hit and the normals are unchanged.  One texture per mesh, one UV per vertex: a UV seam needs duplicated vertices, as
 * any OBJ loader produces them.
 *
 * Decode, once per rpt_set_mesh_textures, on the device.  The input is RGBA8, alpha ignored, width * height * 4 bytes, row 0 first.
 * The linear value L[k] of byte value k:
 *     gamma == 1.0f:  L[k] = (float)k / 255.0f
 *     otherwise:      L[0] = 0;  L[255] = 1;  L[k] = rpt_powf((float)k / 255.0f, gamma) for every other k
 * The end points are by definition: nothing rests on pow(1, g).  A decoded texel is {L[R], L[G], L[B], 0}, four f32, 16 B: a filter
 * tap is one gather.
 *
 * Lookup at the hit.  u and v are recomputed from the ray and the winning triangle's row exactly as "smooth mesh shading" does — the
 * same operations, the same bits.  (sa, ta), (sb, tb), (sc, tc) are the UVs of the corners a, b, c.
 *     w = (1 - u) - v
 *     s = (w*sa + u*sb) + v*sc
 *     t = (w*ta + u*tb) + v*tc
 * Per axis — x from s with W = width, y from t with H = height — and W_f = (float)W:
 *     REPEAT:   x = s - floorf(s)              (in [0, 1]; 1.0 is reached by rounding for a tiny negative s, and is legal)
 *     CLAMP:    x = s < 0 ? 0 : (s > 1 ? 1 : s)
 *     NEAREST:  i = (int32)floorf(x * W_f);    REPEAT: i == W -> 0;    CLAMP: i = min(i, W - 1)
 *     BILINEAR: p = x * W_f - 0.5f  (two operations);  f0 = floorf(p);  fx = p - f0;  i0 = (int32)f0;  i1 = i0 + 1
 *               REPEAT: i0 < 0 -> i0 + W;  i1 >= W -> i1 - W;          CLAMP: i0 = max(i0, 0);  i1 = min(i1, W - 1)
 * Texel (i, j) is entry j * W + i; row j = 0 is t = 0: there is no flip.
 *     NEAREST:  tex = texel(i, j)
 *     BILINEAR: gx = 1 - fx;  gy = 1 - fy;  top = gx*c00 + fx*c10;  bot = gx*c01 + fx*c11;  tex = gy*top + fy*bot
 * with c00 = texel(i0, j0), c10 = texel(i1, j0), c01 = texel(i0, j1), c11 = texel(i1, j1); every a*b + c*d is two products and one
 * add, per component.  The statement is written once, in csrc/host_tex.h, which the kernels and the host reference both compile.
 *
 * rpt_set_mesh_textures sets or removes the texture of the named meshes of the uploaded scene, before or after any number of moves,
 * rebuilds, shading or light changes; meshes not named keep theirs, and rpt_upload_scene leaves every mesh untextured and drops
 * every texture table.  An item with width == height == 0 and texels == NULL removes its mesh's texture (its uvs are not read).
 * Both arrays of an item are copied inside the call.  On return every texture is decoded on every device of the context
 * (rpt_create_multi: all of them; one process per GPU: every rank makes the call itself, as for rpt_set_mesh_lights).  The checks,
 * in this order, all on the host before any device is touched — a rejected call changes nothing, and rpt_last_error names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_UNSUPPORTED  the scene's meshes hold 2^32 vertices or more;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item, in order: mesh >= n_meshes; a mesh named twice; and when
 *                        setting: n_vertices differs from the mesh's; uvs NULL with a non-zero count; width or height 0 or above
 *                        16384; texels NULL; wrap or filter neither constant; gamma not finite, <= 0 or > 16; a UV that is not
 *                        finite or beyond 2^20 in magnitude (the message names the mesh and the vertex; the bound keeps floorf and
 *                        the casts exact);
 *   RPT_ERR_UNSUPPORTED  the scene's textures would hold more than 2^26 texels in all;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for rpt_update_meshes.
 * While some mesh is textured the scene renders through a kernel of its own — the mesh kernel's body with the lookup above, one
 * form over the smooth scenes' tables (FLAT meshes through all-zero smooth bits) and one over the mesh lights' while some mesh is ON:
 * textures compose with FLAT / SMOOTH and OFF / ON in every combination.  When the last texture is removed the context renders
 * exactly as if the call had never been made — the same kernel, the same tables.  A scene on which the call was never made is
 * untouched by all of this.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms leave UVs and texels alone: no new launch inside a move.
 * rpt_rebuild_meshes reorders slots and changes no textured frame: the lookup goes through the refit's slot -> vertex table and the
 * flattened triangle index, never through slot order.
 *
 * rpt_download_mesh_texture copies the decoded texels the context holds for one textured mesh to host memory from its first device:
 * width * height * 4 f32, row 0 first.  It follows rpt_download_mesh_normals: a mesh out of range, an untextured mesh (it says so), a
 * size that is not the texture's or a NULL destination answer RPT_ERR_INVALID_ARG.  It never changes anything.
 *
 * Memory.  The call brings the refit's tables to every device as rpt_set_mesh_shading does.  While a mesh is textured every device
 * holds, until the last texture is removed or the next rpt_upload_scene: 16 B per texel; 32 B per textured mesh; per triangle of the
 * SCENE 4 B (which texture) and one bit; per vertex of the SCENE 8 B (its UV).  During a call, per device, the new tables beside the
 * old ones, and 4 B per texel plus 1 KiB per image being set.  The host keeps 8 B per vertex of the scene.
 *
 * Timings (one MI355X, tools/mesh_bench.py --textures: scenes.mesh_scene, 393 216 triangles, 1920 x 1080 x 16 spp resident, untextured
 * against a 1024 x 1024 BILINEAR / REPEAT texture on both meshes, alternating in one process, medians of 5): 0.824 Gsamples/s
 * untextured, 0.797 textured (0.967); the textured kernels have the mesh kernel's VGPR count, so its occupancy.  The set call for both
 * images (2 x 2^20 texels): 2.49 ms the first time, 1.09 ms again.  The four move calls take the same time textured and untextured
 * (within 0.01 ms). */
enum { RPT_TEX_WRAP_REPEAT = 0, RPT_TEX_WRAP_CLAMP = 1 };
enum { RPT_TEX_FILTER_NEAREST = 0, RPT_TEX_FILTER_BILINEAR = 1 };

typedef struct rpt_mesh_texture {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t n_vertices;              /* of `uvs`: the uploaded mesh's n_vertices */
    const float* uvs;                 /* HOST, 2 floats per vertex, all of the mesh's vertices */
    uint32_t width, height;
    const uint8_t* texels;            /* HOST, RGBA8; width == height == 0 and texels == NULL: remove this mesh's texture */
    uint32_t wrap, filter;            /* RPT_TEX_WRAP_*, RPT_TEX_FILTER_* */
    float gamma;                      /* 1.0f: the bytes are linear; 2.2f: the usual decode of an sRGB-like image */
} rpt_mesh_texture;

int rpt_set_mesh_textures(rpt_ctx* ctx, const rpt_mesh_texture* items, uint32_t n_items);
int rpt_download_mesh_texture(rpt_ctx* ctx, uint32_t mesh, float* texels /* host, width*height*4 f32, decoded */, uint32_t width,
                              uint32_t height);

/* ---- environment lighting — PROJECT-DEFINED ----------------------------------------------------------------------------------------
 * One image-based sky for the uploaded MESH scene: a square f32 RGB image in an OCTAHEDRAL layout replaces rpt_background at a miss
 * and, with RPT_ENV_SAMPLED, is one more pickable light of direct_light, importance-sampled by texel and weighed against BSDF
 * sampling by the power heuristic at the miss, so nothing is counted twice.  Every operation is stated, so that tables, lookups,
 * samples and frames stay checkable bit for bit (tests/test_gpu_mesh_env.py holds them to a numpy restatement).  All arithmetic is
 * f32, one rounding per operation, nothing contracted; the divide and the root are the library's correctly rounded ones; dot and
 * F::MAX are those of "triangle meshes".  The layout needs no atan2 or acos: direction to texel and back is fabs, compares,
 * products, divides and one root.  The statement is written once, in csrc/host_env.h, which the kernels and the host reference
 * both compile.
 *
 * Lookup of a direction d.  S = size, S_f = (float)S, sgn(x) = x >= 0 ? 1 : -1 (so sgn(-0) = 1).
 *     l1 = (|d.x| + |d.y|) + |d.z|;   !(l1 > 0 && l1 <= F::MAX)  ->  radiance (0,0,0), k = none     (also a NaN d)
 *     px = d.x / l1;  pz = d.z / l1
 *     d.y < 0:  (px, pz) = ((1 - |pz|) * sgn(px), (1 - |px|) * sgn(pz))       both from the OLD px, pz   (d.y = -0 does not fold)
 *     s = px * 0.5f + 0.5f;  t = pz * 0.5f + 0.5f                              (two operations each; in [0, 1])
 *     i = min((int32)floorf(s * S_f), S - 1);  j likewise from t;  k = j * S + i
 *     radiance.c = texel_k.c * scale                                           one product per channel
 * The lookup is NEAREST only, so the sampler's density is exactly proportional to what the lookup returns.  +y is the centre of the
 * image, -y its four corners: the lower hemisphere folds into them.  +x is the middle of the right edge (i = S - 1), +z the middle of
 * the last row.
 *
 * Table (RPT_ENV_SAMPLED only): the "mesh lights" table with texels for triangles.
 *     w_k = (r + g) + b;   W_max = max over k of w_k;   the table is DARK if W_max == 0
 *     E: the integer with W_max = f * 2^E, f in [0.5, 1)   (a subnormal W_max included)
 *     q_k = floor(w_k * 2^(36 - E)) as a uint64;   C_k = q_0 + ... + q_k;   Q = C_(S*S-1)  (below 2^60 at 4096 x 4096)
 * It is computed on the device, in integers: no summation order needs a promise.
 *
 * Sampling from scatter_pos.  The draws come after the light-index draw and are r0a, r0b, r1, r2; all four are always taken.  A dark
 * table leaves LightSampleRec::new()'s zeros.  J, T and the binary search for k are exactly as "mesh lights" states them.  Then
 *     i = k % S;  j = k / S
 *     s = ((float)i + r1) / S_f;  t = ((float)j + r2) / S_f
 *     px = s * 2 - 1;  pz = t * 2 - 1;  py = (1 - |px|) - |pz|
 *     py < 0:  (px, pz) = ((1 - |pz|) * sgn(px), (1 - |px|) * sgn(pz))        old values; py stays as it is
 *     l2 = dot(p, p);  len = sqrt(l2);  direction = p / len  (per component)
 *     sel = (float)q_k / (float)Q                                  each integer rounded to nearest f32, ties to even; one divide
 *     pdf = (sel * ((S_f * S_f) * 0.25f)) * (l2 * len)
 *     dist = +inf (as RPT_LIGHT_DISTANT);  normal = -direction;  emission = N_f * (texel_k * scale);  light.area = 1 (the MIS weight
 *     of direct_light applies)
 * l2 * len = |p|^3 is the octahedral map's Jacobian: d omega = dp_x dp_z / |p|^3 on the square of area 4.  The emission is that of
 * the PICKED texel k, not a second lookup of the rounded direction (which, within an ulp of a texel border, may be a neighbour).
 * scatter_pos does not enter: the light is at infinity.
 *
 * Pickable lights.  N = n_lights + ON meshes + (1 if an environment is set and SAMPLED); the environment takes the LAST index, and
 * N_f replaces `n_lights as F` everywhere, as "mesh lights" arranges.  A BACKGROUND_ONLY environment does not count in N.
 *
 * Miss side.  Where the path adds background * throughput it adds (w * radiance(d)) * throughput, in this order: the lookup of
 * ray.d gives k, p = (px, d.y / l1, pz) BEFORE the fold, and the texel {r, g, b, (float)q_k} by one 16 B gather; radiance as above;
 *     w = 1   at bounce 0; for BACKGROUND_ONLY; for a dark table; when k = none; when q_k == 0;
 *     else lp = pdf above for this k and this p  (the same function the sampler calls: csrc/host_env.h, env_pdf);  lp == 0: w = 1;
 *     else w = power_heuristic(scatter_pdf, lp)
 * then w * radiance per channel, then the product with the throughput.
 *
 * Stated costs.  The weights carry no solid-angle factor: per solid angle, texels near the octahedron's corners (the six axis
 * directions, |p|^3 = 1) are sampled up to about 5 times denser than those at its face centres (|p|^3 = 3^-1.5), where an ideal
 * sampler of a uniform sky would treat both alike — unbiased, since the pdf says so.  A texel
 * more than 2^36 below the brightest has q_k == 0 and is never picked by next-event estimation; BSDF sampling still finds it at
 * full weight.
 *
 * rpt_set_environment sets (env != NULL) or removes (env == NULL) the environment of the uploaded scene, before or after any number
 * of moves, shading, light or texture changes.  The image is copied inside the call; on return the tables are current on every
 * device of the context.  The checks, in this order, all on the host before any device is touched — a rejected call changes nothing,
 * and rpt_last_error names the fault:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_INVALID_ARG  size is 0 or above 4096; texels is NULL; mode is neither constant; scale is not finite or is negative; a
 *                        texel component is not finite, is negative or is above 2^100 (the message names the texel);
 *   RPT_ERR_UNSUPPORTED  SAMPLED would bring N to 2^24 (rpt_set_mesh_lights counts a SAMPLED environment in its own rule);
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for the other mesh calls.
 * Removing the environment leaves the context rendering exactly as if the call had never been made — the same kernel, the same
 * tables.  rpt_upload_scene drops the environment.  While an environment is set the scene renders through ONE kernel of its own,
 * the mesh kernel's body over the textured mesh-light form; a feature the scene does not use goes through empty tables, so the
 * environment composes with FLAT / SMOOTH, OFF / ON and textures in every combination.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms do not touch the environment: no launch is added to a move.
 *
 * rpt_download_environment_table copies C_k (size * size uint64) and E from the context's first device.  RPT_ERR_INVALID_ARG: no
 * SAMPLED environment is set (it says so), n_texels is not size * size, or a NULL destination.  A dark table is all zeros, E = 0.
 *
 * Memory.  The call brings the refit's tables to every device as rpt_set_mesh_shading does.  While an environment is set every
 * device holds 16 B per texel, SAMPLED 8 B more and 8 B per 256 texels, and per triangle of the SCENE 4 B and one bit (the empty
 * tables); during the call 12 B per texel more.
 *
 * Timings: not measured yet.  tools/mesh_bench.py --environment alternates, in one process, frames of scenes.mesh_scene without an
 * environment, with a BACKGROUND_ONLY one and with a SAMPLED one (1024 x 1024), and times the set call. */
enum { RPT_ENV_BACKGROUND_ONLY = 0, RPT_ENV_SAMPLED = 1 };

typedef struct rpt_environment {
    uint32_t size;                    /* the image is size x size texels, 1 .. 4096 */
    const float* texels;              /* HOST, linear RGB, size*size*3 f32, row 0 first; copied inside the call */
    float scale;                      /* finite, >= 0 */
    uint32_t mode;                    /* RPT_ENV_BACKGROUND_ONLY or RPT_ENV_SAMPLED */
} rpt_environment;

int rpt_set_environment(rpt_ctx* ctx, const rpt_environment* env /* NULL: remove */);
int rpt_download_environment_table(rpt_ctx* ctx, uint64_t* cdf /* host, size*size */, uint32_t n_texels, int32_t* exponent);

/* ---- mesh cutouts — PROJECT-DEFINED ------------------------------------------------------------------------------------------------
 * Per mesh, geometry cut out by a mask: one A8 image, looked up through the mesh's texture UVs INSIDE the triangle test, so that a
 * ray through a hole goes on to whatever lies behind it and a shadow ray through a hole is not occluded: leaves, fences, grilles,
 * decals.  Every operation is stated, so that masks, walks and frames stay checkable bit for bit (tests/test_gpu_mesh_cutout.py holds
 * them to a numpy restatement).  The mask is given on its own, as A8: the library does not keep a texture's bytes, rpt_mesh_texture
 * and the decoded texels (rpt_download_mesh_texture) are what they were.  The statement is written once, in csrc/host_cut.h, which
 * the kernels and the host reference both compile.
 *
 * Mask bits.  Bit k = j * width + i of a mesh's mask is
 *     alpha[k] >= threshold                                          an integer compare; 1: the texel is OPAQUE
 * stored as bit k % 32 of word k / 32.  Each mask starts at a 16 B boundary (it is padded with zero bits to a multiple of 128
 * texels).  The bits are made on the device, one lane per texel and one ballot per wave; nothing in them depends on the launch.
 *
 * Cut test.  The triangle test of "triangle meshes" gains one last line, after the point check, for a triangle whose mesh has a
 * cutout ON.  It uses that test's own u and v — the same operations on the same words — and tex_interp, tex_wrap and the NEAREST
 * index of "mesh textures" (csrc/host_tex.h), reused and not restated.  The mesh's TEXTURE supplies the UVs (sa, ta), (sb, tb),
 * (sc, tc) of the corners a, b, c and the wrap; W and H are the MASK's width and height, which need not be the texture's:
 *     w = (1 - u) - v
 *     s = (w*sa + u*sb) + v*sc;   t = (w*ta + u*tb) + v*tc
 *     x = wrap(s);  y = wrap(t)                                      REPEAT or CLAMP, as "mesh textures" states them
 *     i = nearest(x, W);  j = nearest(y, H)                          i = (int32)floorf(x * W_f); REPEAT: i == W -> 0; CLAMP: min(i, W - 1)
 *     !bit(j * W + i)  ->  miss
 * The mask is always looked up NEAREST, whatever the colour filter.  Stated cost: with a BILINEAR colour texture, a texel next to a
 * hole bleeds the hole's RGB into the opaque side; paint the holes' RGB like their neighbours'.
 *
 * closest_hit and any_hit are unchanged in wording: they use "the triangle test".  The library applies the cut test only to a
 * candidate that would otherwise be accepted — in the closest walk after t < best (or the tie rule), in the any-hit walk after
 * t < max_dist: rejecting a candidate that would not have been accepted changes nothing, and it is what keeps rejected candidates
 * from paying for the lookup.  The hierarchy returns the ordered loop's answer as before: the test is a function of
 * (ray, triangle) alone, and rejecting more candidates never moves a hit outside its triangle's box.
 *
 * Composition.  Cutouts compose with FLAT / SMOOTH, textures of any wrap and filter, and an environment in either mode.  A path
 * that hits an emissive cutout mesh sees its emission only where the mesh is opaque.  A cutout mesh cannot be a mesh light (next-
 * event estimation would sample points inside holes): rpt_set_mesh_cutouts answers RPT_ERR_UNSUPPORTED for a mesh that is ON, and
 * rpt_set_mesh_lights answers the same for turning ON a mesh with a cutout.  A cutout needs the mesh's UVs: an untextured mesh is
 * RPT_ERR_INVALID_ARG (a 1 x 1 white texture is enough).  rpt_set_mesh_textures that would remove the texture of a mesh whose cutout
 * is ON is RPT_ERR_INVALID_ARG ("remove the cutout first"); replacing the texture keeps the cutout, which then reads the new UVs and
 * wrap.  rpt_upload_scene drops all cutouts.
 *
 * rpt_set_mesh_cutouts sets (ON) or removes (OFF) the cutout of the named meshes of the uploaded scene; meshes not named keep
 * theirs.  `alpha` is copied inside the call; on return every mask is current on every device of the context.  The checks, in this
 * order, all on the host before any device is touched — a rejected call changes nothing, and rpt_last_error starts with
 * "rpt_set_mesh_cutouts: " and names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item, in order: mesh >= n_meshes, or a mesh named twice; mode
 *                        neither constant; ON with width or height 0 or above 16384; ON with alpha NULL; ON with threshold outside
 *                        1 .. 255; OFF with a non-zero size or a non-NULL alpha; ON on an untextured mesh;
 *   RPT_ERR_UNSUPPORTED  ON on a mesh light;
 *   RPT_ERR_UNSUPPORTED  all masks together would hold more than 2^26 texels;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for the other mesh calls.
 * While some cutout is ON the scene renders through a kernel of its own — the mesh kernel's body with the two walks above, one form
 * over the textured mesh-light tables (absent lights through empty tables, as the environment form does it) and one over the
 * environment form.  Turning every cutout OFF leaves the context rendering through exactly the kernels and tables it had before
 * the first call.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms leave masks alone and add no launch: the cut test goes
 * through the refit's slot -> vertex table and the flattened triangle index, never through slot order.
 *
 * rpt_download_mesh_cutout copies one mesh's mask bits from the context's first device: n_words = ceil(width * height / 32) words.
 * A mesh out of range, a mesh without a cutout (it says so), another n_words or a NULL destination answer RPT_ERR_INVALID_ARG.
 *
 * Memory.  While a cutout is ON every device holds one bit per mask texel (each mask padded to 128 texels), 16 B per mesh of the
 * scene (the descriptors are indexed by texture ordinal; the table is sized for every mesh being textured), and 4 B per triangle of
 * the SCENE (the empty light table); during the call, per device, the new tables beside the old ones and one byte per texel of the
 * masks being set.  Per candidate of a cutout mesh that passes the distance compare the walk gathers 4 B (which texture), the 16 B
 * descriptor, three slot -> vertex words, three UVs and one mask word; a candidate of another mesh the first 4 B only.
 *
 * Timings: not measured yet.  tools/mesh_bench.py --cutouts alternates, in one process, frames of scenes.mesh_scene textured as
 * --textures does with no mask, under a 1024 x 1024 checker mask on both meshes (rays pass through holes: faster or slower, both are
 * legitimate) and under an all-opaque mask (the pure cost of the test), and times the set call and the four move calls.  Registers:
 * meshcut_regen_kernel 110 VGPRs and meshcut_env_regen_kernel 112, next to meshtex_light_regen_kernel's 111 and
 * meshenv_regen_kernel's 113; neither uses scratch. */
enum { RPT_MESH_CUTOUT_OFF = 0, RPT_MESH_CUTOUT_ON = 1 };

typedef struct rpt_mesh_cutout {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_CUTOUT_* ; OFF: width == height == 0, alpha == NULL */
    uint32_t width, height;           /* of the mask: its own size, need not be the texture's */
    const uint8_t* alpha;             /* HOST, one byte per texel, row 0 first; copied inside the call */
    uint32_t threshold;               /* 1 .. 255: a texel is OPAQUE when alpha >= threshold */
} rpt_mesh_cutout;

int rpt_set_mesh_cutouts(rpt_ctx* ctx, const rpt_mesh_cutout* items, uint32_t n_items);
int rpt_download_mesh_cutout(rpt_ctx* ctx, uint32_t mesh, uint32_t* bits /* host */, uint32_t n_words);

/* ---- mesh normal maps — PROJECT-DEFINED ------------------------------------------------------------------------------------------
 * Per mesh, surface detail without triangles: one RGBA8 tangent-space normal map, looked up through the mesh's texture UVs at the
 * winning triangle, bends the SHADING normal — the flat one, or "smooth mesh shading"'s.  Every operation is stated, so that texels,
 * hit normals and frames stay checkable bit for bit (tests/test_gpu_mesh_normal_map.py holds them to a numpy restatement).  The
 * statement is written once, in csrc/host_nrm.h, which the kernels and the host harness both compile; it reuses tex_interp,
 * tex_wrap and tex_lookup of "mesh textures" (csrc/host_tex.h) and does not restate them.  All arithmetic is f32, one rounding per
 * operation, nothing contracted, with the library's correctly rounded divide and root; dot, cross and F::MAX are those of
 * "triangle meshes".
 *
 * Decode.  Once per call, on the device, one lane per texel.  For a byte k
 *     c(k) = max(((float)k - 128) / 127, -1)                         c(128) = 0, c(255) = 1, c(0) = c(1) = -1, all exactly
 * and a decoded texel is four f32, 16 B:
 *     {sx * c(R), sy * c(G), c(B), 0}                                sx = strength; sy = strength, or -strength with FLIP_GREEN
 * z is neither scaled nor clamped; alpha is ignored.
 *
 * Lookup at the hit.  The triangle test's own u and v are recomputed as "mesh textures" does it — the same operations on the same
 * words.  (s, t) = tex_interp over the UVs of the mesh's TEXTURE; that texture's wrap applies, the MAP's own filter, and W and H
 * are the map's, which need not be the texture's.  tex_lookup over the decoded texels gives (x, y, z).
 *
 * Bend.  N is the normal the hit would have had without the map; e1, e2 are the triangle row's; (sa, ta), (sb, tb), (sc, tc) the
 * corners' UVs.
 *     x == 0 && y == 0                                      -> N     a flat map is the identity, bit for bit
 *     du1 = sb - sa;  dv1 = tb - ta;  du2 = sc - sa;  dv2 = tc - ta
 *     D = du1*dv2 - du2*dv1                                          two products, one subtraction
 *     !(D < 0 || D > 0)                                     -> N     degenerate UVs, NaN
 *     g = D > 0 ? 1 : -1
 *     T0.i = g * (e1.i*dv2 - e2.i*dv1);  B0.i = g * (e2.i*du1 - e1.i*du2)                    i = x, y, z
 *     k = dot(N, T0);  T1.i = T0.i - N.i*k;  l2 = dot(T1, T1)
 *     !(l2 > 0 && l2 <= F::MAX)                             -> N
 *     T = T1 / sqrt(l2)                                              one root, three divides
 *     B = cross(N, T);  dot(B, B0) < 0 -> B = -B                     mirrored UVs; B is not normalised again
 *     m.i = (x*T.i + y*B.i) + z*N.i;  l2 = dot(m, m)
 *     !(l2 > 0 && l2 <= F::MAX)                             -> N
 *     result m / sqrt(l2)                                            one root, three divides
 * The tangent is per TRIANGLE, from positions and UVs at the hit: there is no per-vertex tangent table, so no move adds a launch
 * and a rebuild changes nothing.  Stated cost: across a coarse SMOOTH mesh the tangent turns facet by facet.  Stated cost of the
 * result: like the smooth normal it is not turned toward the ray and not bent back; near grazing view it can face away from the
 * ray, and the hit is then shaded from the other side.  Unchanged: the triangle test, acceptance, any_hit, materials, emission, the
 * mesh-light sampler and hit weight (which use the flat normal), cutouts and the environment.
 *
 * Composition.  Normal maps compose with FLAT / SMOOTH, OFF / ON lights, textures of any wrap and filter, cutouts, and an
 * environment in either mode.  A normal map needs the mesh's UVs: an untextured mesh is RPT_ERR_INVALID_ARG (a 1 x 1 white texture
 * is enough).  rpt_set_mesh_textures that would remove the texture of a mesh whose map is ON is RPT_ERR_INVALID_ARG ("remove the
 * normal map first"); replacing the texture keeps the map, which then reads the new UVs and wrap.  rpt_upload_scene drops all maps.
 *
 * rpt_set_mesh_normal_maps sets (ON) or removes (OFF) the map of the named meshes of the uploaded scene; meshes not named keep
 * theirs.  `texels` is copied inside the call; on return every map is current on every device of the context.  The checks, in this
 * order, all on the host before any device is touched — a rejected call changes nothing, and rpt_last_error starts with
 * "rpt_set_mesh_normal_maps: " and names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item, in order: mesh >= n_meshes, or a mesh named twice; mode
 *                        neither constant; ON with width or height 0 or above 16384; ON with texels NULL; filter not a constant; an
 *                        unknown flag bit; strength not finite, negative or above 16; OFF with a non-zero size or a non-NULL
 *                        texels; ON on an untextured mesh;
 *   RPT_ERR_UNSUPPORTED  all maps together would hold more than 2^26 texels;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for the other mesh calls.
 * While some map is ON the scene renders through a kernel of its own — the mesh kernel's body with the hit normal above, one form
 * each over the textured mesh-light tables (absent lights through empty tables), the environment form and the two cutout forms,
 * picked by (cutouts, environment).  Turning every map OFF leaves the context rendering through exactly the kernels and tables it
 * had before the first call.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms leave maps alone and add no launch: the bend reads the
 * triangle row the walk tested, the refit's slot -> vertex table and the flattened triangle index, never slot order.
 *
 * rpt_download_mesh_normal_map copies one mesh's DECODED texels from the context's first device: width * height * 4 f32.  A mesh
 * out of range, a mesh without a map (it says so), another size or a NULL destination answer RPT_ERR_INVALID_ARG.
 *
 * Memory.  While a map is ON every device holds 16 B per map texel, 16 B per mesh of the scene (the descriptors are indexed by
 * texture ordinal; the table is sized for every mesh being textured), and 4 B per triangle of the SCENE (the empty light table);
 * during the call, per device, the new tables beside the old ones and 4 B per texel of the maps being set.  Per hit on a mapped mesh
 * the kernel gathers 4 B (which texture), the 16 B descriptor, three slot -> vertex words, three UVs and one (NEAREST) or four
 * (BILINEAR) 16 B texels; a hit on another mesh the first 4 B, or with it the descriptor.
 *
 * Timings (MI355X, 1080p x 16 spp, medians of 5): 0.794 Gsamples/s with no map, 0.784 under a flat map (0.989) and 0.416 under a
 * bump map (0.524); rpt_set_mesh_normal_maps for both 1024 x 1024 maps 0.7 ms the first time and 0.7 ms again; the four move calls
 * without / with maps: update_meshes 0.45 / 0.44 ms; rebuild_meshes 1.19 / 1.18 ms; update_meshes_device 0.16 / 0.16 ms;
 * rebuild_meshes_device 0.75 / 0.75 ms.  tools/mesh_bench.py --normal-maps alternates, in one process, frames of scenes.mesh_scene textured as
 * --textures does with no map, under a flat 1024 x 1024 map on both meshes (the pure cost of the lookup: the bend returns at its
 * first line) and under a 1024 x 1024 BILINEAR bump map, and times the set call and the four move calls with and without maps. */
enum { RPT_MESH_NORMAL_MAP_OFF = 0, RPT_MESH_NORMAL_MAP_ON = 1 };
enum { RPT_NORMAL_MAP_FLIP_GREEN = 1u << 0 };      /* a map authored with +y down (the "DirectX" convention) */

typedef struct rpt_mesh_normal_map {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_NORMAL_MAP_* ; OFF: width == height == 0, texels == NULL */
    uint32_t width, height;           /* of the map: its own size, need not be the texture's */
    const uint8_t* texels;            /* HOST, RGBA8 like rpt_mesh_texture (alpha ignored), row 0 first; copied inside the call */
    uint32_t filter;                  /* RPT_TEX_FILTER_NEAREST / RPT_TEX_FILTER_BILINEAR */
    uint32_t flags;                   /* RPT_NORMAL_MAP_FLIP_GREEN or 0 */
    float strength;                   /* finite, 0 .. 16: scales x and y */
} rpt_mesh_normal_map;

int rpt_set_mesh_normal_maps(rpt_ctx* ctx, const rpt_mesh_normal_map* items, uint32_t n_items);
int rpt_download_mesh_normal_map(rpt_ctx* ctx, uint32_t mesh, float* texels /* host, width*height*4 f32, decoded */, uint32_t width, uint32_t height);

/* ---- mesh material maps — PROJECT-DEFINED ----------------------------------------------------------------------------------------
 * Per mesh, a material that varies across the surface: one RGBA8 map, looked up through the mesh's texture UVs at the winning
 * triangle, scales the mesh material's ROUGHNESS and METALLIC.  Every operation is stated, so that texels, hit materials and frames
 * stay checkable bit for bit (tests/test_gpu_mesh_material_map.py holds them to a numpy restatement).  The statement is written
 * once, in csrc/host_mmap.h, which the kernels and the host harness both compile; it reuses tex_interp, tex_wrap and tex_lookup of
 * "mesh textures" (csrc/host_tex.h) and does not restate them.  All arithmetic is f32, one rounding per operation, nothing
 * contracted, with the library's correctly rounded divide.
 *
 * Decode.  Once per call, on the device, one lane per texel.  For a byte k
 *     c(k) = (float)k / 255                                          c(0) = 0, c(255) = 1, both exactly
 * and a decoded texel is four f32, 16 B, so that tex_lookup serves it unchanged:
 *     {fr, fm, 0, 0}          fr = c(byte of roughness_channel), or exactly 1 for RPT_MATERIAL_MAP_CHANNEL_NONE; fm likewise for
 *                             metallic_channel
 * The channel choice is resolved here: the render kernels never see it.
 *
 * Lookup at the hit.  The triangle test's own u and v are recomputed as "mesh textures" does it — the same operations on the same
 * words.  (s, t) = tex_interp over the UVs of the mesh's TEXTURE; that texture's wrap applies, the MAP's own filter, and W and H
 * are the map's, which need not be the texture's.  tex_lookup over the decoded texels gives (fr, fm, .).
 * There is no clamp: BILINEAR cannot leave [0, 1].  A weight f below 1/2 comes from p = x*n - 1/2 with x*n >= 1/2, so it is a
 * multiple of 2^-24 and g = 1 - f is exact (as it is for f >= 1/2); with a, b in [0, 1], rn(g*a) + rn(f*b) <= g + f = 1 and rounding
 * is monotone; the second blend repeats the argument.  For the same reason an all-255 map looks up exactly 1 (and an all-0 map
 * exactly 0) under either filter; any other constant image is returned exactly by NEAREST only — BILINEAR rounds g*c and f*c
 * separately (tests/test_mesh_material_map_host.py counts both over all byte pairs and 65 weights).
 *
 * Apply.  After the base's hit_material — after "mesh textures" has written rgb:
 *     mat.roughness = mat.roughness * fr;  mat.metallic = mat.metallic * fm                   one multiplication each
 * Everything derived from them follows as for any material: the max(roughness, 0.01), ax, ay, the lobe weights.  Unchanged:
 * emission, rgb, the triangle test, acceptance, any_hit, normals, the mesh-light sampler and hit weight, cutouts, the environment.
 *
 * Composition.  Material maps compose with FLAT / SMOOTH, OFF / ON lights (which emit as before), textures of any wrap and filter,
 * cutouts, normal maps, and an environment in either mode.  A material map needs the mesh's UVs: an untextured mesh is
 * RPT_ERR_INVALID_ARG (a 1 x 1 white texture is enough).  rpt_set_mesh_textures that would remove the texture of a mesh whose map is
 * ON is RPT_ERR_INVALID_ARG ("remove the material map first"); replacing the texture keeps the map, which then reads the new UVs and
 * wrap.  rpt_upload_scene drops all maps.
 *
 * rpt_set_mesh_material_maps sets (ON) or removes (OFF) the map of the named meshes of the uploaded scene; meshes not named keep
 * theirs.  `texels` is copied inside the call; on return every map is current on every device of the context (one process per GPU:
 * every rank makes the call).  The checks, in this order, all on the host before any device is touched — a rejected call changes
 * nothing, and rpt_last_error starts with "rpt_set_mesh_material_maps: " and names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item, in order: mesh >= n_meshes, or a mesh named twice; mode
 *                        neither constant; ON with width or height 0 or above 16384; ON with texels NULL; filter not a constant; a
 *                        channel neither 0 .. 3 nor NONE; ON with both channels NONE; OFF with a non-zero size or a non-NULL
 *                        texels; ON on an untextured mesh;
 *   RPT_ERR_UNSUPPORTED  all maps together would hold more than 2^26 texels;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for the other mesh calls.
 * While some map is ON the scene renders through a kernel of its own — the mesh kernel's body with the hit material above, one
 * form over each of the eight textured forms that hold every table: the textured mesh-light one (absent lights through empty
 * tables; a scene that would take the plain textured form takes this one), the environment form, the two cutout forms and the four
 * normal-mapped forms, picked by (normal maps, cutouts, environment).  Turning every map OFF leaves the context rendering through
 * exactly the kernels and tables it had before the first call.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms leave maps alone and add no launch: the lookup reads the
 * triangle row the walk tested, the refit's slot -> vertex table and the flattened triangle index, never slot order.
 *
 * rpt_download_mesh_material_map copies one mesh's DECODED texels from the context's first device: width * height * 4 f32.  A mesh
 * out of range, a mesh without a map (it says so), another size or a NULL destination answer RPT_ERR_INVALID_ARG.
 *
 * Memory.  While a map is ON every device holds 16 B per map texel, 16 B per mesh of the scene (the descriptors are indexed by
 * texture ordinal; the table is sized for every mesh being textured), and 4 B per triangle of the SCENE (the empty light table);
 * during the call, per device, the new tables beside the old ones and 4 B per texel of the maps being set.  Per hit on a mapped mesh
 * the kernel gathers 4 B (which texture), the 16 B descriptor, three slot -> vertex words, three UVs and one (NEAREST) or four
 * (BILINEAR) 16 B texels; a hit on another mesh the first 4 B, or with it the descriptor.
 *
 * Registers (gfx950, VGPRs / spilled SGPRs, base form in brackets, no scratch in any form; tools/kernel_meta.py): meshmap 111 / 156
 * (111 / 152), meshmap_env 113 / 154 (113 / 148), meshmap_cut 110 / 188 (110 / 179), meshmap_cut_env 112 / 191 (112 / 187),
 * meshmap_nrm 111 / 150 (111 / 156), meshmap_nrm_env 113 / 150 (113 / 146), meshmap_nrm_cut 111 / 193 (110 / 189),
 * meshmap_nrm_cut_env 112 / 185 (112 / 191): the lookup recomputes u, v and the UV interpolation and still fits its base's budget.
 *
 * Timings (MI355X, 1080p x 16 spp, medians of 5): 0.794 Gsamples/s with no map, 0.786 under an all-255 map (0.991) and 0.764
 * under a noise map (0.963); rpt_set_mesh_material_maps for both 1024 x 1024 maps 1.9 ms the first time in a process and 0.6 ms again;
 * the four move calls without / with maps: update_meshes 0.42 / 0.44 ms; rebuild_meshes 1.02 / 1.02 ms; update_meshes_device 0.16 /
 * 0.16 ms; rebuild_meshes_device 0.75 / 0.74 ms.  The no-map rate is that of the textured kernel, unchanged (mesh normal maps: 0.794).
 * tools/mesh_bench.py --material-maps alternates, in one process, frames of scenes.mesh_scene textured as --textures does with no
 * map, under an all-255 1024 x 1024 map on both meshes (the pure cost of the lookup: both factors are exactly 1) and under a
 * 1024 x 1024 BILINEAR noise map, and times the set call and the four move calls with and without maps. */
enum { RPT_MESH_MATERIAL_MAP_OFF = 0, RPT_MESH_MATERIAL_MAP_ON = 1 };
#define RPT_MATERIAL_MAP_CHANNEL_NONE 0xFFFFFFFFu

typedef struct rpt_mesh_material_map {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_MATERIAL_MAP_* ; OFF: width == height == 0, texels == NULL */
    uint32_t width, height;           /* of the map: its own size, need not be the texture's */
    const uint8_t* texels;            /* HOST, RGBA8, row 0 first; copied inside the call */
    uint32_t filter;                  /* RPT_TEX_FILTER_NEAREST / RPT_TEX_FILTER_BILINEAR */
    uint32_t roughness_channel;       /* 0 .. 3 (R, G, B, A) or RPT_MATERIAL_MAP_CHANNEL_NONE; glTF's metallicRoughness: 1 */
    uint32_t metallic_channel;        /* 0 .. 3 or RPT_MATERIAL_MAP_CHANNEL_NONE; glTF's metallicRoughness: 2 */
} rpt_mesh_material_map;

int rpt_set_mesh_material_maps(rpt_ctx* ctx, const rpt_mesh_material_map* items, uint32_t n_items);
int rpt_download_mesh_material_map(rpt_ctx* ctx, uint32_t mesh, float* texels /* host, width*height*4 f32, decoded */, uint32_t width, uint32_t height);

/* ---- mesh emission maps — PROJECT-DEFINED ----------------------------------------------------------------------------------------
 * Per mesh, an emission that varies across the surface: one RGBA8 map, looked up through the mesh's texture UVs, scales the mesh
 * material's EMISSION — where a path hits the mesh, where the mesh-light sampler picks a point on it, and at the emitter exit.  The
 * three act together, so the estimator stays unbiased with next-event estimation; the sampler's pdf does not change, so every
 * multiple-importance weight of the integrator is what it was.  Every operation is stated, so that texels, probed emissions and
 * frames stay checkable bit for bit (tests/test_gpu_mesh_emission_map.py holds them to a numpy restatement).  The statement is
 * written once, in csrc/host_emap.h, which the kernels and the host harness both compile; it reuses tex_decode_value, tex_interp,
 * tex_wrap and tex_lookup of "mesh textures" (csrc/host_tex.h) and does not restate them.  All arithmetic is f32, one rounding per
 * operation, nothing contracted, with the library's correctly rounded divide and root.
 *
 * Scope.  A map is per mesh.  It needs the mesh's texture UVs, as a material map does: an untextured mesh is RPT_ERR_INVALID_ARG (a
 * 1 x 1 white texture is enough).  It has its own size, its own filter and its own gamma; the wrap is the texture's.
 *
 * Decode.  Exactly the decode of "mesh textures", by that section's own launch (no second decode kernel exists): once per call, on
 * the device, the table L[0 .. 255] of the map's `gamma` — L[0] = 0 and L[255] = 1 by definition, rpt_powf(k / 255, gamma) in
 * between, k / 255 when gamma == 1 — then one lane per texel.  A decoded texel is four f32, 16 B: {L[R], L[G], L[B], 0}.
 *
 * Lookup.  E(u, v; a, b, c) for barycentrics (u, v) over a triangle with corners a, b, c in its own order:
 *     w = (1 - u) - v;  s = tex_interp(w, u, v, s_a, s_b, s_c);  t = tex_interp(w, u, v, t_a, t_b, t_c)
 *     E = tex_lookup(the map's decoded texels, W, H, the TEXTURE's wrap, the MAP's filter, s, t)
 * (s_x, t_x) are the corners' UVs of the mesh's texture, W and H the map's, which need not be the texture's.  There is no clamp,
 * for the reason "mesh material maps" gives: BILINEAR over texels in [0, 1] stays in [0, 1].  An all-255 map looks up exactly 1 under
 * either filter and any gamma; any other constant image is returned exactly by NEAREST only.
 *
 * Hit side.  At a winning triangle of a mapped mesh, after the base's hit_material has run (after "mesh textures" has written rgb
 * and "mesh material maps" roughness and metallic):
 *     mat.emission.c = mat.emission.c * E.c           c = r, g, b; one product each
 * with E looked up at the triangle test's own (u, v), recomputed from the ray and the triangle row as "mesh textures" does it — the
 * same operations on the same words — and the corners' UVs read through the refit's slot -> vertex table.  The hit weight w of "mesh
 * lights" is unchanged.
 *
 * Emitter exit.  Where an rpt_light is found in front of the hit, the term the exit adds for the triangle behind it takes the same
 * value: hit_emission's material emission, then the same product with the same E.
 *
 * Sampler side.  For an ON mesh with a map, "sampling an ON mesh" is unchanged except for its emission line: the draws, the
 * triangle pick, the point, the normal and pdf = dist_sq / (A_tot * |c|) all stay.  With su = sqrt(r1), bu = 1 - su, bv = r2 * su
 * (the sampler's own three operations, so the bits are the sampled point's) and a, b, c the picked triangle's corners through the
 * vertex indices the sampler already reads:
 *     E = E(bu, bv; a, b, c);   e.c = m.emission[c] * E.c;   emission.c = N_f * e.c             the products in this order
 * A_tot and the CDF stay area-only: moves add no launch and rpt_download_mesh_light_table is unchanged.  (Weighting the triangle
 * pick by the map's luminance is not done: a map that is dark over most of a mesh makes most samples of it carry no light.)
 *
 * Composition.  Emission maps compose with FLAT / SMOOTH, OFF / ON lights, textures of any wrap and filter, material maps, cutouts,
 * normal maps, and an environment in either mode.  A cutout mesh cannot be a mesh light, so there the map acts on the hit side and
 * at the emitter exit only.  A mesh whose material emission is 0 renders as without the map.  rpt_set_mesh_textures that would
 * remove the texture of a mesh whose map is ON is RPT_ERR_INVALID_ARG ("remove the emission map first"); replacing the texture
 * keeps the map, which then reads the new UVs and wrap.  rpt_set_mesh_lights keeps the maps.  rpt_upload_scene drops all maps.
 *
 * rpt_set_mesh_emission_maps sets (ON) or removes (OFF) the map of the named meshes of the uploaded scene; meshes not named keep
 * theirs.  `texels` is copied inside the call; on return every map is current on every device of the context (one process per GPU:
 * every rank makes the call).  The checks, in this order, all on the host before any device is touched — a rejected call changes
 * nothing, and rpt_last_error starts with "rpt_set_mesh_emission_maps: " and names the item:
 *   RPT_ERR_INVALID_ARG  ctx is NULL;
 *   RPT_ERR_NO_SCENE     no scene with meshes is uploaded;
 *   RPT_ERR_INVALID_ARG  items NULL with a non-zero count; then per item, in order: mesh >= n_meshes, or a mesh named twice; mode
 *                        neither constant; ON with width or height 0 or above 16384; ON with texels NULL; filter not a constant; ON
 *                        with a gamma that is not finite, not above 0 or above 16; OFF with a non-zero size or a non-NULL texels;
 *                        ON on an untextured mesh;
 *   RPT_ERR_UNSUPPORTED  all maps together would hold more than 2^26 texels;
 *   RPT_OK               n_items == 0: nothing is done;
 *   RPT_ERR_HIP          a runtime call failed part-way: the context is left with NO scene, as for the other mesh calls.
 * While some map is ON the scene renders through a kernel of its own — the mesh kernel's body with the three functions above, one
 * form over each of the eight material-mapped forms, picked by (normal maps, cutouts, environment) as those are.  A scene with no
 * material map ON takes them through an all-zero material-map descriptor table carried in the emission maps' own allocation ("no map
 * on this mesh" for every mesh).  Turning every map OFF leaves the context rendering through exactly the kernels and tables it had
 * before the first call.
 *
 * Moves.  rpt_update_meshes, rpt_rebuild_meshes and both _device forms leave maps alone and add no launch: the hit side reads the
 * triangle row the walk tested, the refit's slot -> vertex table and the flattened triangle index, the sampler its own face ->
 * vertex table; neither reads slot order.
 *
 * rpt_download_mesh_emission_map copies one mesh's DECODED texels from the context's first device: width * height * 4 f32.  A mesh
 * out of range, a mesh without a map (it says so), another size or a NULL destination answer RPT_ERR_INVALID_ARG.
 *
 * Memory.  While a map is ON every device holds 16 B per map texel, 48 B per mesh of the scene (the hit side's descriptors by texture
 * ordinal, the sampler's by light ordinal, the all-zero material-map descriptors) and 4 B per triangle of the SCENE (the empty light
 * table); during the call, per device, the new tables beside the old ones and 4 B per texel plus 1 KiB per map being set.  Per hit on
 * a mapped mesh the kernel gathers what a material map's lookup gathers; per sample of a mapped ON mesh the 16 B descriptor, three
 * face -> vertex words, three UVs, the material row and one (NEAREST) or four (BILINEAR) 16 B texels.
 *
 * Registers (gfx950, VGPRs / spilled SGPRs, the material-mapped base form in brackets, no scratch in any form;
 * tools/kernel_meta.py): meshemit 111 / 158 (111 / 156), meshemit_env 113 / 160 (113 / 154), meshemit_cut 111 / 197 (110 / 188),
 * meshemit_cut_env 112 / 185 (112 / 191), meshemit_nrm 111 / 164 (111 / 150), meshemit_nrm_env 113 / 166 (113 / 150),
 * meshemit_nrm_cut 111 / 201 (111 / 193), meshemit_nrm_cut_env 113 / 201 (112 / 185): at most 113 of the 128 VGPRs that four
 * waves per SIMD allow.  The one edit to a header other kernels include (dev_integrator.h: the emitter exit calls a forwarding
 * function that defaults to hit_emission) left every other object of the build byte for byte what it was.
 *
 * Timings (MI355X, 1080p x 16 spp, medians of 5): 0.585 Gsamples/s with the torus ON and no map, 0.572 under an all-255 map (0.977)
 * and 0.571 under a noise map (0.975); rpt_set_mesh_emission_maps for the 1024 x 1024 map 0.6 ms the first time and 0.5 ms again; the
 * four move calls without / with the map, the torus ON in both: update_meshes 1.18 / 1.18 ms; rebuild_meshes 1.74 / 1.76 ms;
 * update_meshes_device 0.92 / 0.91 ms; rebuild_meshes_device 1.49 / 1.50 ms.  tools/mesh_bench.py --emission-maps alternates, in one
 * process, frames of scenes.mesh_scene textured as --textures does with its torus emissive and ON under no map, under an all-255
 * 1024 x 1024 map on the torus (the pure cost of the lookups: every factor is exactly 1) and under a 1024 x 1024 BILINEAR noise map,
 * and times the set call and the four move calls with and without the map. */
enum { RPT_MESH_EMISSION_MAP_OFF = 0, RPT_MESH_EMISSION_MAP_ON = 1 };

typedef struct rpt_mesh_emission_map {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t mode;                    /* RPT_MESH_EMISSION_MAP_* ; OFF: width == height == 0, texels == NULL */
    uint32_t width, height;           /* of the map: its own size, need not be the texture's */
    const uint8_t* texels;            /* HOST, RGBA8, row 0 first (alpha is ignored); copied inside the call */
    uint32_t filter;                  /* RPT_TEX_FILTER_NEAREST / RPT_TEX_FILTER_BILINEAR */
    float gamma;                      /* the decode's exponent, as rpt_mesh_texture's: finite, > 0, <= 16; 1: the bytes are linear */
} rpt_mesh_emission_map;

int rpt_set_mesh_emission_maps(rpt_ctx* ctx, const rpt_mesh_emission_map* items, uint32_t n_items);
int rpt_download_mesh_emission_map(rpt_ctx* ctx, uint32_t mesh, float* texels /* host, width*height*4 f32, decoded */, uint32_t width, uint32_t height);

/* ---- mesh media — PROJECT-DEFINED ------------------------------------------------------------------------------------------------
 * A mesh may bound a homogeneous medium: coloured absorption inside a glass mesh (Beer-Lambert), a glowing volume, fog.  The media
 * arithmetic is "participating media" above, unchanged: phase_hg, sample_hg, the transmittance, steps 1-4 of the bounce loop, the
 * draw order inside a SCATTER medium, Russian roulette, the max_depth accounting, "no nesting" and "false at the camera".  Here is
 * only how a mesh scene reads every word of those steps that says "material".
 *
 * Media come in through rpt_set_mesh_media after the upload, like every other per-mesh feature; a mesh scene uploaded with
 * RPT_SCENE_MEDIA stays RPT_ERR_UNSUPPORTED, and the medium fields of a mesh's rpt_material are not read.
 *
 * Which medium a hit carries.  A winning triangle carries its mesh's medium, if that mesh has one that is not NONE.  A hit on a
 * sphere or a plane carries none: in_medium and state.medium stay as they are (the existing rule for a material without a medium).
 * In a mesh scene only meshes have media.
 *
 * Step 4, the side test.  After the next ray is set, if the winning triangle's mesh carries a medium:
 *     in_medium = dot(new ray direction, G) < 0,   G = normalize(cross(e1, e2))
 * G is the FLAT normal of the winning triangle — the very value a FLAT mesh without a normal map has as its hit normal, not turned
 * toward the ray — and when the test is true state.medium = that mesh's medium.  Smooth shading and normal maps bend what the BSDF
 * sees; they do not move the boundary.  For a FLAT mesh without a map this is bit for bit step 4 as written above.
 *
 * Step 1 at a miss.  The background, or the environment with its miss-side MIS weight (which reads scatter_sample.pdf: after a medium
 * scatter the phase pdf), is added unattenuated, also inside a medium.
 *
 * Steps 2 and 3, light samples.  The pick is the mesh scenes' pick ("pickable lights"): N = n_lights + ON meshes + (1 if the
 * environment is SAMPLED), the environment last.  At a scatter point scatter_pos is the point itself: no eps offset, no normal.  The
 * facing test of the sampled light is unchanged.  The phase function stands in place of the BSDF for f, pdf and the MIS weight.  The
 * unoccluded `li` is multiplied by the medium's transmittance over light_sample.dist only when that distance is finite: an
 * environment sample (dist = +inf) is never attenuated.  The mesh-light hit weight and the emitter exit read scatter_sample.pdf as
 * always.
 *
 * Shadow rays stay the scene's binary any_hit, cutouts included: a medium's own boundary occludes lights outside it.  A hole in a
 * cutout boundary lets a path through without changing in_medium, because no triangle was hit there.
 *
 * Composes with FLAT / SMOOTH, lights OFF / ON (a mesh may be both ON and carry a medium), textures, material, emission and normal
 * maps, cutouts and an environment.  rpt_update_meshes, rpt_rebuild_meshes and their _device forms leave the media alone and add no
 * launch: the tables go by mesh and by flattened triangle index, never by slot.  An upload drops every medium.
 *
 * rpt_set_mesh_media follows rpt_set_mesh_lights in every convention: listed meshes change, the others stay; n_items == 0 is RPT_OK
 * and does nothing; everything is checked before anything is stored, so a rejected call changes nothing; a runtime failure part-way
 * leaves the context with no scene.  RPT_ERR_NO_SCENE unless the scene has meshes.  RPT_ERR_INVALID_ARG, in this order: items NULL
 * with a non-zero count; then per item mesh >= n_meshes, a mesh named twice, a type beyond RPT_MEDIUM_EMISSIVE, a negative or
 * non-finite density, a non-finite colour, a non-finite anisotropy.  RPT_ERR_UNSUPPORTED when more than 32766 meshes would carry a
 * medium (what a path can remember).  The anisotropy is clamped to [-0.9, 0.9] as Material::finalize does, once, in the call.  An
 * item of type NONE removes the mesh's medium (its other fields are checked and dropped).  When the last medium goes back to NONE
 * the context renders exactly as if the call had never been made: same kernel, same tables.  On a rpt_create_multi context the call
 * writes every device; ranks of rpt_create_rank each call it.
 *
 * Kernel forms: eight, one over each emission-mapped form (a scene without emission maps, material maps, textures or mesh lights
 * reaches them through empty tables the media's own allocation carries), strict arithmetic only: RPT_RENDER_FAST_MATH, NESTED_LOOPS
 * and SMALL_COMPACT stay unsupported for mesh scenes; RPT_RENDER_RUSSIAN_ROULETTE works, as it does after a medium scatter elsewhere.
 *
 * Registers (gfx950, VGPRs / spilled SGPRs, the emission-mapped base form in brackets, no scratch in any form;
 * tools/kernel_meta.py): meshmed 116 / 162 (111 / 158), meshmed_env 118 / 164 (113 / 160), meshmed_cut 116 / 216 (111 / 197),
 * meshmed_cut_env 118 / 224 (112 / 185), meshmed_nrm 116 / 164 (111 / 164), meshmed_nrm_env 118 / 162 (113 / 166),
 * meshmed_nrm_cut 116 / 220 (111 / 201), meshmed_nrm_cut_env 118 / 228 (113 / 201): at most 118 of the 128 VGPRs that four waves per
 * SIMD allow.  The one edit to a header other kernels include (dev_integrator.h: step 4's side test reads its normal through a
 * forwarding function that defaults to the caller's) left the code objects of every other library what they were.
 *
 * Timings (MI355X, 1080p x 16 spp, medians of 5): 0.565 Gsamples/s with no medium, 0.552 with an ABSORB medium on the glass icosphere
 * (0.977) and 0.421 with a SCATTER medium on it (0.745: the fog frames do more work per path by construction); rpt_set_mesh_media
 * 6-7 ms the first time on a context (it makes the refit tables) and 0.36 ms again; the four move calls without / with a medium:
 * update_meshes 0.44 / 0.44 ms; rebuild_meshes 1.02 / 1.00 ms; update_meshes_device 0.16 / 0.16 ms; rebuild_meshes_device 0.73 /
 * 0.73 ms.  tools/mesh_bench.py --media alternates, in one process, frames of scenes.mesh_scene with its icosphere made glass under no
 * medium, an ABSORB medium and a SCATTER medium on it, and times the set call and the four move calls with and without a medium. */
typedef struct rpt_mesh_medium {
    uint32_t mesh;                    /* index into the uploaded scene's rpt_scene_desc.meshes */
    uint32_t medium_type;             /* RPT_MEDIUM_* ; RPT_MEDIUM_NONE removes the mesh's medium */
    float density;
    float color[3];
    float anisotropy;                 /* clamped to [-0.9, 0.9] as Material::finalize does */
} rpt_mesh_medium;

int rpt_set_mesh_media(rpt_ctx* ctx, const rpt_mesh_medium* items, uint32_t n_items);
/* What the context holds for `mesh`: the clamped anisotropy; RPT_MEDIUM_NONE and zeros for a mesh without a medium. */
int rpt_download_mesh_medium(rpt_ctx* ctx, uint32_t mesh, rpt_mesh_medium* out);

/* ---- ray queries — PROJECT-DEFINED ------------------------------------------------------------------------------------------------
 * A context that holds a mesh scene answers questions about it for rays the caller brings: what a ray hits first (rpt_trace_rays*),
 * whether anything lies along it (rpt_occluded*), what the surface there is (rpt_surface), and which rays the camera sends
 * (rpt_camera_rays_device).  One call serves any mesh scene, whatever features are set; no render form, setter or hook changes.
 *
 * Closest hit.  The answer is the integrator's: the geometry pass of closest_hit of "triangle meshes", exactly — spheres, then planes,
 * then the flattened triangles, from dist = F::MAX, with the acceptance rules stated there.  A scene with cutouts ON uses the cut test
 * inside the walk ("mesh cutouts"): a ray through a hole goes on.  rpt_lights are not geometry and are never reported.  max_dist is not
 * read by the closest query.
 *   the winner   the triangle, if the walk returned one; otherwise the last accepted plane, that is, the highest accepted index;
 *                otherwise the nearest sphere; otherwise RPT_HIT_NONE
 *   t            the accepted distance, bit for bit; +inf's bits for NONE.  A primitive accepted by the "first primitive" rule —
 *                sphere 0, or plane 0 of a scene without spheres — carries whatever t its test returned, as in the integrator: for
 *                a ray with a NaN or infinite component the sphere test can return a NaN, which is then the answer (kind SPHERE,
 *                t a NaN whose sign and payload are the hardware's), and no later primitive is nearer than a NaN
 *   primitive    the index into spheres / planes / the flattened triangle list; 0xFFFFFFFF for NONE
 *   mesh, triangle   the mesh and the index within the mesh; 0xFFFFFFFF unless a triangle won
 *   u, v         the triangle test's u and v, in its operation order — the very values textures and smooth normals interpolate with;
 *                0 for anything but a triangle
 *   reserved     written 0 in outputs, ignored in rpt_ray
 * A ray with a NaN component hits no triangle ("triangle meshes"); what the spheres and planes answer is what their tests answer.
 *
 * rpt_surface is written only when surfaces_dev / surfaces is not NULL.  It holds what SHADE would build for this hit before
 * State::finalize:
 *   ng           the geometric normal: for a triangle normalize(cross(e1, e2)), NOT turned toward the ray; for spheres and planes the
 *                integrator's normal
 *   ns           the normal the scene's hit_normal returns: smooth interpolation ("smooth mesh shading") and the normal map ("mesh
 *                normal maps") where they are ON; ng's bits where they are not
 *   rgb, roughness, metallic   those fields of the material after the scene's hit_material: texture, material map, and the planes'
 *                layered patches over the nearest sphere's
 *   emission     hit_emission_at: an emission map multiplies it ("mesh emission maps")
 *   material     the winner's index into materials
 * For RPT_HIT_NONE everything is zero.
 *
 * Occlusion.  occluded[i] = 1 when some sphere, plane or triangle (one that passes the cut test) is hit with t < max_dist, otherwise 0.
 * The ray's max_dist is always honoured, whatever RPT_SCENE_ANYHIT_USES_MAX_DIST says; pass +inf for "anything along the ray".  A NaN
 * max_dist gives 0.
 *
 * Camera rays.  rpt_camera_rays_device writes width * height rays, row 0 on top, pixel (x, y) at y * width + x: each the reference
 * camera's ray for that pixel with both jitter draws replaced by 0.5f — camera_ray(make_camera(...), px, py, 0.5, 0.5), the very
 * function and frame-invariant part a render uses, px and py what a render launch computes for the pixel — and max_dist = +inf.
 * Tracing these rays with surfaces_dev gives first-hit depth (t), normal (ng, ns), albedo (rgb) and id (primitive, mesh, material)
 * buffers: what a compositor or an external denoiser asks for.
 *
 * Ordering.  The _device forms enqueue on `stream` and return without waiting.  They see the effect of every earlier call on the
 * context — uploads, the four move calls, every setter: those calls wait for their own device work before they return.  Work of the
 * CALLER's on another stream (the kernel that writes rays_dev, a reader of hits_dev) is the caller's to order, as with
 * rpt_render_device's buffers.  rays_dev, hits_dev and surfaces_dev must be 16-byte aligned (occluded_dev, a byte array, needs no
 * alignment) and all of them on the context's device; a misaligned pointer is rejected whatever n is.  The host forms stage through device
 * memory of the context and block.  The first query after an upload makes a small allocation of the query's own (the meshes'
 * first-triangle offsets and the empty tables that stand for absent features) and waits for it once.
 *
 * Errors.  RPT_ERR_NO_SCENE without a scene; RPT_ERR_UNSUPPORTED for a scene that is not a mesh scene (analytical, large and SDF
 * scenes: not yet) and for a context with more than one local device (an rpt_create_rank context has one and works);
 * RPT_ERR_INVALID_ARG for a NULL ctx, a NULL array with n > 0, a misaligned pointer, flags != 0 (reserved), zero width or height, and
 * more rays than a grid of 0x7FFFFFFF workgroups of 256 holds.  n == 0 is RPT_OK and launches nothing.  A rejected call writes
 * nothing.
 *
 * The kernels (csrc/k_query.hip, a code object library of their own) are nine: closest and occluded, each without and with the cut
 * test; the closest hit with its surface per normal map x cutout; the camera's rays.  One ray per lane, the ray read as two 16-byte
 * loads, rpt_hit written as two 16-byte stores and rpt_surface as four.  DESIGN.md ("ray queries") has their registers and rates. */
typedef struct rpt_ray {
    float origin[3];
    float max_dist;                   /* occlusion only: hits at t >= max_dist do not count */
    float direction[3];               /* as handed to the integrator: not normalised here */
    uint32_t reserved;
} rpt_ray;                            /* 32 B */

enum { RPT_HIT_NONE = 0, RPT_HIT_SPHERE = 1, RPT_HIT_PLANE = 2, RPT_HIT_TRIANGLE = 3 };

typedef struct rpt_hit {
    float t;
    uint32_t kind;                    /* RPT_HIT_* */
    uint32_t primitive;
    uint32_t mesh;
    uint32_t triangle;
    float u, v;
    uint32_t reserved;
} rpt_hit;                            /* 32 B */

typedef struct rpt_surface {
    float ng[3];
    float ns[3];
    float rgb[3];
    float emission[3];
    float roughness, metallic;
    uint32_t material;
    uint32_t reserved;
} rpt_surface;                        /* 64 B */

#if defined(__cplusplus)
static_assert(sizeof(rpt_ray) == 32 && sizeof(rpt_hit) == 32 && sizeof(rpt_surface) == 64, "ray query records are 32, 32 and 64 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rpt_ray) == 32 && sizeof(rpt_hit) == 32 && sizeof(rpt_surface) == 64, "ray query records are 32, 32 and 64 bytes");
#endif

int rpt_trace_rays_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, rpt_hit* hits_dev, rpt_surface* surfaces_dev /* or NULL */,
                          uint32_t flags, void* stream);
int rpt_occluded_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, uint8_t* occluded_dev, uint32_t flags, void* stream);
int rpt_camera_rays_device(rpt_ctx* ctx, uint32_t width, uint32_t height, rpt_ray* rays_dev, void* stream);
int rpt_trace_rays(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, rpt_hit* hits, rpt_surface* surfaces /* or NULL */, uint32_t flags);   /* host memory, blocks */
int rpt_occluded(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, uint8_t* occluded, uint32_t flags);                                     /* host memory, blocks */

/* ---- radiance queries — PROJECT-DEFINED ---------------------------------------------------------------------------------------------
 * How much light arrives along a ray the caller brings: the integrator's own estimate, with every feature the context has set —
 * smooth shading, mesh lights, textures, the three kinds of maps, cutouts, the environment, media.  Light probes, irradiance volumes,
 * lightmap baking and a camera model of the caller's own ask this.  Ray queries (above) stop at geometry; these keep path state and
 * draw random numbers.  One call serves any mesh scene, whatever features are set; no render form, setter or hook changes.
 *
 * One sample.  Sample s of ray i is one pass of the integrator's bounce loop (tracer.rs:61-103, as the mesh render forms run it),
 * started from rays[i].origin and rays[i].direction exactly as given: the direction is not normalised (rpt_ray), and max_dist and
 * reserved are not read.
 *   the stream   Rng::init(frame_key(seed, frames_done + s), first_index + i), first_index + i in uint32 arithmetic (it wraps)
 *   two draws    the stream's first two draws are made and discarded: the draws a camera sample spends on its jitter
 *   the rest     as a camera path starts: hit_dist = -1, scatter_pdf = 0, bounce 0, throughput 1, radiance 0, not inside any medium.
 *                A ray whose origin lies inside a mesh that bounds a medium starts OUTSIDE it, as a camera placed there does
 *                ("mesh media": a path enters a medium by crossing its boundary)
 * Russian roulette is a render flag and is never applied here.
 *
 * Accumulation.  out[i] (4 f32) is a ColorBuffer pixel, read and written.  The spp samples enter it in sample order through the
 * render's own blend (mix_color, tracer.rs:108-117) with weight 1 / (frames_done + s + 1); alpha is blended toward 1, and a sample
 * that is not finite is blended as black.  spp = S is bit-identical to S calls with spp = 1 and frames_done counted up; the library
 * cuts spp above the kernels' samples-per-launch limit (512) into successive launches, which changes no word.  spp == 0 or n == 0 is
 * RPT_OK and launches nothing.  A scene with max_depth == 0 blends zeros.
 *
 * The camera's sample rays.  rpt_camera_sample_rays_device writes width * height rays, row 0 on top, pixel (x, y) at y * width + x:
 * the ray a render of frame `frame` with `seed` sends for that pixel — camera_ray(make_camera(...), px, py, offx, offy), px and py what
 * a render launch computes for the pixel, offx and offy the first two draws of the stream (seed, frame, pixel index) — and
 * max_dist = +inf.  (rpt_camera_rays_device is the same with both draws replaced by 0.5f.)
 *
 * Therefore, for every mesh scene and every feature set: rpt_radiance_device over these rays with first_index = 0, frames_done =
 * frame and spp = 1, into a copy of a ColorBuffer, leaves THE VERY WORDS rpt_render_device (flags 0) leaves there for that frame.
 * tests/test_gpu_radiance.py holds all 36 render forms to this.
 *
 * Ordering.  The _device forms enqueue on `stream` and return without waiting.  They see the effect of every earlier call on the
 * context — uploads, the four move calls, every setter: those calls wait for their own device work before they return.  Work of the
 * CALLER's on another stream (the kernel that writes rays_dev, a reader of out_dev) is the caller's to order, as with
 * rpt_render_device's buffers.  rays_dev and out_dev must be 16-byte aligned and on the context's device; a misaligned pointer is
 * rejected whatever n is.  rpt_radiance stages through device memory of the context and blocks.  The first radiance query after an
 * upload makes a small allocation of its own (the empty tables that stand for absent features: host_rad.h) and waits for it once.
 *
 * Errors.  RPT_ERR_NO_SCENE without a scene; RPT_ERR_UNSUPPORTED for a scene that is not a mesh scene and for a context with more
 * than one local device (an rpt_create_rank context has one and works); RPT_ERR_INVALID_ARG for a NULL ctx, a NULL array with n > 0,
 * a misaligned pointer, flags != 0 (reserved), zero width or height, more rays than a grid of 0x7FFFFFFF workgroups of 256 holds, and
 * frames_done + spp > 2^64 - 1 (the launch domain, rpt_render: frames_done is a stream selector here, and every 64-bit value is one).
 * A rejected call writes nothing.  rpt_debug_mesh_form and rpt_debug_kernel_choice (rpt_test.h) keep reporting the last RENDER launch.
 *
 * The kernels (csrc/k_rad.hip, a code object library of their own) are nine: the render's path-regenerating state machine over a
 * 1-D grid of rays, 256 per workgroup, a wave's lanes sharing their rays' samples, per normal map x cutout x environment over the
 * media forms' scene types; and the camera's sample rays.  DESIGN.md ("radiance queries") has their registers, LDS and rates. */
int rpt_radiance_device(rpt_ctx* ctx, const rpt_ray* rays_dev, uint64_t n, float* out_dev /* n x 4 f32, in/out */, uint64_t frames_done, uint32_t spp,
                        uint64_t seed, uint32_t first_index, uint32_t flags /* reserved: 0 */, void* stream);
int rpt_radiance(rpt_ctx* ctx, const rpt_ray* rays, uint64_t n, float* out, uint64_t frames_done, uint32_t spp, uint64_t seed, uint32_t first_index,
                 uint32_t flags);                                                                                                       /* host memory, blocks */
int rpt_camera_sample_rays_device(rpt_ctx* ctx, uint32_t width, uint32_t height, uint64_t frame, uint64_t seed, rpt_ray* rays_dev, void* stream);

/* Tracer::render (tracer.rs:22-123) on a HOST ColorBuffer.
 *   pixels      in/out, width*height*4 f32, RGBA, row 0 = top (buffer.rs:6-26)
 *   frames_done ColorBuffer.frames before the call; the caller adds `spp` afterwards
 *   spp         number of render() calls to fold into this one; spp = 1 is exactly
 *               one reference render(); spp = S is bit-identical to S calls
 *   seed        RNG seed (the reference's thread_rng, tracer.rs:44, is unseedable)
 * Blocks until `pixels` holds the result.
 *
 * The launch domain — PROJECT-DEFINED.  Every 64-bit value of frames_done and of seed is a frame and a seed of its own: both words
 * of either enter the stream's key (frame_key), and sample s is frame frames_done + s in 64-bit arithmetic wherever a call is cut
 * into launches or chunks.  The weight of frame f is 1 / (float)(f + 1), the conversion rounded to nearest even (exact below 2^24).
 * The domain ends at frames_done + spp <= 2^64 - 1: one sample further f + 1 wraps to 0, the weight is infinite and the pixel NaN
 * for good.  Beyond it rpt_render, rpt_render_device, rpt_resident_render (against the resident counter) and
 * rpt_radiance / rpt_radiance_device return RPT_ERR_INVALID_ARG and write nothing; spp == 0 is inside it for every frames_done.
 * width or height may be 1.  tests/test_launch_domain.py and tests/test_gpu_launch_domain.py hold the ends of this domain. */
int rpt_render(rpt_ctx* ctx, float* pixels, uint32_t width, uint32_t height,
               uint64_t frames_done, uint32_t spp, uint64_t seed, uint32_t flags);

/* ---- resident ColorBuffer (the reference's interactive loop without the PCIe round trip) --------------
 * renderer/src/main.rs:113-124 does, per redraw: pt.render(&mut buffer); buffer.convert_to_u8(frame).  With
 * rpt_render that moves 2 x 16 B per pixel over PCIe per frame.  Here the context owns a device ColorBuffer
 * (pixels + frames, buffer.rs:6-14): render accumulates into it, and the host fetches either the f32 pixels or
 * directly the gamma-encoded u8 frame (4 B per pixel).  Changing width/height or calling rpt_resident_reset
 * starts a new buffer (ColorBuffer::new, buffer.rs:18-26). */
/* (the launch domain, rpt_render: resident frames + spp <= 2^64 - 1, else RPT_ERR_INVALID_ARG and neither the buffer nor the counter changes) */
int rpt_resident_render(rpt_ctx* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t seed, uint32_t flags);
int rpt_resident_frames(const rpt_ctx* ctx, uint64_t* frames);          /* ColorBuffer.frames */
/* Device time of the last rpt_resident_render's launches (HIP events on the stream they ran on; the slowest of this
 * context's devices).  Waits for them. */
int rpt_resident_kernel_ms(rpt_ctx* ctx, float* ms);
int rpt_resident_download(rpt_ctx* ctx, float* pixels);                 /* width*height*4 f32 */
int rpt_resident_download_u8(rpt_ctx* ctx, uint8_t* frame);             /* convert_to_u8 on the device, width*height*4 bytes */
int rpt_resident_reset(rpt_ctx* ctx);
/* Page-lock a host buffer the caller will hand to rpt_resident_download[_u8] / rpt_render again and again (the redraw loop's
 * frame, renderer/src/main.rs:122): copies to and from page-locked memory are one DMA at the link's rate (8.3 MB of a 1080p u8
 * frame: ~0.2 ms), copies to pageable memory are staged by the runtime at ~7 GB/s (1.2 ms).  The buffer must stay allocated
 * until rpt_host_unpin; a buffer the caller has registered with HIP itself is as good.  Not needed for correctness. */
int rpt_host_pin(void* buffer, size_t bytes);
int rpt_host_unpin(void* buffer);
/* The resident image assembled ON THE ROOT DEVICE (no PCIe): RCCL gather of the tiles + scatter kernel, enqueued
 * behind the renders on the context's streams.  image_dev: width*height*4 f32 on rank 0's device (ignored on other
 * ranks; NULL = into the context's own staging image).  Returns without waiting; rpt_resident_sync waits.
 * world = 1: a device-to-device copy. */
int rpt_resident_gather_device(rpt_ctx* ctx, float* image_dev);
/* Block until everything enqueued on this context's devices has finished. */
int rpt_resident_sync(rpt_ctx* ctx);
/* Start the resident buffer from a host ColorBuffer (pixels + frames): what resuming a cloned ColorBuffer is in the
 * reference (buffer.rs:5 derives Clone).  Each rank uploads only the rows it owns. */
int rpt_resident_upload(rpt_ctx* ctx, const float* pixels, uint32_t width, uint32_t height, uint64_t frames);

/* Same on a DEVICE-resident buffer, asynchronously on `stream` (a hipStream_t; NULL is
 * HIP's null stream).  With world > 1 the image is row-tiled: rows are
 * dealt in blocks of `tile_rows` rows, block b to rank b % world, and `pixels` is
 * this rank's COMPACT tile buffer (rpt_tile_row_count(...) rows of `width` RGBA
 * pixels).  The RNG is keyed by the global pixel, so the image does not depend on
 * world.  world = 1, rank = 0 renders the whole image in place.
 * Calls on one context are ordered by the caller (one thread at a time).  The wavefront form of large scenes keeps its paths in
 * buffers of the context: a launch on another stream than the previous one waits (on the device) for that one to finish with
 * them; use one context per render that is to run concurrently. */
/* (the launch domain, rpt_render: frames_done + spp <= 2^64 - 1, else RPT_ERR_INVALID_ARG and nothing is enqueued) */
int rpt_render_device(rpt_ctx* ctx, float* pixels_dev, uint32_t width, uint32_t height,
                      uint64_t frames_done, uint32_t spp, uint64_t seed, uint32_t flags,
                      uint32_t tile_rows, uint32_t rank, uint32_t world, void* stream);

/* Number of image rows rank `rank` owns under the cyclic row-block tiling. */
uint32_t rpt_tile_row_count(uint32_t height, uint32_t tile_rows, uint32_t rank, uint32_t world);
/* Global image row of local row `local_row` of rank `rank`. */
uint32_t rpt_tile_global_row(uint32_t local_row, uint32_t tile_rows, uint32_t rank, uint32_t world);
/* Rows of the largest tile: what every rank's tile buffer is padded to, so that the gather moves equal counts. */
uint32_t rpt_tile_rows_padded(uint32_t height, uint32_t tile_rows, uint32_t world);
/* How a rank's rows move between a top-down host image and its compact tile (what rpt_render / rpt_resident_upload
 * do per device, each over its own PCIe link): `full_blocks` blocks of `block_rows` rows, block i at host row
 * host_row0 + i * host_row_stride and at tile row i * block_rows (ONE strided copy), plus `ragged_rows` rows of the
 * image's short last block from host row ragged_host_row0 to tile row ragged_tile_row0 when this rank owns it. */
typedef struct rpt_tile_plan {
    uint32_t full_blocks, block_rows, host_row0, host_row_stride;
    uint32_t ragged_rows, ragged_host_row0, ragged_tile_row0;
} rpt_tile_plan;
int rpt_tile_copy_plan(uint32_t height, uint32_t tile_rows, uint32_t rank, uint32_t world, rpt_tile_plan* out);

/* Scatter a rank-major concatenation of compact tiles (what an all-gather of the
 * per-rank tile buffers yields, each padded to `rows_padded` rows) into the full
 * top-down image, on the device. */
int rpt_untile_device(rpt_ctx* ctx, const float* gathered_dev, float* image_dev,
                      uint32_t width, uint32_t height, uint32_t tile_rows,
                      uint32_t world, uint32_t rows_padded, void* stream);

/* ColorBuffer::convert_to_u8 (buffer.rs:55-64): powf(0.4545)*255 saturating cast to
 * u8 for r,g,b; a*255 for alpha.  Device buffers; the step that follows render in the
 * reference's only caller (renderer/src/main.rs:118-122). */
int rpt_convert_to_u8_device(rpt_ctx* ctx, const float* pixels_dev, uint8_t* out_dev,
                             uint32_t width, uint32_t height, void* stream);

/* ColorBuffer::convert_to_u8_at (buffer.rs:67-89): blit the buffer into a larger u8 frame (frame_width x
 * frame_height, exactly that many RGBA bytes) at offset (at_x, at_y): no gamma, p*255 saturating cast, only
 * x in (at_x, at_x + width) and y in (at_y, at_y + height) with y = frame row + 1 — the reference's bounds. Pixels
 * outside keep their previous contents.  Device buffers. */
int rpt_convert_to_u8_at_device(rpt_ctx* ctx, const float* pixels_dev, uint32_t width, uint32_t height, uint8_t* frame_dev,
                                uint32_t at_x, uint32_t at_y, uint32_t frame_width, uint32_t frame_height, void* stream);

/* ---- denoiser ("Implement a denoiser" is a Todo of the reference, Readme.md:14) — PROJECT-DEFINED -----------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on the colour buffer alone, run in a compressed colour
 * space so that fireflies do not dominate: a separate pass over a ColorBuffer, never part of render().  There is no reference
 * behaviour to match; the arithmetic (f32, this operation order) is the one in oracle/rpt_oracle.hpp, denoise():
 *   c' = c / (1 + c)                                       per r, g, b of every pixel (alpha is not filtered)
 *   iteration i = 0 .. iterations-1, step s = 2^i, k_i = edge_k * 4^i; for every pixel p, over the 3x3 taps
 *   q = p + s * (dx, dy), dy = -1..1 outer, dx = -1..1 inner, q inside the image:
 *       d = c'_p - c'_q;  d2 = fma(d.r, d.r, fma(d.g, d.g, d.b*d.b));  a tap whose d2 is not < inf (NaN or +inf) is skipped;
 *       t = fma(-d2, k_i, 1);  g = t > 0 ? t : 0;  wt = (H[dy+1] * H[dx+1]) * (g * g),  H = {0.25, 0.5, 0.25};
 *       acc = fma(c'_q, wt, acc);  wsum += wt          (fma: ONE rounding, written out on both sides since round 4)
 *   c'_p <- wsum > 0 ? acc / wsum : c'_p                   (all pixels at once: out of place)
 *   finally c = c' / (1 - c'), alpha = the input's.  A pixel whose compressed colour is not finite — an input r, g or b that is
 *   NaN, +-inf or exactly -1 (c' = -inf) — is copied through unchanged and takes no part in its neighbours' sums (every tap
 *   that reaches it has d2 NaN or +inf), so it makes no other pixel non-finite.  For a finite compressed colour |c'| <= 1.7e7
 *   and d2 <= ~4e15: skipping +inf as well as NaN changes no other pixel.
 * The filter is a weighted mean of compressed colours: it darkens a noisy region slightly (1-4 % at 1-4 spp on the
 * reference's scene; tests/test_denoise.py) — the price of taming fireflies without auxiliary buffers.
 * iterations 1..6 (footprint 2^(iterations+1) - 1 pixels), edge_k > 0 (larger = sharper edges, less smoothing; 2 is a good
 * default at 1-16 spp).  Per iteration the pass reads and writes the buffer once: 32 B per pixel of HBM traffic.
 * pixels_dev and out_dev are width*height*4 f32 device buffers and must not overlap; the context keeps one more buffer of
 * that size between calls. */
int rpt_denoise_device(rpt_ctx* ctx, const float* pixels_dev, float* out_dev, uint32_t width, uint32_t height,
                       uint32_t iterations, float edge_k, void* stream);
/* The same on HOST buffers (upload, filter, download; blocks). */
int rpt_denoise(rpt_ctx* ctx, const float* pixels, float* out, uint32_t width, uint32_t height, uint32_t iterations, float edge_k);

/* ---- guided denoiser — PROJECT-DEFINED -------------------------------------------------------------------------------------------------
 * The filter of "denoiser" with the normal and position buffers of Dammertz et al. restored, a key that no tap crosses, and albedo
 * demodulation: texture detail is divided out before filtering and multiplied back afterwards.  Its auxiliary buffers are first-hit
 * GUIDES, one rpt_guide per pixel, packed from the records of "ray queries" (rpt_camera_rays_device, then rpt_trace_rays_device with
 * surfaces).  Guides are a record of their own so that a static camera packs them once and filters every progressive frame against
 * them; a caller may also write guides of their own (a key per material, say).  Neither call needs a scene: guides are a function of
 * the three records alone, the filter of pixels and guides alone.
 *
 * Packing (rpt_denoise_guides*), per record i, every operation rounded once, nothing fused:
 *   kind = hit.kind
 *   RPT_HIT_NONE     everything 0, except t = +inf and albedo = 1, 1, 1
 *   otherwise        t = hit.t;  position_c = origin_c + direction_c * t;  ns, ng and albedo = rgb copied from rpt_surface;
 *                    key = (kind << 28) | (id & 0x0FFFFFFF), id = hit.mesh for a triangle, hit.primitive otherwise
 *   reserved = 0.
 *
 * The filter (rpt_denoise_guided*), f32 in this operation order, H = {0.25, 0.5, 0.25}, FLOOR = 1/64:
 *   1 compress, per r, g, b of every pixel:  a = albedo < FLOOR ? FLOOR : albedo;  e = c / a (the IEEE quotient);  c' = e / (1 + e)
 *   2 the pixel's plane scale:  kx_p = plane_k > 0 ? plane_k / (t_p * t_p) : 0
 *   3 iteration i = 0 .. iterations-1, step s = 2^i, k_i = edge_k * 4^i (f32 products); for every pixel p, over the 3x3 taps
 *     q = p + s * (dx, dy), dy = -1..1 outer, dx = -1..1 inner:
 *         d = c'_p - c'_q;  d2 = fma(d.r, d.r, fma(d.g, d.g, d.b*d.b));  dn2 = the same expression on ns_p - ns_q;
 *         r = position_q - position_p;  dpl = fma(ng_p.x, r.x, fma(ng_p.y, r.y, ng_p.z*r.z));  dp2 = dpl*dpl;
 *         the tap is skipped when q lies outside the image, when key_q != key_p, or when any of d2, dn2, dp2 is not < inf;
 *         tc = fma(-d2, k_i, 1);  tn = fma(-dn2, normal_k, 1);  tx = fma(-dp2, kx_p, 1);  each g = t > 0 ? t : 0;
 *         wt = (((H[dy+1] * H[dx+1]) * (gc*gc)) * (gn*gn)) * (gx*gx);  acc = fma(c'_q, wt, acc);  wsum += wt
 *     c'_p <- wsum > 0 ? acc / wsum : c'_p               (all pixels at once: out of place; guides are never filtered)
 *   4 expand:  e = c' / (1 - c');  out = e * a;  alpha = the input's.  A pixel whose e of step 1 has a channel that is NaN, +-inf or
 *     exactly -1 is copied through unchanged.
 * Every g lies in [0, 1] and wt in [0, 0.25]; neither can be NaN, because t > 0 is false for a NaN.  Consequences:
 *   - miss pixels (key 0, t = +inf, normals 0) filter among themselves, and only by colour;
 *   - a NaN t or position keeps its pixel unchanged: every tap of it, its own included, has a NaN dp2 or a weight of 0;
 *   - plane_k is dimensionless: the tap's distance from the centre's tangent plane relative to the centre's depth;
 *   - first-hit guides do not describe what a mirror or a glass shows: there the colour term is the only one that sees the edge;
 *   - a packed guide is sampled at the pixel's centre, the pixel's colour is the mean over its footprint: a pixel that straddles a
 *     texture edge is divided by an albedo that is too small or too large by up to the texture's contrast, and the filter spreads
 *     that.  On frames whose pixels are large against the texture's features and whose contrast is high (60 : 1 at 64 x 48:
 *     tests/test_gpu_denoise_guided.py) the textured surfaces come out worse than from the colour-only filter; a caller who
 *     has them can write guides whose albedo is averaged over the footprint;
 *   - with guides that are all the RPT_HIT_NONE record every extra factor is exactly 1, a and 1/a are 1, and the call returns the
 *     very words rpt_denoise_device returns.
 * iterations 1..6, edge_k > 0 and finite, normal_k >= 0 and plane_k >= 0 and both finite (0 switches the term off), flags reserved: 0.
 * Defaults that serve 1-4 spp: 4 iterations, edge_k 0.25, normal_k 4, plane_k 1000 (the colour term may be much looser than in
 * "denoiser": the guides hold the geometric edges).  What the guides do not hold — shadows, highlights — only the colour term keeps:
 * from about 16 spp on, 2-3 iterations and edge_k 2 blur less than the noise costs.
 *
 * Arguments and errors.  Every pointer 16-byte aligned and (the _device forms) on the context's device; out must overlap neither
 * pixels nor guides.  RPT_ERR_INVALID_ARG for a NULL ctx, a NULL array (with n > 0, for the pack), a misaligned pointer whatever n is,
 * an argument out of the ranges above or a NaN, flags != 0, zero width or height, and more records than a grid of 0x7FFFFFFF workgroups
 * of 256 holds.  n == 0 is RPT_OK and launches nothing.  A rejected call writes nothing.  The _device forms enqueue on `stream` and
 * return; the filter shares the context's intermediate buffer with rpt_denoise_device, under the same rule for streams.  The host
 * forms stage through device memory of the context and block.
 *
 * The kernels (csrc/k_gdn.hip, a code object library of their own) are four: the pack; the first two iterations fused through LDS on
 * 32 x 16 tiles (and its one-iteration form), staging per cell the compressed colour and the 32 bytes of guide a tap reads
 * (position, key, ns, t), the centre's ng and albedo read once per pixel; a step kernel for the later iterations.  Every record moves
 * as 16-byte loads and stores.  DESIGN.md ("guided denoiser") has their registers, LDS and rates. */
typedef struct rpt_guide {
    float position[3]; uint32_t key;
    float ns[3];       float t;
    float ng[3];       uint32_t kind;      /* RPT_HIT_* */
    float albedo[3];   uint32_t reserved;  /* written 0 */
} rpt_guide;                               /* 64 B */

#if defined(__cplusplus)
static_assert(sizeof(rpt_guide) == 64, "a guide is 64 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rpt_guide) == 64, "a guide is 64 bytes");
#endif

int rpt_denoise_guides_device(rpt_ctx* ctx, const rpt_ray* rays_dev, const rpt_hit* hits_dev, const rpt_surface* surfaces_dev, uint64_t n,
                              rpt_guide* guides_dev, void* stream);
int rpt_denoise_guides(rpt_ctx* ctx, const rpt_ray* rays, const rpt_hit* hits, const rpt_surface* surfaces, uint64_t n, rpt_guide* guides);   /* host memory, blocks */
int rpt_denoise_guided_device(rpt_ctx* ctx, const float* pixels_dev, const rpt_guide* guides_dev, float* out_dev, uint32_t width, uint32_t height,
                              uint32_t iterations, float edge_k, float normal_k, float plane_k, uint32_t flags /* reserved: 0 */, void* stream);
int rpt_denoise_guided(rpt_ctx* ctx, const float* pixels, const rpt_guide* guides, float* out, uint32_t width, uint32_t height,
                       uint32_t iterations, float edge_k, float normal_k, float plane_k, uint32_t flags);                                   /* host memory, blocks */

/* ---- temporal accumulation — PROJECT-DEFINED -------------------------------------------------------------------------------------------
 * Carries samples from one redraw to the next while the camera (or the geometry) moves.  A ColorBuffer's running mean is valid only
 * while the camera stands still; this step reprojects each pixel's first hit (its rpt_guide of "guided denoiser") into the PREVIOUS
 * frame, fetches the previous frame's accumulated colour where the previous guides say the same surface was seen, blends the new frame
 * into it, and carries a per-pixel sample count and the first two moments of luminance in an rpt_history record.  No scene is needed:
 * the result is a function of the pixels, the two sets of guides, the previous history and the two cameras alone.  The caller keeps
 * two history buffers and two guide buffers and swaps them every frame.
 *
 * Every operation is f32, rounded once, in this order; dot(a, b) = fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)); every quotient is the IEEE
 * one; min(a, b) = a < b ? a : b; W = (float)width, H = (float)height.
 *
 * Host part, once per call.
 *   From prev_camera, exactly as a render prepares a camera for (prev_camera, width, height) (camera/pinhole.rs:38-54; nothing fused):
 *     half_width = tan(to_radians(fov_deg) * 0.5)  (the strict tan);  half_height = half_width / (W / H);  o = origin;
 *     w = (origin - center) / |origin - center|, the length sqrt(x*x + y*y + z*z) summed left to right, three quotients;
 *     u = cross((0, 1, 0), w);  v = cross(w, u)  (cross(a, b).x = a.y*b.z - a.z*b.y, ...).
 *   Then gx = 0.5f / (half_width * dot(u, u)) and gy = 0.5f / (half_height * dot(v, v)).  (The reference's camera does not normalise u
 *   and v: both have the length sqrt(w.x^2 + w.z^2), which is 1 only for a camera that looks horizontally.  A ray through the screen
 *   point (sx, sy) is u*half_width*(2 sx - 1) + v*half_height*(2 sy - 1) - w, so its u coordinate over its depth is dot(u, u) times
 *   half_width*(2 sx - 1): the factor belongs in the inverse.)
 *   From camera: the frame-invariant part of a render's camera ray for (camera, width, height): rd0 = lower_left - origin, horizontal,
 *   vertical, psx = 1 / W, psy = 1 / H.
 *   IDENTITY mode: the two rpt_camera records are equal word for word and prev_positions is NULL.
 *
 * Per pixel (x, y), row 0 on top, i = y * width + x, g = guides[i]:
 *   1 what to reproject.  g.kind != RPT_HIT_NONE: src = prev_positions[i] (xyz) if given, else g.position; d = src - o.
 *     g.kind == RPT_HIT_NONE (the sky): d is the CURRENT camera's unnormalised ray direction through the pixel's centre, as
 *     rpt_camera_rays_device computes it before normalising: px = (float)x / W;  py = 1 - ((float)(y + 1) / H);
 *     s = psx * 0.5f + px;  t = psy * 0.5f + py;  d = (rd0 + horizontal * s) + vertical * t, per component.  The sky reprojects as a
 *     point at infinity: by the previous camera's orientation only.
 *   2 project.  lam = -dot(w, d); no history unless lam > 0.  a = dot(u, d) / lam;  b = dot(v, d) / lam;
 *     sx = fma(a, gx, 0.5f);  sy = fma(b, gy, 0.5f);  fx = fma(sx, W, -0.5f);  fy = fma(1 - sy, H, -0.5f)  — the inverse of the
 *     camera ray: row 0 on top, pixel centres at integers.  No history unless -1 < fx < W and -1 < fy < H (false for a NaN).
 *   3 taps.  x0 = floor(fx), wx = fx - x0, likewise y0, wy; taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in this order with the
 *     weights (1-wx)*(1-wy), wx*(1-wy), (1-wx)*wy, wx*wy.  In IDENTITY mode steps 2 and 3 are replaced by the single tap q = (x, y)
 *     with weight 1.
 *   4 a tap q is VALID when it lies inside the image; prev_history[q].n >= 1 and its rgb, m1 and m2 are all finite;
 *     prev_guides[q].key == g.key; and, for g.kind != RPT_HIT_NONE, dot(g.ns, prev_guides[q].ns) >= normal_min and
 *     fma(-(dpl*dpl), kx, 1) > 0 with r = prev_guides[q].position - src, dpl = dot(g.ng, r), kx = plane_k > 0 ? plane_k / dot(d, d) : 0.
 *     A NaN fails either test.  The distance from the pixel's tangent plane is measured relative to the distance from the previous
 *     camera, so plane_k is dimensionless as in "guided denoiser".
 *   5 history.  wsum = the sum of the valid taps' weights, from 0, in tap order; there is history when wsum > 0.  Each of r, g, b, n,
 *     m1, m2: acc = fma(value_q, weight_q, acc) over the valid taps in order, from 0; h = acc / wsum.
 *   6 blend.  c = the pixel's rgb; if any channel's exponent bits are all ones (NaN, +-inf) c is black, as in a render's blend.
 *     L = fma(0.2126f, c.r, fma(0.7152f, c.g, 0.0722f * c.b)).
 *     With history:    n' = min(n_h + 1, n_max);  al = 1 / n';  out = (1 - al) * h + c * al  (two products and one sum, nothing fused:
 *                      a render's blend); m1' likewise from m1_h and L, m2' from m2_h and L * L.
 *     Without history: n' = 1;  out = c;  m1' = L;  m2' = L * L.
 *     out.alpha = the pixel's alpha;  history[i] = {out.rgb, n', m1', m2', 0, 0}.
 * Consequences:
 *   - a static camera (IDENTITY) with n_max >= the number of frames gives the running mean of the frames in a render's blend order,
 *     bit for bit; max(m2 - m1*m1, 0) is the luminance variance of the samples behind a pixel;
 *   - once n' reaches n_max the mean becomes an exponential one with al = 1 / n_max;
 *   - a disoccluded pixel — no valid tap — starts again at n = 1, and so does one whose history holds a NaN or an infinity;
 *   - a tap of weight 0 (fx or fy an integer) is valid or not like any other and contributes nothing;
 *   - what a mirror shows is reprojected as if it were painted on the mirror: first-hit guides describe only the first surface, as in
 *     "guided denoiser"; shadows and highlights that move over a surface lag by about n_max frames.
 * n_max >= 1 and finite, -1 <= normal_min <= 1, plane_k >= 0 and finite (0 switches the plane test off), both cameras' fields finite
 * and origin != center, width and height 1..65535 (a tile row or column per workgroup index), flags reserved: 0.  prev_guides, prev_history and prev_camera all NULL: the first frame, no pixel has history
 * (prev_positions is then ignored).  Defaults that serve 1 spp per redraw: n_max 32, normal_min 0.9, plane_k 1000 (DESIGN.md has what
 * was tried).
 *
 * prev_positions (n x 4 f32, the fourth word ignored) says, per pixel, where the surface point seen there WAS in the previous frame, in
 * world space: for geometry that moves.  NULL: static geometry.  The library has no producer of it yet: a caller who moves meshes
 * gathers it from the rpt_hit records (mesh, triangle, u, v) and the previous vertices.
 *
 * Arguments and errors.  Every pointer 16-byte aligned and (the _device form) on the context's device; out and history must overlap no
 * input and not each other.  RPT_ERR_INVALID_ARG for a NULL ctx, a NULL pixels, guides, camera, out or history, some but not all of
 * prev_guides, prev_history and prev_camera NULL, a misaligned pointer, an argument out of the ranges above or a NaN, flags != 0, and
 * a width or height of zero or above 65535.  A rejected call writes nothing.  The _device form enqueues one kernel on `stream` and returns; it uses no
 * memory of the context.  The host form stages through device memory of the context and blocks.
 *
 * The kernels (csrc/k_tacc.hip, a code object library of their own) are three forms of one template — first frame, IDENTITY,
 * reprojecting — one pixel per lane on 32 x 8 tiles; a tap reads 32 of a guide's 64 bytes (position + key, ns + t) and the 32-byte
 * history record, everything as 16-byte loads and stores.  DESIGN.md ("temporal accumulation") has their registers and rates. */
typedef struct rpt_history {
    float rgb[3]; float n;                 /* the accumulated colour; the number of samples behind it, at most n_max */
    float m1, m2;                          /* the first and second moment of luminance */
    uint32_t reserved[2];                  /* written 0 */
} rpt_history;                             /* 32 B */

#if defined(__cplusplus)
static_assert(sizeof(rpt_history) == 32, "a history record is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(rpt_history) == 32, "a history record is 32 bytes");
#endif

int rpt_temporal_accumulate_device(rpt_ctx* ctx, const float* pixels_dev, const rpt_guide* guides_dev, const rpt_camera* camera,
                                   const rpt_guide* prev_guides_dev, const rpt_history* prev_history_dev, const rpt_camera* prev_camera,
                                   const float* prev_positions_dev /* n x 4 f32, or NULL */, float* out_dev, rpt_history* history_dev,
                                   uint32_t width, uint32_t height, float n_max, float normal_min, float plane_k, uint32_t flags /* reserved: 0 */,
                                   void* stream);
int rpt_temporal_accumulate(rpt_ctx* ctx, const float* pixels, const rpt_guide* guides, const rpt_camera* camera, const rpt_guide* prev_guides,
                            const rpt_history* prev_history, const rpt_camera* prev_camera, const float* prev_positions /* or NULL */, float* out,
                            rpt_history* history, uint32_t width, uint32_t height, float n_max, float normal_min, float plane_k,
                            uint32_t flags);                                                                                             /* host memory, blocks */

/* The same on HOST buffers (upload, convert, download; blocks): what ColorBuffer::convert_to_u8
 * does for a caller that owns a host ColorBuffer (buffer.rs:55-64, frame = width*height*4 bytes). */
int rpt_convert_to_u8(rpt_ctx* ctx, const float* pixels, uint8_t* frame, uint32_t width, uint32_t height);

int rpt_synchronize(rpt_ctx* ctx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RPT_H */
