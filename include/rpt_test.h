/* rpt_test.h — TEST HOOKS of the MI355X-native path-tracing integrator.  NOT part of the drop-in surface (include/rpt.h) and NOT
 * exported by the shipped library: librpt_hip_test.so — the same objects, linked with these entry points and the probe kernels
 * (python rust-pathtracer_amd/build.py builds both) — exports them, and rpt_build_has_test_hooks() tells which library is loaded.
 * The parity tests use them to localise a frame mismatch to one function. */
#ifndef RPT_TEST_H
#define RPT_TEST_H

#include "rpt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- probes ------------------------------------------------------------------
 * Evaluate one device function over arrays (device pointers), so tests can compare
 * leaf functions with the oracle bit for bit.  */
enum {
    RPT_PROBE_SIN = 0, RPT_PROBE_COS = 1, RPT_PROBE_LOG2 = 2, RPT_PROBE_POW = 3,
    RPT_PROBE_DIV = 4, RPT_PROBE_SQRT = 5, RPT_PROBE_RNG = 6, RPT_PROBE_EXP = 7, RPT_PROBE_LOG = 8,
    RPT_PROBE_DIV3 = 9,               /* three quotients by one denominator, the library's shared-reciprocal form: see dev_math.h */
    /* OR'ed into `fn`: the same function from the relaxed-arithmetic build (RPT_RENDER_FAST_MATH's: hipcc's fast divide / sqrt,
     * FMA contraction; k_probes.hip built a second time with those flags) instead of the strict one */
    RPT_PROBE_RELAXED = 1u << 8
};
int rpt_probe_math(rpt_ctx* ctx, uint32_t fn, const float* a_dev, const float* b_dev,
                   float* out_dev, uint64_t n, void* stream);

/* One integrator function per record, for tests that localise a frame mismatch: records are RPT_PROBE_IN_STRIDE floats
 * in, RPT_PROBE_OUT_STRIDE floats out (u32 values as their bit patterns), device pointers.  Layouts (in -> out):
 *   GEN_RAY        {px, py, offx, offy}; camera = the uploaded scene's, params = {width, height} (host)
 *                  -> {origin[3], direction[3]}                                      camera/pinhole.rs:38-60
 *   HIT_SPHERE     {o[3], d[3], centre[3], radius} -> {hit, t}                       analytical.rs:166-190
 *   HIT_PLANE      {o[3], d[3], normal[3], point[3], min_denom, max_t} -> {hit, t}   analytical.rs:193-204
 *   SAMPLE_LIGHT   {type, position[3], emission[3], radius, area, u[3], v[3], scatter_pos[3], n_lights, scene flags,
 *                   rng state, rng increment, -} -> {normal[3], emission[3], direction[3], dist, pdf, draws}   tracer.rs:173-220
 *   DISNEY_EVAL    {material: rgb[3], emission[3], anisotropic, metallic, roughness, subsurface, specular_tint, sheen,
 *                   sheen_tint, clearcoat, clearcoat_gloss, spec_trans, ior (before finalize), eta, v[3], n[3], l[3]}
 *                  -> {f[3], pdf}                                                    tracer.rs:555-626
 *   DISNEY_SAMPLE  {material (17), eta, v[3], n[3], l_stale[3], rng state, rng increment, -}
 *                  -> {f[3], l[3], pdf, draws}                                       tracer.rs:441-553            */
enum {
    RPT_PROBE_FN_GEN_RAY = 0, RPT_PROBE_FN_HIT_SPHERE = 1, RPT_PROBE_FN_HIT_PLANE = 2, RPT_PROBE_FN_SAMPLE_LIGHT = 3,
    RPT_PROBE_FN_DISNEY_EVAL = 4, RPT_PROBE_FN_DISNEY_SAMPLE = 5, RPT_PROBE_FN_COUNT = 6
};
#define RPT_PROBE_IN_STRIDE 32
#define RPT_PROBE_OUT_STRIDE 16
int rpt_probe_fn(rpt_ctx* ctx, uint32_t fn, const float* in_dev, float* out_dev, uint64_t n, const float* params, void* stream);

/* Ray queries against the uploaded LARGE scene's spheres, for testing the acceleration structure:
 * rays_dev = n x {origin[3], direction[3], max_dist}; out_dev = n x {t (f32 bits), nearest sphere index
 * or 0xFFFFFFFF, any_hit (0/1) with max_dist honoured}.  use_grid = 0 forces the brute-force loops. */
int rpt_probe_rays(rpt_ctx* ctx, const float* rays_dev, uint32_t* out_dev, uint64_t n, uint32_t use_grid, void* stream);

/* Ray queries against the uploaded MESH scene's triangles (include/rpt.h, "triangle meshes"), through the device functions the mesh
 * kernel calls: rays_dev = n x {origin[3], direction[3], max_dist}; out_dev = n x {t (f32 bits; +inf's bits when nothing is hit), the
 * nearest triangle's flattened index or 0xFFFFFFFF, any_hit (0/1)} — closest over the triangles alone, from dist = F::MAX; any_hit
 * with max_dist honoured when `flags` bit 0 is set.  `flags` bit 1: the ordered loop over every triangle instead of the BVH.
 * RPT_ERR_NO_SCENE unless the uploaded scene has meshes. */
enum { RPT_MESH_QUERY_USE_MAX = 1u << 0, RPT_MESH_QUERY_BRUTE = 1u << 1 };
int rpt_debug_mesh_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The normal a winning triangle is shaded with (include/rpt.h, "smooth mesh shading"), through the hit_normal the smooth scenes' render
 * kernel calls: rays_dev as for rpt_debug_mesh_query (max_dist is not read); out_dev = n x 4 dwords {the nearest triangle's flattened
 * index or 0xFFFFFFFF, the normal's three words (zeros when nothing is hit)}.  `flags`: RPT_MESH_QUERY_BRUTE or 0.
 * RPT_ERR_NO_SCENE unless the uploaded scene has meshes; RPT_ERR_INVALID_ARG while no mesh is SMOOTH (that kernel does not run then). */
int rpt_debug_mesh_normal_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The sampler of mesh lights (include/rpt.h, "mesh lights"), through the device function the mesh light scenes' render kernel calls:
 * in_dev = n x 8 floats {scatter_pos[3], r0a, r0b, r1, r2, the ON mesh's ordinal (ascending mesh index) as the bits of an f32};
 * out_dev = n x 9 dwords {the picked triangle's index within the mesh or 0xFFFFFFFF (a dark mesh, an ordinal out of range: the rest
 * are LightSampleRec::new()'s zeros), direction[3], normal[3], dist, pdf, as bits}.  The draws are taken as given: multiples of 2^-24
 * in [0, 1) are what the kernel's own draws are.  RPT_ERR_NO_SCENE unless the uploaded scene has meshes; RPT_ERR_INVALID_ARG while
 * no mesh is ON (that kernel does not run then). */
int rpt_debug_mesh_light_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream);

/* The base colour a winning triangle is shaded with (include/rpt.h, "mesh textures"), through the hit_material the textured scenes'
 * render kernels call: rays_dev as for rpt_debug_mesh_query (max_dist is not read); out_dev = n x 4 dwords {the nearest triangle's
 * flattened index or 0xFFFFFFFF, the three words of mat.rgb (zeros when nothing is hit)}.  `flags`: RPT_MESH_QUERY_BRUTE or 0.
 * RPT_ERR_NO_SCENE unless the uploaded scene has meshes; RPT_ERR_INVALID_ARG while no mesh is textured (those kernels do not run then). */
int rpt_debug_mesh_texture_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The walks of a scene some mesh of which has a cutout ON (include/rpt.h, "mesh cutouts"), through the device functions the cutout
 * scenes' render kernels call: rays_dev, out_dev and `flags` exactly as for rpt_debug_mesh_query — per ray {t's bits or +inf's, the
 * winning triangle's flattened index or 0xFFFFFFFF, any_hit}, over the triangles that pass the cut test, through the hierarchy or
 * (RPT_MESH_QUERY_BRUTE) the ordered loop.  RPT_ERR_NO_SCENE unless the uploaded scene has meshes; RPT_ERR_INVALID_ARG while no
 * cutout is ON (those kernels do not run then). */
int rpt_debug_mesh_cutout_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The normal a winning triangle is shaded with in a scene some mesh of which has a normal map ON (include/rpt.h, "mesh normal
 * maps"), through the hit_normal the normal-mapped scenes' render kernels call (the form over the textured mesh-light tables):
 * rays_dev, out_dev and `flags` exactly as for rpt_debug_mesh_normal_query — per ray {the winning triangle's flattened index or
 * 0xFFFFFFFF, the normal's three words (zeros when nothing is hit)}, RPT_MESH_QUERY_BRUTE or 0.  RPT_ERR_NO_SCENE unless the uploaded
 * scene has meshes; RPT_ERR_INVALID_ARG while no map is ON (those kernels do not run then). */
int rpt_debug_mesh_normal_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The roughness and metallic a winning triangle is shaded with in a scene some mesh of which has a material map ON (include/rpt.h,
 * "mesh material maps"), through the hit_material the material-mapped scenes' render kernels call (the form over the textured
 * mesh-light tables), before the max(roughness, 0.01) every material gets: rays_dev, out_dev and `flags` exactly as for
 * rpt_debug_mesh_normal_map_query — per ray {the winning triangle's flattened index or 0xFFFFFFFF, mat.roughness' bits,
 * mat.metallic's bits, 0} (zeros when nothing is hit), RPT_MESH_QUERY_BRUTE or 0.  RPT_ERR_NO_SCENE unless the uploaded scene has
 * meshes; RPT_ERR_INVALID_ARG while no map is ON (those kernels do not run then). */
int rpt_debug_mesh_material_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The emission a winning triangle is shaded with in a scene some mesh of which has an emission map ON (include/rpt.h, "mesh emission
 * maps"), through the hit_material and the emitter exit's hit_emission_at the emission-mapped scenes' render kernels call (the form
 * over the textured mesh-light tables): rays_dev and `flags` exactly as for rpt_debug_mesh_material_map_query; out_dev = n x 7 dwords
 * — per ray {the winning triangle's flattened index or 0xFFFFFFFF, the three words of mat.emission, the three words of the emitter
 * exit's emission} (zeros when nothing is hit).  RPT_ERR_NO_SCENE unless the uploaded scene has meshes; RPT_ERR_INVALID_ARG while no
 * map is ON (those kernels do not run then). */
int rpt_debug_mesh_emission_map_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* The mesh-light sampler of such a scene, through the function its render kernels' mesh_light_nee calls: in_dev exactly as for
 * rpt_debug_mesh_light_sample — n x 8 floats {scatter_pos, r0a, r0b, r1, r2, the ON mesh's ordinal as bits}; out_dev = n x 8 dwords
 * {k (0xFFFFFFFF: a dark mesh or an ordinal out of range), the three words of emission, the three words of direction, pdf's bits}.
 * RPT_ERR_INVALID_ARG while no map is ON or no mesh is ON. */
int rpt_debug_mesh_emission_map_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream);

/* The join of meshes and media (include/rpt.h, "mesh media"), through the closest walk and the hit_medium_index, medium_at and
 * medium_side_normal the media scenes' render kernels call (the form over the textured mesh-light tables), one ray per lane: rays_dev
 * = n x 9 floats {o, d, l}; out_dev = n x 4 dwords — per ray {the winning triangle's flattened index or 0xFFFFFFFF, its mesh's
 * medium ordinal or 0xFFFF (none), the bits of dot(l, G) with G the winning triangle's flat normal (0 when nothing is hit),
 * in_medium after step 4 started from false}; `flags`: RPT_MESH_QUERY_BRUTE or 0.  RPT_ERR_NO_SCENE unless the uploaded scene has
 * meshes; RPT_ERR_INVALID_ARG while no mesh carries a medium (those kernels do not run then). */
int rpt_debug_mesh_media_query(rpt_ctx* ctx, const float* rays_dev, uint64_t n, uint32_t* out_dev, uint32_t flags, void* stream);

/* Which mesh render form the context's first device's last launch took: 0 .. 11 the twelve forms of csrc/mesh_args.h in MeshForm's
 * order (nrm_cut_env, nrm_cut, nrm_env, nrm, cut_env, cut, env, light_tex, tex, light, smooth, flat), 12 .. 19 a material map over
 * the eight textured forms that hold every table (csrc/mesh_args_mmap.h: light_tex, env, cut, cut_env, nrm, nrm_env, nrm_cut,
 * nrm_cut_env), 20 .. 27 an emission map over those eight in the same order (csrc/mesh_args_emap.h), with or without a material
 * map, 28 .. 35 a medium over those eight in the same order (csrc/mesh_args_med.h: some mesh carries a medium; bit 24 of
 * rpt_debug_kernel_choice, the media form, is set as well); 0xFFFFFFFF when that launch was no mesh scene's or there was none.  rpt_debug_kernel_choice has no bit left for material or
 * emission maps and keeps its meaning: bits 26-31 say which of the other features are present. */
int rpt_debug_mesh_form(rpt_ctx* ctx, uint32_t* form);

/* The lookup of the environment (include/rpt.h, "environment lighting"), through the device function the miss exit of the environment
 * scenes' render kernel calls: dirs_dev = n x 3 floats, one direction each (taken as given: not normalised); out_dev = n x 5 dwords
 * {the texel k or 0xFFFFFFFF, the radiance's three words, lp as bits: the pdf the sampler has for that direction, 0 where the miss
 * weight is 1 whatever the bounce (BACKGROUND_ONLY, a dark table, q_k == 0, no texel)}.  RPT_ERR_NO_SCENE unless the uploaded scene has
 * meshes; RPT_ERR_INVALID_ARG while no environment is set (that kernel does not run then). */
int rpt_debug_env_query(rpt_ctx* ctx, const float* dirs_dev, uint64_t n, uint32_t* out_dev, void* stream);

/* The sampler of the environment, through the device function that kernel's direct_light calls: in_dev = n x 7 floats {scatter_pos[3]
 * (not read: the light is at infinity), r0a, r0b, r1, r2}; out_dev = n x 8 dwords {the picked texel k or 0xFFFFFFFF (not SAMPLED, or a
 * dark table: the rest are LightSampleRec::new()'s zeros), direction[3], pdf, emission[3], as bits}.  Errors as rpt_debug_env_query. */
int rpt_debug_env_sample(rpt_ctx* ctx, const float* in_dev, uint64_t n, uint32_t* out_dev, void* stream);

/* The uploaded mesh scene's hierarchy (csrc/host_bvh.h): its interior nodes, the depth of its deepest leaf, and the host time its build
 * took in rpt_upload_scene — after rpt_rebuild_meshes the rebuilt hierarchy's, and the wall time of that call's device part.
 * RPT_ERR_NO_SCENE unless the uploaded scene has meshes.  (tools/mesh_bench.py) */
int rpt_debug_mesh_stats(rpt_ctx* ctx, uint32_t* n_nodes, uint32_t* depth, float* build_ms);

/* On how many of the context's devices the hierarchy's walk serves the uploaded mesh scene's rays: all of them, or — while a coordinate
 * some triangle uses lies beyond 2^60 (include/rpt.h, "triangle meshes") — none: the ordered loop serves them.  RPT_ERR_NO_SCENE
 * unless the uploaded scene has meshes. */
int rpt_debug_mesh_walk(rpt_ctx* ctx, uint32_t* walk);

/* Copy the uploaded mesh scene's triangle rows (which = 0: 48 B per triangle, in leaf order) or hierarchy nodes (which = 1: 64 B each,
 * csrc/host_bvh.h BvhNode) from the context's first device to the host, as rpt_update_meshes / rpt_rebuild_meshes (include/rpt.h) left them.  *bytes = the
 * table's size; RPT_ERR_INVALID_ARG when `out` is NULL or holds fewer than that (*bytes is still set).  RPT_ERR_NO_SCENE unless the
 * uploaded scene has meshes.  Waits for the device. */
int rpt_debug_mesh_tables(rpt_ctx* ctx, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes);

/* Multi-device contexts, after rpt_render / rpt_resident_render: the time in ms from the moment device index `b` (position in
 * rpt_create_multi's list) BEGAN its part of the last render to the moment device index `a` ENDED its part (HIP events on their
 * streams).  Positive for a != b means the two overlapped: what the fan-out inside render() promises (tracer.rs:29-32).  Events
 * of two different physical devices cannot be compared (RPT_ERR_UNSUPPORTED): the probe is for virtual ranks, i.e. repeated
 * device ids.  Waits for both events. */
int rpt_debug_render_overlap_ms(rpt_ctx* ctx, int a, int b, float* ms);

/* What the last launch on the context's first device left for the next one's dispatch (rpt_set_dispatch): per tile of that launch
 * (16x16 pixels, row-major over the device's rows) out[tile * 4 + wave] = the time, in 10 ns, wave `wave` of the tile's last unit
 * held its slot, then from out[4 * n] the dispatch order (position -> tile: a permutation of 0 .. n - 1) and 5 * n more words of
 * development data (tools/dispatch_timeline.py).  `out` holds 10 * capacity_tiles dwords; *n_tiles = n.  Waits for the device. */
int rpt_debug_sched_read(rpt_ctx* ctx, uint32_t* out, uint32_t capacity_tiles, uint32_t* n_tiles);

/* Which instantiation of its kernel class the context's last render launch took on its first device (csrc/launch.h, KernelChoice):
 * bit 0 the table sizes known at compile time, bit 1 the material table (at most 3 primitives), bit 2 its 64-row form (4 primitives),
 * bit 3 the table by class of accepted set (5-12 primitives), bits 8-15 the number of classes then, bits 16-19 the SDF object's
 * compile-time primitive count, bit 20 the relaxed-arithmetic build (RPT_RENDER_FAST_MATH), bit 21 small scenes' compacting kernel
 * (else the class's megakernel), bit 22 its dense form (at most 3 072 workgroups), bit 23 the nested-loop kernel, bit 24 the class's
 * participating-media form (the scene has media: RPT_SCENE_MEDIA), bit 25 the mesh scene class's kernel (k_mesh.hip), bit 26 beside it its smooth-shading form (k_smooth.hip: some mesh is SMOOTH), bit 27 some mesh is ON (include/rpt.h, "mesh lights"): the kernel that ran is k_light.hip's, which serves flat and smooth meshes alike — with bit 26 set as well it is still that one kernel, shading the SMOOTH meshes through their per-triangle bit;
 * bit 28 some mesh is textured (include/rpt.h, "mesh textures"): the kernel that ran is one of k_tex.hip's two, the one over the mesh
 * lights' tables while bit 27 is set as well, else the one over the smooth scenes' tables; bit 29 an environment is set
 * (include/rpt.h, "environment lighting"): the kernel that ran is k_env.hip's one form, whatever bits 26-28 say.; bit 30 some mesh's
 * cutout is ON (include/rpt.h, "mesh cutouts"): the kernel that ran is one of k_cut.hip's two, the one over the environment form while
 * bit 29 is set as well, else the one over the textured mesh-light form; bit 31 some mesh's normal map is ON (include/rpt.h, "mesh
 * normal maps"): the kernel that ran is one of k_nrm.hip's four, picked by bits 30 and 29.  For tests that must know that the kernel they aim at is the one
 * that ran. */
int rpt_debug_kernel_choice(rpt_ctx* ctx, uint32_t* out);

/* Read the environment's knobs (csrc/knobs.h: the library reads them ONCE per process) again: for tests that change one between two
 * scenes or contexts of one process. */
int rpt_debug_reload_knobs(void);

#ifdef __cplusplus
}
#endif
#endif /* RPT_TEST_H */
