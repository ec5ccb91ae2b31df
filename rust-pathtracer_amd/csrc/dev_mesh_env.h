// dev_mesh_env.h — environment lighting on the device (include/rpt.h, "environment lighting"): what a path that leaves the scene
// adds, and the sampler of the environment as one more pickable light, for SceneMeshEnvT only.  dev_integrator.h reaches both through
// `if constexpr (MeshEnv<S>::value)`: the other scene classes' kernels contain none of this.  The arithmetic is host_env.h's
// statement, compiled here for the device.  Included after dev_mesh_tex.h and launch_env.h, before regen_body.h.
#pragma once

namespace rptdev {

template <class Base> struct MeshLights<SceneMeshEnvT<Base>> { static constexpr bool value = true; };
template <class Base> struct MeshEnv<SceneMeshEnvT<Base>> { static constexpr bool value = true; };

// The lookup of direction d (host_env.h, env_lookup): the texel's index (0xFFFFFFFF: none), its radiance, and lp, the pdf the sampler
// has for this direction (0 where next-event estimation cannot produce it).
template <class S> RPT_DEV uint32_t mesh_env_lookup(const S& sc, v3 d, v3& radiance, float& lp)
{
    const float dir[3] = {d.x, d.y, d.z};
    float rad[3];
    const uint32_t k = rpthost::env_lookup(sc.env_texels, sc.env_size, sc.env_q, sc.env_q_f, sc.env_scale, dir, rad, &lp);
    radiance = mk3(rad[0], rad[1], rad[2]);
    return k;
}

// What the miss exit adds before the throughput: w * radiance(d) (include/rpt.h, "miss side").
template <class S> RPT_DEV v3 mesh_env_miss(const S& sc, const RayD& ray, const PathState& ps, uint32_t bounce)
{
    v3 radiance;
    float lp;
    (void)mesh_env_lookup(sc, ray.d, radiance, lp);
    float w = 1.0f;
    if (bounce != 0u && lp != 0.0f) w = power_heuristic(ps.scatter_pdf, lp);
    return w * radiance;
}

// Sampling the environment with the draws r0a, r0b, r1, r2 (host_env.h, env_sample).  Returns the picked texel (0xFFFFFFFF: the table
// is dark and `ls` keeps LightSampleRec::new()'s zeros).  The emission is the PICKED texel's, not a lookup of the rounded direction.
template <class S> RPT_DEV uint32_t mesh_env_sample(const S& sc, float r0a, float r0b, float r1, float r2, LightSample& ls)
{
    ls.normal = mk3(0.0f, 0.0f, 0.0f); ls.emission = mk3(0.0f, 0.0f, 0.0f); ls.direction = mk3(0.0f, 0.0f, 0.0f);
    ls.dist = 0.0f; ls.pdf = 0.0f;                                  // LightSampleRec::new, globals.rs:119-129
    float dir[3], em[3], pdf;
    const uint32_t k = rpthost::env_sample(sc.env_texels, sc.env_cdf, uniform_here(sc.env_size), sc.env_q, sc.env_q_f, sc.env_scale, sc.n_lights_f,
                                           r0a, r0b, r1, r2, dir, &pdf, em);
    if (k == rpthost::kEnvNone) return k;
    ls.direction = mk3(dir[0], dir[1], dir[2]);
    ls.normal = -ls.direction;
    ls.dist = __builtin_inff();
    ls.pdf = pdf;
    ls.emission = mk3(em[0], em[1], em[2]);
    return k;
}

// nee_sample's branch for the environment's index: the four draws, always, then the sampler.  Returns light.area (1: the MIS weight
// applies).
template <class S> RPT_DEV float mesh_env_nee(const S& sc, LightSample& ls, Rng& rng)
{
    const float r0a = rng.gen();
    const float r0b = rng.gen();
    const float r1 = rng.gen();
    const float r2 = rng.gen();
    (void)mesh_env_sample(sc, r0a, r0b, r1, r2, ls);
    return 1.0f;
}

}  // namespace rptdev
