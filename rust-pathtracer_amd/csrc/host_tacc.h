// host_tacc.h — the host part of temporal accumulation (include/rpt.h, "temporal accumulation"): the previous camera's origin, basis
// and screen scales, the current camera's frame-invariant part, and the form.  Plain C++ (compiled with -ffp-contract=off like
// everything else); the basis repeats make_camera's operations (host_scene.h), which returns only what a camera ray needs of them.
#pragma once

#include <cmath>
#include <cstring>

#include "host_scene.h"
#include "launch_tacc.h"

namespace rpthost {

inline bool tacc_camera_ok(const rpt_camera& c)
{
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(c.origin[k]) || !std::isfinite(c.center[k])) return false;
    if (!std::isfinite(c.fov_deg)) return false;
    return c.origin[0] != c.center[0] || c.origin[1] != c.center[1] || c.origin[2] != c.center[2];
}

// o, u, v, w, gx, gy of `prev` for a width x height image.
inline void tacc_prev_camera(const rpt_camera& prev, float width, float height, rptscene::TaccArgs& a)
{
    const float ratio = width / height;
    const float half_width = rpt_tanf((prev.fov_deg * (3.14159265358979323846f / 180.0f)) * 0.5f);
    const float half_height = half_width / ratio;
    float w[3] = {prev.origin[0] - prev.center[0], prev.origin[1] - prev.center[1], prev.origin[2] - prev.center[2]};
    const float wl = __builtin_sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int k = 0; k < 3; ++k) w[k] = w[k] / wl;
    const float up[3] = {0.0f, 1.0f, 0.0f};
    const float u[3] = {up[1] * w[2] - up[2] * w[1], up[2] * w[0] - up[0] * w[2], up[0] * w[1] - up[1] * w[0]};
    const float v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};
    const auto dot = [](const float* p, const float* q) { return __builtin_fmaf(p[0], q[0], __builtin_fmaf(p[1], q[1], p[2] * q[2])); };
    for (int k = 0; k < 3; ++k) { a.o[k] = prev.origin[k]; a.u[k] = u[k]; a.v[k] = v[k]; a.w[k] = w[k]; }
    a.gx = 0.5f / (half_width * dot(u, u));
    a.gy = 0.5f / (half_height * dot(v, v));
}

// Everything the kernel takes beside its buffers, and its form.  `prev` NULL: the first frame.
inline rptscene::TaccForm tacc_args(const rpt_camera& cam, const rpt_camera* prev, bool has_prev_positions, uint32_t width, uint32_t height, float n_max,
                                    float normal_min, float plane_k, rptscene::TaccArgs& a)
{
    std::memset(&a, 0, sizeof(a));
    a.cam = make_camera(cam, (float)width, (float)height);
    a.n_max = n_max; a.normal_min = normal_min; a.plane_k = plane_k;
    a.width = width; a.height = height;
    if (!prev) return rptscene::kTaccFirst;
    tacc_prev_camera(*prev, (float)width, (float)height, a);
    const bool same = std::memcmp(&cam, prev, sizeof(rpt_camera)) == 0;
    return same && !has_prev_positions ? rptscene::kTaccIdentity : rptscene::kTaccReproject;
}

}  // namespace rpthost
