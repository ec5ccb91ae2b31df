// launch_tacc.h — the seam between capi.hip and the kernels of temporal accumulation (k_tacc.hip, a code object library of its own:
// build.py, tacc_lib_of).  A header of its own beside launch_gdn.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "../../include/rpt.h"

namespace rptscene {

// The host part of include/rpt.h ("temporal accumulation"): what the kernel takes beside its buffers.
struct TaccArgs {
    DevCamera cam;                              // the CURRENT camera's frame-invariant part (make_camera): the sky's direction
    float o[3], u[3], v[3], w[3];               // the PREVIOUS camera's origin and basis (tacc_prev_camera)
    float gx, gy;                               // 0.5 / (half_width * dot(u, u)), 0.5 / (half_height * dot(v, v))
    float n_max, normal_min, plane_k;
    uint32_t width, height;
};

enum TaccForm : uint32_t { kTaccFirst = 0u, kTaccIdentity = 1u, kTaccReproject = 2u };

}  // namespace rptscene

namespace rptlaunch {

// rpt_temporal_accumulate_device: one pixel per lane on 32 x 8 tiles.  kTaccFirst reads neither prev_* array (they may be NULL),
// kTaccIdentity requires prev_positions == NULL.  width, height > 0.
hipError_t tacc_accumulate(rptscene::TaccForm form, const rptscene::TaccArgs& args, const float* pixels, const rpt_guide* guides, const rpt_guide* prev_guides,
                           const rpt_history* prev_history, const float* prev_positions, float* out, rpt_history* history, hipStream_t st);

}  // namespace rptlaunch
