// launch_gdn.h — the seam between capi.hip and the kernels of the guided denoiser (k_gdn.hip, a code object library of its own:
// build.py, gdn_lib_of).  A header of its own beside launch_query.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rpt.h"

namespace rptlaunch {

// rpt_denoise_guides_device: one rpt_guide per (ray, hit, surface) record.  n > 0, at most 0x7FFFFFFF workgroups of 256.
hipError_t gdn_pack(const rpt_ray* rays, const rpt_hit* hits, const rpt_surface* surfaces, uint64_t n, rpt_guide* guides, hipStream_t st);
// rpt_denoise_guided_device: `iterations` a-trous passes in -> out through `scratch` (each width * height * 4 f32; scratch is
// touched only when iterations > 1), every tap weighed by `guides` (width * height records).
hipError_t gdn_filter(const float* in, const rpt_guide* guides, float* out, float* scratch, uint32_t width, uint32_t height, uint32_t iterations,
                      float edge_k, float normal_k, float plane_k, hipStream_t st);

}  // namespace rptlaunch
