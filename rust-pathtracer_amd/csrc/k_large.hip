// k_large.hip — scenes beyond the kernarg tables (BASELINE configs[4]: 10 k spheres, 16 lights): tables in HBM, uniform grid
// (dev_scene_large.h).  Built with the range tests next to every operation (kernel_common.h).
#include "kernel_common.h"

#include "regen_body.h"

// Large scenes: same schedule; the scene tables are streamed from HBM (dev_scene_large.h).  5 waves per SIMD: 96 VGPRs, 12 of them
// spilled (44 B of scratch per lane).  With the two tiers of cell lists 5 / 6 / 7 waves run at 1 881 / 1 874 / 1 858 Msamples/s (10 k
// spheres, 2048^2 x 32 spp) — and move 0.32 / 42 / 77 GB through HBM per launch: at 6 and 7 waves (80 / 72 VGPRs, 53 / 65 spilled) the
// resident waves' scratch no longer fits the L2s (profiles/r3/c5_megakernel vs c5_megakernel_7waves).  (Before the tiers 7 waves were
// 1.5 % ahead: 5: 1 660, 6: 1 664, 7: 1 689; round 2, hipcc's divide, 2048^2 x 8: 4: 1 165, 5: 1 387, 6: 1 454, 7: 1 372, 8: 1 200.)
#ifndef RPT_LARGE_WAVES_PER_SIMD
#define RPT_LARGE_WAVES_PER_SIMD 5
#endif
__global__ __launch_bounds__(256, RPT_LARGE_WAVES_PER_SIMD) void RPT_K(render_large_regen_kernel)(const SceneLarge sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
#ifndef RPT_RELAXED_BUILD
__global__ __launch_bounds__(256, RPT_LARGE_WAVES_PER_SIMD) void RPT_K(render_large_regen_media_kernel)(const WithMedia<SceneLarge> sc, const RenderParams rp) { render_regen_body_tf(sc, rp); }
#endif

namespace RPT_LAUNCH_NS {

#if defined(RPT_PROFILE_BLOCKS) && !defined(RPT_RELAXED_BUILD)
hipError_t prof_read_large(unsigned long long* out) { return prof_read(out); }
#endif

hipError_t render_large(const SceneLarge& scl, bool media, const RenderParams& rp, uint32_t nblocks, hipStream_t st)
{
    const dim3 tiles(nblocks), wg(256);
    (void)hipGetLastError();
#ifdef RPT_RELAXED_BUILD
    if (media) return hipErrorNotSupported;
#else
    if (media) hipLaunchKernelGGL(RPT_K(render_large_regen_media_kernel), tiles, wg, 0, st, WithMedia<SceneLarge>(scl), rp);
    else
#endif
    hipLaunchKernelGGL(RPT_K(render_large_regen_kernel), tiles, wg, 0, st, scl, rp);
    return hipGetLastError();
}

}  // namespace RPT_LAUNCH_NS
