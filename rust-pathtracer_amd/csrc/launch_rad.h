// launch_rad.h — the seam between capi.hip and the kernels of radiance queries (k_rad.hip, a code object library of its own: build.py,
// rad_lib_of).  A header of its own beside launch_query.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_rad.h"
#include "launch_med.h"
#include "../../include/rpt.h"

namespace rptscene {

// What a radiance kernel takes beside its scene: the batch and one launch's share of the call's samples.
struct RadArgs {
    const rpt_ray* rays;
    float* out;                                 // n x 4 f32, a ColorBuffer pixel per ray: read, blended into, written
    uint64_t n;
    uint64_t frames_done;                       // of this launch: sample s is frame frames_done + s
    uint64_t seed;
    uint32_t spp;                               // <= kMaxSppPerLaunch
    uint32_t first_index;                       // ray i's stream is keyed by first_index + i (uint32: it wraps)
    uint32_t shade_threshold;                   // as RenderParams::shade_threshold
};

}  // namespace rptscene

namespace rptlaunch {

// The eight forms: normal map x cutout x environment over the media forms' scene types.
hipError_t radiance(const rptscene::SceneMeshMed& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_env(const rptscene::SceneMeshMedEnv& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_cut(const rptscene::SceneMeshMedCut& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_cut_env(const rptscene::SceneMeshMedCutEnv& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_nrm(const rptscene::SceneMeshMedNrm& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_nrm_env(const rptscene::SceneMeshMedNrmEnv& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_nrm_cut(const rptscene::SceneMeshMedNrmCut& sc, const rptscene::RadArgs& a, hipStream_t st);
hipError_t radiance_nrm_cut_env(const rptscene::SceneMeshMedNrmCutEnv& sc, const rptscene::RadArgs& a, hipStream_t st);
// rpt_camera_sample_rays_device: width * height rays of `cam`, row 0 on top, jittered by the two first draws of each pixel's stream
// under `fkey` = frame_key(seed, frame).
hipError_t radiance_camera_rays(const rptscene::DevCamera& cam, uint32_t width, uint32_t height, rptscene::FrameKey fkey, rpt_ray* rays, hipStream_t st);
// kMaxSppPerLaunch as the kernels were built with it
uint32_t radiance_max_spp();

}  // namespace rptlaunch
