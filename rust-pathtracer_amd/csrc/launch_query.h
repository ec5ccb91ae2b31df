// launch_query.h — the seam between capi.hip and the kernels of ray queries (k_query.hip, a code object library of its own: build.py,
// query_lib_of).  A header of its own beside launch_emap.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_query.h"
#include "launch_emap.h"
#include "../../include/rpt.h"

namespace rptscene {

// What a query kernel takes beside its scene: the batch and the meshes' first-triangle offsets (host_query.h).
struct QueryArgs {
    const rpt_ray* rays;
    rpt_hit* hits;                              // the closest query
    rpt_surface* surfaces;                      // ... of a surface kernel
    uint8_t* occluded;                          // the occlusion query
    const uint32_t* tri_first;
    uint32_t n_meshes;
    uint64_t n;
};

}  // namespace rptscene

namespace rptlaunch {

// The closest hit without surfaces: over a scene without a cutout, and over one with (the walk tests the mask).
hipError_t query_closest(const rptscene::SceneMesh& sc, const rptscene::QueryArgs& q, hipStream_t st);
hipError_t query_closest_cut(const rptscene::SceneMeshCut& sc, const rptscene::QueryArgs& q, hipStream_t st);
// Occlusion, likewise.
hipError_t query_occluded(const rptscene::SceneMesh& sc, const rptscene::QueryArgs& q, hipStream_t st);
hipError_t query_occluded_cut(const rptscene::SceneMeshCut& sc, const rptscene::QueryArgs& q, hipStream_t st);
// The closest hit with its rpt_surface: normal map x cutout over the form that holds every table beneath them.
hipError_t query_surface(const rptscene::SceneMeshEmit& sc, const rptscene::QueryArgs& q, hipStream_t st);
hipError_t query_surface_cut(const rptscene::SceneMeshEmitCut& sc, const rptscene::QueryArgs& q, hipStream_t st);
hipError_t query_surface_nrm(const rptscene::SceneMeshEmitNrm& sc, const rptscene::QueryArgs& q, hipStream_t st);
hipError_t query_surface_nrm_cut(const rptscene::SceneMeshEmitNrmCut& sc, const rptscene::QueryArgs& q, hipStream_t st);
// rpt_camera_rays_device: width * height rays of `cam`, row 0 on top.
hipError_t query_camera_rays(const rptscene::DevCamera& cam, uint32_t width, uint32_t height, rpt_ray* rays, hipStream_t st);

}  // namespace rptlaunch
