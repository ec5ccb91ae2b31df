// launch_smooth.h — the seam between capi.hip and the kernels of smooth mesh shading (k_smooth.hip, a code object library of its own:
// build.py, smooth_lib_of).  A header of its own beside launch.h, like launch_move.h: the kernel translation units that include
// launch.h do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"

namespace rptscene {

// A mesh scene some mesh of which is SMOOTH (include/rpt.h, "smooth mesh shading"): the mesh scene's tables — rows and nodes byte
// for byte what they are — plus what a smooth hit reads.
struct SceneMeshSmooth : SceneMesh {
    const uint32_t* slot_vertex;      // [3][n_tris]: slot -> its corners in the concatenated vertex array (host_refit.h: the refit's table)
    const float4* vnormals;           // concatenated vertex -> {its normal, 0}; (0, 0, 0) for the vertices of FLAT meshes
    const uint32_t* smooth_bits;      // one bit per flattened triangle index: its mesh is SMOOTH
};

}  // namespace rptscene

namespace rptlaunch {

// The normals of every SMOOTH mesh from the positions in `vertices` (xyz per concatenated vertex), one launch pair whatever the
// number of meshes: the face pass (face_vertex: [3][n_faces] -> face: 16 B per face), then the vertex pass over all n_vertices
// (adj_first / adj: host_smooth.h, SmoothPlan -> normals: 16 B per vertex).
hipError_t smooth_normals(const float* vertices, const uint32_t* face_vertex, float4* face, uint32_t n_faces, const uint32_t* adj_first,
                          const uint32_t* adj, float4* normals, uint32_t n_vertices, hipStream_t st);
// mesh_regen_kernel's body over a SceneMeshSmooth (k_mesh.hip, render_mesh)
hipError_t render_mesh_smooth(const rptscene::SceneMeshSmooth& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_normal_query (include/rpt_test.h): per ray {the winning triangle's flattened index or 0xFFFFFFFF, its normal's bits}
hipError_t mesh_normal_query(const rptscene::SceneMeshSmooth& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
