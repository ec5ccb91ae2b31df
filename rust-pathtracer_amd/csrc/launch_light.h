// launch_light.h — the seam between capi.hip and the kernels of mesh lights (k_light.hip, a code object library of its own: build.py,
// light_lib_of).  A header of its own beside launch_smooth.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "launch_smooth.h"

namespace rptscene {

// One ON mesh (include/rpt.h, "mesh lights"), 32 B: host_light.h's kLightDescWords words.
struct LightMeshDesc {
    uint32_t first;                   // its first face: the base of its CDF and of its rows of face_vertex
    uint32_t n;                       // its triangles
    uint32_t material;                // rpt_mesh.material
    float area;                       // A_tot; 0: the mesh is dark
    int32_t exponent;                 // E
    uint32_t a_max;                   // the bits of A_max (the table kernels' scratch)
    uint32_t pad[2];
};

// What the table kernels read and write, on one device (host_light.h, LightLayout).
struct LightTables {
    LightMeshDesc* desc;              // per ON mesh
    uint64_t* cdf;                    // per face: C_k
    uint64_t* part;                   // per face: the scan's partial sums (scratch)
    uint64_t* block;                  // per 256 faces: the scan's block sums (scratch)
    float* area;                      // per face: A_k (scratch)
    const uint32_t* face_vertex;      // [3][n_faces]: face -> its corners in the concatenated vertex array
    const uint32_t* face_mesh;        // face -> its ON mesh's ordinal
    uint32_t n_on, n_faces;
};

// A mesh scene some mesh of which is ON: the smooth form's tables (no mesh SMOOTH: all-zero smooth bits, so every hit takes the flat
// normal) plus what the sampler and the hit side read.  n_lights_f is (float)n_pick here: include/rpt.h, "pickable lights".
struct SceneMeshLight : SceneMeshSmooth {
    const float* vertices;            // xyz per concatenated vertex: the positions the context holds (host_refit.h: the refit's table)
    const uint32_t* face_vertex;      // as LightTables
    const LightMeshDesc* light_desc;  // ordinal -> the ON mesh
    const uint64_t* light_cdf;
    const uint32_t* tri_light;        // flattened triangle -> its mesh's ordinal, or 0xFFFFFFFF
    uint32_t n_faces;
    uint32_t n_pick;                  // N = n_lights + the number of ON meshes
};

}  // namespace rptscene

namespace rptlaunch {

// The tables of every ON mesh from the positions in `vertices`, five launches whatever the number of meshes: reset, areas and their
// maxima, quantise and scan within 256 faces, scan the block sums, CDF and A_tot.
hipError_t light_tables(const float* vertices, const rptscene::LightTables& t, hipStream_t st);
// mesh_regen_kernel's body over a SceneMeshLight
hipError_t render_mesh_light(const rptscene::SceneMeshLight& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_light_sample (include/rpt_test.h)
hipError_t mesh_light_sample(const rptscene::SceneMeshLight& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st);

}  // namespace rptlaunch
