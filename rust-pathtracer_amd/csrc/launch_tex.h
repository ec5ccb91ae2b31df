// launch_tex.h — the seam between capi.hip and the kernels of mesh textures (k_tex.hip, a code object library of its own: build.py,
// tex_lib_of).  A header of its own beside launch_light.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_tex.h"
#include "launch_light.h"

namespace rptscene {

// A mesh scene some mesh of which is textured (include/rpt.h, "mesh textures"): the base form's tables — SceneMeshSmooth's (no mesh
// SMOOTH: all-zero smooth bits) or, while some mesh is ON, SceneMeshLight's — plus what the lookup at a hit reads.
template <class Base> struct SceneMeshTexT : Base {
    const rpthost::TexDesc* tex_desc;     // ordinal -> the textured mesh's image
    const uint32_t* tri_tex;              // flattened triangle -> its mesh's ordinal, or 0xFFFFFFFF
    const float* uvs;                     // st per concatenated vertex
    const rpthost::TexTexel* texels;      // every image's decoded texels, 16 B each
};
using SceneMeshTex = SceneMeshTexT<SceneMeshSmooth>;
using SceneMeshLightTex = SceneMeshTexT<SceneMeshLight>;

}  // namespace rptscene

namespace rptlaunch {

// One image: L[0 .. 255] of `gamma` into `table` (256 floats of device scratch), then one lane per texel: `bytes` (RGBA8, device) ->
// `out`.  Two launches.
hipError_t tex_decode(const uint8_t* bytes, float* table, rpthost::TexTexel* out, uint32_t n_texels, float gamma, hipStream_t st);
// mesh_regen_kernel's body over a SceneMeshTex / a SceneMeshLightTex
hipError_t render_mesh_tex(const rptscene::SceneMeshTex& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_light_tex(const rptscene::SceneMeshLightTex& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_texture_query (include/rpt_test.h): per ray {the winning triangle's flattened index or 0xFFFFFFFF, mat.rgb's bits}
hipError_t mesh_texture_query(const rptscene::SceneMeshTex& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
