// launch_mmap.h — the seam between capi.hip and the kernels of mesh material maps (k_mmap.hip, a code object library of its own:
// build.py, mmap_lib_of).  A header of its own beside launch_nrm.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_mmap.h"
#include "launch_nrm.h"

namespace rptscene {

// A mesh scene some mesh of which has a material map ON (include/rpt.h, "mesh material maps"): any of the eight textured forms that
// hold every table — the textured mesh-light one (no mesh ON: tri_light all 0xFFFFFFFF, lent by the map's own allocation), the
// environment's, either cutout form's, or one of the four normal-mapped forms — plus what the lookup at a hit reads.
template <class Base> struct SceneMeshMapT : Base {
    const rpthost::MmapDesc* map_desc;    // texture ordinal -> the mesh's map (flags 0: none)
    const float4* map_texels;             // every map's decoded texels {fr, fm, 0, 0}, 16 B each
};
using SceneMeshMap = SceneMeshMapT<SceneMeshLightTex>;
using SceneMeshMapEnv = SceneMeshMapT<SceneMeshEnv>;
using SceneMeshMapCut = SceneMeshMapT<SceneMeshCut>;
using SceneMeshMapCutEnv = SceneMeshMapT<SceneMeshCutEnv>;
using SceneMeshMapNrm = SceneMeshMapT<SceneMeshNrm>;
using SceneMeshMapNrmEnv = SceneMeshMapT<SceneMeshNrmEnv>;
using SceneMeshMapNrmCut = SceneMeshMapT<SceneMeshNrmCut>;
using SceneMeshMapNrmCutEnv = SceneMeshMapT<SceneMeshNrmCutEnv>;

}  // namespace rptscene

namespace rptlaunch {

// One map: `bytes` (RGBA8, device) -> `out`, one lane per texel: {c(roughness byte) or 1, c(metallic byte) or 1, 0, 0}.  One launch.
hipError_t mmap_decode(const uint8_t* bytes, rpthost::TexTexel* out, uint32_t n_texels, uint32_t roughness_channel, uint32_t metallic_channel, hipStream_t st);
// mesh_regen_kernel's body over the eight material-mapped forms
hipError_t render_mesh_map(const rptscene::SceneMeshMap& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_env(const rptscene::SceneMeshMapEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_cut(const rptscene::SceneMeshMapCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_cut_env(const rptscene::SceneMeshMapCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_nrm(const rptscene::SceneMeshMapNrm& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_nrm_env(const rptscene::SceneMeshMapNrmEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_nrm_cut(const rptscene::SceneMeshMapNrmCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_map_nrm_cut_env(const rptscene::SceneMeshMapNrmCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_material_map_query (include/rpt_test.h): per ray {the winning triangle's flattened index or 0xFFFFFFFF, the bits of
// mat.roughness and of mat.metallic, 0}
hipError_t mesh_material_map_query(const rptscene::SceneMeshMap& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);

}  // namespace rptlaunch
