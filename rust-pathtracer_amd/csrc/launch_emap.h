// launch_emap.h — the seam between capi.hip and the kernels of mesh emission maps (k_emap.hip, a code object library of its own:
// build.py, emap_lib_of).  A header of its own beside launch_mmap.h: the other kernel translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_scene.h"
#include "host_emap.h"
#include "launch_mmap.h"

namespace rptscene {

// A mesh scene some mesh of which has an emission map ON (include/rpt.h, "mesh emission maps"): any of the eight material-mapped
// forms (no material map ON: an all-zero descriptor table, lent by the emission map's own allocation) plus what the lookups read.
template <class Base> struct SceneMeshEmitT : Base {
    const rpthost::EmapDesc* emit_desc;         // texture ordinal -> the mesh's map (flags 0: none): the hit side and the emitter exit
    const rpthost::EmapDesc* emit_light_desc;   // light ordinal -> the mesh's map (flags 0: none): the sampler
    const float4* emit_texels;                  // every map's decoded texels {r, g, b, 0}, 16 B each
};
using SceneMeshEmit = SceneMeshEmitT<SceneMeshMap>;
using SceneMeshEmitEnv = SceneMeshEmitT<SceneMeshMapEnv>;
using SceneMeshEmitCut = SceneMeshEmitT<SceneMeshMapCut>;
using SceneMeshEmitCutEnv = SceneMeshEmitT<SceneMeshMapCutEnv>;
using SceneMeshEmitNrm = SceneMeshEmitT<SceneMeshMapNrm>;
using SceneMeshEmitNrmEnv = SceneMeshEmitT<SceneMeshMapNrmEnv>;
using SceneMeshEmitNrmCut = SceneMeshEmitT<SceneMeshMapNrmCut>;
using SceneMeshEmitNrmCutEnv = SceneMeshEmitT<SceneMeshMapNrmCutEnv>;

}  // namespace rptscene

namespace rptlaunch {

// mesh_regen_kernel's body over the eight emission-mapped forms.  (The decode is "mesh textures"' own launch: launch_tex.h, tex_decode.)
hipError_t render_mesh_emit(const rptscene::SceneMeshEmit& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_env(const rptscene::SceneMeshEmitEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_cut(const rptscene::SceneMeshEmitCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_cut_env(const rptscene::SceneMeshEmitCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_nrm(const rptscene::SceneMeshEmitNrm& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_nrm_env(const rptscene::SceneMeshEmitNrmEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_nrm_cut(const rptscene::SceneMeshEmitNrmCut& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
hipError_t render_mesh_emit_nrm_cut_env(const rptscene::SceneMeshEmitNrmCutEnv& sc, const rptscene::RenderParams& rp, uint32_t nblocks, hipStream_t st);
// rpt_debug_mesh_emission_map_query (include/rpt_test.h): per ray {the winning triangle's flattened index or 0xFFFFFFFF, the bits of
// hit_material's mat.emission, the bits of the emitter exit's emission}
hipError_t mesh_emission_map_query(const rptscene::SceneMeshEmit& sc, const float* rays, uint32_t* out, uint64_t n, uint32_t flags, hipStream_t st);
// rpt_debug_mesh_emission_map_sample (include/rpt_test.h): per record {k, the bits of emission, of direction and of pdf}
hipError_t mesh_emission_map_sample(const rptscene::SceneMeshEmit& sc, const float* in, uint32_t* out, uint64_t n, hipStream_t st);

}  // namespace rptlaunch
