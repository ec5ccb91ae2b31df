// launch_build.h — the seam between capi.hip and the hierarchy build of rpt_rebuild_meshes (k_build.hip, a code object library of its
// own: build.py, build_lib_of).  A header of its own beside launch.h: the kernel translation units that include launch.h do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rptlaunch {

// Device pointers of one build: the scene's triangle rows, the NEW node table, the refit's tables (host_refit.h, RefitLayout) and the
// build's own (host_build.h, BuildLayout).
struct BuildTables {
    uint32_t n_slots = 0, max_nodes = 0;
    float4* tris = nullptr;
    float4* nodes = nullptr;          // max_nodes nodes
    const float* slot_box = nullptr;
    uint32_t* slot_vertex = nullptr;
    uint32_t* level_nodes = nullptr;  // max_nodes entries
    uint64_t* keys_in = nullptr;
    uint64_t* keys_out = nullptr;
    uint32_t* vals_in = nullptr;
    uint32_t* vals_out = nullptr;
    uint32_t* gather = nullptr;       // [6][n_slots]
    uint2* range = nullptr;           // max_nodes
    uint32_t* mid = nullptr;          // max_nodes
    uint32_t* flags = nullptr;        // 2 per node of the widest level
    uint32_t* offsets = nullptr;
    uint32_t* levels = nullptr;       // host_build.h, kBuildLevelWords
    uint32_t* bounds = nullptr;       // 6
    void* temp = nullptr;             // rocPRIM's temporary storage: build_temp_bytes(n_slots)
    size_t temp_bytes = 0;
};

// the most temporary storage the sort of n_slots keys and the levels' prefix sums ask for (their query calls; no device is touched)
hipError_t build_temp_bytes(uint32_t n_slots, size_t* bytes);
// the new slot order: keys from the slots' boxes, the sort, the rows' .w words and the vertex indices permuted (the caller then
// runs refit_triangles for the rows and boxes in the new order)
hipError_t build_order(const BuildTables& t, hipStream_t st);
// the new shape over the sorted keys: child words into t.nodes, the levels' first nodes and counts and the status into t.levels
hipError_t build_shape(const BuildTables& t, uint32_t leaf_target, hipStream_t st);

}  // namespace rptlaunch
