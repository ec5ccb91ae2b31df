// host_query.h — the host side of ray queries (include/rpt.h, "ray queries"): the layout of the query's own device allocation and the
// lookup from a flattened triangle index to (mesh, triangle within the mesh).  Plain functions over plain words: k_query.hip compiles
// the lookup for the device, tests/query_harness.cpp runs it on the host (tests/test_query_host.py).
//
// The allocation holds what a surface kernel binds for a feature that is absent (mesh_args_query.h) and the meshes' first-triangle
// offsets.  Nothing in it depends on a setter or on a move: it is made at the first query after an upload and lives until the next.
//   tri_first   n_meshes + 1 words: mesh -> its first triangle in the flattened list (host_refit.h, RefitPlan::tri_first)
//   none        n_tris words of 0xFFFFFFFF: "no triangle belongs to an ON mesh" (tri_light), "... to a textured mesh" (tri_tex)
//   flat_bits   ceil(n_tris / 32) words of zero: "no triangle belongs to a SMOOTH mesh"
//   zero        n_meshes + 1 descriptors of kQueryDescBytes zero bytes: "no map on this texture ordinal" (MmapDesc / EmapDesc: flags 0)
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef RPT_QUERY_FN
#define RPT_QUERY_FN inline
#endif

namespace rpthost {

constexpr size_t kQueryDescBytes = 64;              // at least sizeof of every map descriptor (mesh_args_query.h asserts it)
constexpr uint32_t kQueryNone = 0xFFFFFFFFu;

struct QueryLayout {
    size_t off_tri_first, off_none, off_flat_bits, off_zero, total;
    QueryLayout(uint32_t n_meshes, uint32_t n_tris)
    {
        const auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
        off_tri_first = 0;
        off_none = up(off_tri_first + 4u * ((size_t)n_meshes + 1u));
        off_flat_bits = up(off_none + 4u * (size_t)n_tris);
        off_zero = up(off_flat_bits + 4u * (((size_t)n_tris + 31u) / 32u));
        total = up(off_zero + kQueryDescBytes * ((size_t)n_meshes + 1u));
    }
};

// The mesh that holds flattened triangle `index`: the last m with tri_first[m] <= index (meshes without triangles share their
// offset with the next one and are never the answer), or kQueryNone when index >= tri_first[n_meshes].  tri_first has
// n_meshes + 1 non-decreasing entries starting at 0.
RPT_QUERY_FN uint32_t query_mesh_of(const uint32_t* tri_first, uint32_t n_meshes, uint32_t index)
{
    if (n_meshes == 0u || index >= tri_first[n_meshes]) return kQueryNone;
    uint32_t lo = 0u, hi = n_meshes;                                // tri_first[lo] <= index < tri_first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tri_first[mid] <= index) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace rpthost
