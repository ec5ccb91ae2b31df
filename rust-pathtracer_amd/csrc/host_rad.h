// host_rad.h — the host side of radiance queries (include/rpt.h, "radiance queries"): the plan of the query's own device allocation,
// which of the eight forms a call takes, and how a call's samples are cut into launches.  Plain functions over plain words, no HIP
// type in them: capi.hip includes it, tests/rad_harness.cpp runs it on the host (tests/test_radiance_f64.py).
//
// The allocation.  The eight radiance forms sit over the media forms' scene types (launch_med.h), which hold every table a mesh scene
// can have.  A scene in which some mesh carries a medium binds the media's own allocation, exactly as its render does
// (mesh_args_med.h).  Every other scene binds this one: the media tables of a scene in which NO mesh carries a medium — a MedPlan
// with no medium ON and the MedLayout that goes with it (host_med.h): tri_medium all kMedNone, no row, and with them the empty
// emission-map block, its all-0xFFFFFFFF table and the all-zero smooth bits that mesh_args_med.h lends while those features are
// absent.  Nothing in it depends on a setter or on a move: it is made at the first radiance query after an upload and lives until
// the next.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "host_med.h"

namespace rpthost {

// The plan of the allocation over the scene of `plan`.
inline void build_rad_plan(const RefitPlan& plan, MedPlan& rad)
{
    build_med_plan(plan, std::vector<MedEntry>(), rad);
}

// One byte fill of the allocation (after the whole of it was zeroed): its offset, length and value.
struct RadFill {
    size_t off, bytes;
    int value;
};
// ... the empty emission-map block's (EmapLayout::fills, moved to where the block lies); tri_medium is copied from the plan.
inline std::vector<RadFill> rad_fills(const MedLayout& ml)
{
    std::vector<RadFill> out;
    for (const MapFill& f : ml.emap.fills())
        if (f.bytes && f.value) out.push_back(RadFill{ml.off_emap + f.off, f.bytes, f.value});
    return out;
}

// Which of the eight forms: the features that change a function's body.  (Everything else is data: a table that is bound or lent.)
enum : uint32_t { kRadEnv = 1u, kRadCut = 2u, kRadNrm = 4u, kRadForms = 8u };
inline uint32_t rad_form_of(bool normal_maps, bool cutouts, bool environment)
{
    return (normal_maps ? kRadNrm : 0u) | (cutouts ? kRadCut : 0u) | (environment ? kRadEnv : 0u);
}

// A call's `spp` samples from `frames_done` on as successive launches of at most `max_spp` each: launch k of rad_launches() starts at
// frames_done + k * max_spp and holds rad_launch_spp() samples.  The blends of one ray are sequential and a launch ends before the
// next begins (one stream), so the cut changes no word.
inline uint32_t rad_launches(uint32_t spp, uint32_t max_spp) { return spp / max_spp + (spp % max_spp ? 1u : 0u); }
inline uint32_t rad_launch_spp(uint32_t spp, uint32_t max_spp, uint32_t k)
{
    const uint32_t done = k * max_spp;
    return spp - done < max_spp ? spp - done : max_spp;
}

}  // namespace rpthost
