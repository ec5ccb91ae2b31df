// launch_move.h — the seam between capi.hip and the kernels of the device-source mesh calls (k_move.hip, a code object library of its
// own: build.py, move_lib_of).  A header of its own beside launch.h: the kernel translation units that include launch.h do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_move.h"

namespace rptlaunch {

// The check of one source's `n` vertices, read from `src` (device memory of the current device) through `xf`: the two words of
// host_move.h (kMoveWordBig, kMoveWordBad) reduced into `words`, which the caller zeroed; `referenced`: one byte per vertex of this
// mesh.  Stores nothing else.
hipError_t move_check(const float* src, const rpthost::MoveTransform& xf, const uint8_t* referenced, uint32_t* words, uint32_t n, hipStream_t st);
// The same load and the same statement, stored: dst[3v .. 3v+2] = the position of vertex v.
hipError_t move_apply(const float* src, const rpthost::MoveTransform& xf, float* dst, uint32_t n, hipStream_t st);

}  // namespace rptlaunch
