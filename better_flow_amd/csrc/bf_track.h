// bf_track.h -- launcher of the overlap kernel (bf_track.hip) for bf_track_abi.cpp.  The definition it implements is in
// include/bf_accel.h ("event groups: tracks") and DESIGN.md section 20.  A plain launch on the given stream; no work-group waits
// for another.  The result block is TrackBlock (bf_group_blocks.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf_assign.h"

namespace bf {

// out (zero) += the overlap table of the held grouping a.prior (K = a.K groups under a.wp, a's window) against the kept plane
// `kept` (R x C labels -1 .. Kp-1), every event's time operand the f32 nearest to t + dt_ns.
void launch_track_overlap(const AssignArgs& a, const int32_t* kept, int Kp, long long dt_ns, uint32_t* out, hipStream_t s);

}  // namespace bf
