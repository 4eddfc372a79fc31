// bf_track.h -- launcher of the overlap kernel (bf_track.hip) for bf_track_abi.cpp.  The definition it implements is in
// include/bf_accel.h ("event groups: tracks") and DESIGN.md section 20.  A plain launch on the given stream; no work-group waits
// for another.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf_assign.h"

namespace bf {

// The result block, 32-bit words: overlap[K x (Kp + 1)] (word k * (Kp + 1) + j; j == Kp: a pixel nobody owns), then outside,
// then unassigned.  Every word sits on a 128-byte line of its own (word w at index w * kTrackStride), as the projection's:
// the work-groups' atomics on words of one line queue behind each other.
constexpr int kTrackTail = 2;
constexpr int kTrackStride = 32;
inline int track_out_words(int K, int Kp) { return K * (Kp + 1) + kTrackTail; }
inline size_t track_out_size(int K, int Kp) { return (size_t)track_out_words(K, Kp) * kTrackStride; }

// out (zero) += the overlap table of the held grouping a.prior (K = a.K groups under a.wp, a's window) against the kept plane
// `kept` (R x C labels -1 .. Kp-1), every event's time operand the f32 nearest to t + dt_ns.
void launch_track_overlap(const AssignArgs& a, const int32_t* kept, int Kp, long long dt_ns, uint32_t* out, hipStream_t s);

}  // namespace bf
