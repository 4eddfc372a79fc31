// bf_assign.h -- launchers of the assignment kernels (bf_assign.hip) for bf_assign_abi.cpp.  The definitions they implement are in
// include/bf_accel.h ("event groups: assignment").  Every launcher enqueues plain launches on the given stream; no kernel waits
// for another work-group.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf_device.h"

namespace bf {

constexpr int kAssignMaxModels = 64;
constexpr long long kAssignMaxWords = 1ll << 27;   // K x R x C vote words (and as many box sums when scale > 1)
// The events as stored (slot order; perm null: slot == upload index), the K warps, the window, and the prior (upload order;
// null: every event votes under every model).
struct AssignArgs {
    const uint32_t* xy; const int32_t* t; const uint32_t* perm;
    const WarpParams* wp;      // K, read on the scalar unit
    const int32_t* prior;
    long long n;
    int K, scale, x_sh, y_sh, wsx, wsy, R, C;
};

// Words of the result block: counts[K + 1] (last: unassigned), then changed, then max_score.
inline int assign_out_words(int K) { return K + 3; }

// V (K x R x C words, zero) += the votes.
void launch_assign_vote(const AssignArgs& a, uint32_t* V, hipStream_t s);
// B_k = the scale x scale box sum of V_k, every word of B written (scale > 1).
void launch_assign_box(const uint32_t* V, uint32_t* B, int K, int R, int C, int scale, hipStream_t s);
// gid / score through perm, and the result block (zero on entry).  B: the box sums, or V itself at scale 1.
void launch_assign_pick(const AssignArgs& a, const uint32_t* B, int min_score, int32_t* gid, int32_t* score, uint32_t* out,
                        hipStream_t s);

}  // namespace bf
