// bf_hold_groups.h -- launchers of bf_hold_groups.hip for bf_global_search.cpp: the held flow of a grouping and its K models, and
// the per-group median of a held flow by an exact radix select (include/bf_accel.h, "the held flow of a grouping").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf_device.h"
#include "bf_kernels.h"

namespace bf {

// Slot i of the context's order (upload index perm[i]; null: i) under the warp of its own group's model (wp[gid], gid in upload
// order; -1: zero flow, zero products), from the reset state.  The slot order is copied into h.xy / h.idx, as
// launch_global_hold_best does.
void launch_hold_groups(const uint32_t* xy, const int32_t* t, const uint32_t* perm, const int32_t* gid, const WarpParams* wp,
                        int K, long long n, const GlobalHeld& h, hipStream_t s);

// The select's state for K groups.  Target T = ((group * 2 + axis) * 2 + j), j = 0: rank c/2 - 1 (c/2 for an odd count), j = 1:
// rank c/2; pair = group * 2 + axis.
constexpr int kMedianChunk = 8;   // groups whose tables one work-group of the counting kernel holds in LDS
struct MedianState {
    unsigned long long* prefix;   // 4 K: the digits chosen so far, in their place in the key
    uint32_t* rank;               // 4 K: the target's rank among the values that match its prefix
    uint32_t* count;              // 2 K: the pair's number of values
    uint32_t* hist;               // 4 K x 256: the pass's digit counts, ZERO before every pass
    double* median;               // 2 K: written by the last pass
};
// Bytes of everything but the digit counts (prefix, median, rank, count, in this order), rounded up to 16; and of all of it.
inline size_t median_state_head(int K) { return ((size_t)K * (4 * 8 + 2 * 8 + 4 * 4 + 2 * 4) + 15) & ~(size_t)15; }
inline size_t median_state_bytes(int K) { return median_state_head(K) + (size_t)K * 4 * 256 * 4; }
// Pass `pass` (0 .. 7) of the select over the n held (u, v) and ids, both in upload order: the counting launch (none when
// n == 0) and the one-work-group pick.  st.hist zero on entry; before pass 0 everything of the state zero.
void launch_median_pass(const double2* uv, const int32_t* gid, long long n, int K, int pass, const MedianState& st, hipStream_t s);

}  // namespace bf
