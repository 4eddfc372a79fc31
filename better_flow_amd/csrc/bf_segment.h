// bf_segment.h -- launchers of the segmentation kernels (bf_segment.hip) for bf_segment_abi.cpp.  The definitions they implement
// are in include/bf_accel.h ("moving-object segmentation").  Every launcher enqueues plain launches on the given stream; no
// kernel waits for another work-group.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bf_accel.h"

namespace bf {

// The scalars of one segmentation on the device: the exact reduction of step 2, then the counts of steps 3 and 4.
struct SegDev {
    long long q_sum;
    unsigned long long n1;
    long long mu;
    uint32_t fg, found, kept, pad;
};

// How a pixel becomes foreground: a host-style mask (non-zero), or step 3 on (T, c) with the mean in SegDev.
struct SegMask {
    const uint8_t* mask;
    const float* T;
    const uint32_t* cnt;
    long long A, B;
    int use_a, use_b;
    uint32_t min_count;
};

constexpr int kSegRankPx = 2048;   // pixels per work-group of the ordered compaction (k_seg_count / k_seg_assign)
inline int seg_rank_blocks(long long P) { return (int)((P + kSegRankPx - 1) / kSegRankPx); }

// step 2: Q, n1 (one 64-bit atomic each per work-group) and mu.  *dev must be zero.
void launch_seg_mean(const float* T, const uint32_t* cnt, long long P, SegDev* dev, hipStream_t s);
// steps 3 and 4 up to the flattened roots: lab[p] = smallest pixel index of p's component, -1 for background; sz[root] = its
// pixels (sz must be zero); dev->fg.
void launch_seg_label(const SegMask& m, int R, int C, int connectivity, int32_t* lab, int32_t* sz, SegDev* dev, hipStream_t s);
// size filter and renumbering: nid[root] = id in 0 .. K-1 or -1; dev->found, dev->kept.  scratch: seg_rank_blocks(P) words.
void launch_seg_rank(const int32_t* lab, const int32_t* sz, int32_t* nid, long long P, int min_pixels, unsigned long long* scratch,
                     SegDev* dev, hipStream_t s);
// lab becomes the final labels in place; the table's K rows (T null: q_sum stays 0).
void launch_seg_table(int32_t* lab, const int32_t* nid, const float* T, bf_component* table, int K, int R, int C, hipStream_t s);
// step 6: cl_id through perm (null: slot == upload index) and the components' event counts.
struct SegEvents {
    const uint32_t* xy; const float2* p; const uint8_t* noise; const uint32_t* perm;
    long long n;
    int scale, x_sh, y_sh, wsx, wsy, C;
};
void launch_seg_events(const SegEvents& e, const int32_t* labels, int32_t* cl_id, bf_component* table, hipStream_t s);

}  // namespace bf
