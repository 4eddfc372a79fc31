// bf_track.hip -- tracking objects across slices: the overlap table between the held grouping of the slice uploaded now and the
// owner plane kept from an earlier slice.  The definition is in include/bf_accel.h ("event groups: tracks") and DESIGN.md section
// 20; the C-ABI around this kernel is in bf_track_abi.cpp (bf_track_keep drives the projection's kernels and launches nothing of
// its own).  A plain launch on the context's stream; no work-group waits for another; after an event's pixel everything is an
// integer count and the only atomics are adds without a return value, so no result depends on the order events are stored or
// work-groups run in.
//
//   T1 k_track_overlap  four events per thread, as k_project_vote takes them (a work-group's are consecutive per round; one
//                       flush per 1024 events instead of per 256).  The id through perm, as k_hold_groups reads it; the K warps
//                       staged once per work-group in LDS and selected per lane; bf_assign_groups' pixel and window test with
//                       the time operand the f32 nearest to the 64-bit t + dt (assign_pixel_ft); ONE 4-byte gather from the kept
//                       plane.  The tally: an LDS table of K x (Kp + 1) words, key k * (Kp + 1) + j.  After a bf_run_groups sort
//                       a wave holds one k and mostly one j, so equal keys are folded per wave into one LDS add by the leader
//                       (for_each_wave_key's rounds) -- but at most kTrackRounds of them: a wave of 64 distinct keys would
//                       take 64 rounds of two ballots each (DESIGN section 19's follow-up), so the lanes still pending after
//                       the last round add 1 each with their own LDS atomic.  outside / unassigned by ballot.  Then one global
//                       atomic per work-group and non-zero word, each word on a line of its own.
#include <hip/hip_runtime.h>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"
#include "bf_track.h"

namespace bf {

namespace {

constexpr int kTrackEv = 4;       // events per thread
constexpr int kTrackRounds = 4;   // leader rounds per wave and event round; the lanes left over add for themselves
constexpr int kTrackTabWords = TrackBlock::words(kAssignMaxModels, kAssignMaxModels);   // 16.6 KiB

__global__ __launch_bounds__(kThreads) void k_track_overlap(AssignArgs a, const int32_t* __restrict__ kept, int Kp, long long dt,
                                                            uint32_t* __restrict__ out) {
    __shared__ uint32_t s_tab[kTrackTabWords];   // the block's words, compact: overlap[K][Kp + 1], outside, unassigned
    __shared__ WarpParams s_wp[kAssignMaxModels];
    const int K = a.K, W = Kp + 1;
    const int words = K * W, all = TrackBlock::words(K, Kp);   // the table's words, and with outside and unassigned behind them
    stage_warps_lds(s_wp, a.wp, K);
    for (int w = threadIdx.x; w < all; w += kThreads) s_tab[w] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool leader = lane == 0;
#pragma unroll
    for (int j = 0; j < kTrackEv; ++j) {   // (wave-uniform: every lane reaches every ballot)
        const long long i = ((long long)blockIdx.x * kTrackEv + j) * kThreads + threadIdx.x;
        int key = -1;   // the table's word this event counts in; -1: outside, unassigned or no event
        bool outside = false, unassigned = false;
        if (i < a.n) {
            const uint32_t up = a.perm ? a.perm[i] : (uint32_t)i;
            const int g = a.prior[up];
            if ((unsigned)g < (unsigned)K) {
                const float ft = (float)((long long)a.t[i] + dt);   // the f32 nearest (ties to even) to the 64-bit sum
                const int px = assign_pixel_ft(s_wp[g], a.xy[i], ft, a.scale, a.x_sh, a.y_sh, a.wsx, a.wsy, a.C);
                if (px >= 0) {   // (inside the window: 0 <= px < R * C, the kept plane's size)
                    const int lab = kept[px];
                    key = g * W + ((unsigned)lab < (unsigned)Kp ? lab : Kp);
                } else {
                    outside = true;
                }
            } else {
                unassigned = true;
            }
        }
        const unsigned long long b_out = __ballot(outside), b_un = __ballot(unassigned);
        unsigned long long pending = __ballot(key >= 0);
        for (int r = 0; r < kTrackRounds && pending; ++r) {   // for_each_wave_key's rounds, bounded
            const int k0 = __shfl(key, __ffsll((long long)pending) - 1, 64);
            const unsigned long long same = __ballot(key == k0);
            if (leader) atomicAdd(&s_tab[k0], (uint32_t)__popcll(same));
            pending &= ~same;
        }
        if ((pending >> lane) & 1ull) atomicAdd(&s_tab[key], 1u);   // (a pending lane has a key)
        if (leader) {
            if (b_out) atomicAdd(&s_tab[words], (uint32_t)__popcll(b_out));
            if (b_un) atomicAdd(&s_tab[words + 1], (uint32_t)__popcll(b_un));
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < all; w += kThreads) {
        const uint32_t c = s_tab[w];
        if (c) atomicAdd(out + TrackBlock::word(w), c);
    }
}

}  // namespace

void launch_track_overlap(const AssignArgs& a, const int32_t* kept, int Kp, long long dt_ns, uint32_t* out, hipStream_t s) {
    if (a.n <= 0) return;
    const long long per = (long long)kThreads * kTrackEv;
    hipLaunchKernelGGL(k_track_overlap, dim3((unsigned)((a.n + per - 1) / per)), dim3(kThreads), 0, s, a, kept, Kp, dt_ns, out);
}

}  // namespace bf
