// bf_merge.hip -- how much of a group's contrast survives under another group's model: the pairwise merge gains of motion
// segmentation by motion compensation.  The definitions are in include/bf_accel.h ("event groups: merge gains") and DESIGN.md
// section 18; the C-ABI around these kernels is in bf_assign_abi.cpp.  The base planes B_k (every group under its own model) are
// bf_project_groups' own: launch_project_vote and launch_assign_box.  After an event's pixel everything is an integer count or a
// sum, so no result depends on the order work-groups or waves run in.  The per-id tallies are for_each_wave_key's and the wave
// reductions bf_device_fns.h's.
//
//   M1 k_merge_total   one pixel per thread and round: N = sum_k B_k, written; sum N and sum N^2 in registers until the loop ends,
//                      then one global atomic per work-group and non-zero word.
//   M2 k_merge_vote    the grid's second axis is the target model a of the pass, so its warp is wave-uniform and read on the
//                      scalar unit (k_assign_vote's form).  Four events per thread; an event with id g >= 0, g != a, that is
//                      inside under a adds 1 to plane (a_local K + g): one atomic add without a return value.  inside[g][a] per
//                      distinct id of the wave into LDS, then one global atomic per work-group and non-zero word.  The
//                      diagonal is not voted again: T[a][a] is the base plane B_a and inside[a][a] the base pass's count (the
//                      same integers: one model, one pixel function), which saves 1 / K of this kernel's scatters.
//      (bf_assign.hip) k_assign_box over the A K trial planes (scale > 1).
//   M3 k_merge_gain    the second axis is the target again; one pixel per thread and round in work-groups of 1024, at most 512
//                      per target (k_project_compose's measured shape).  N[p] once, then the K trial planes four at a time: the
//                      four loads are issued before the first ballot, so a round waits for one memory latency per four planes
//                      and not per plane (DESIGN section 17 named that chain); plane b == a is read from the base planes.  A
//                      plane without a non-zero word in the wave is skipped by ballot and its B_b is not loaded; else the
//                      64-bit term T (2 (N - B_b) + T), a wave sum, and one lane's 64-bit add into an LDS table of K words.
//                      One global atomic per work-group and non-zero word.
// Every word of the result block sits on a 128-byte line of its own (MergeBlock, bf_group_blocks.h; DESIGN section 17 measured
// why).
#include <hip/hip_runtime.h>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr int kMergeEv = 4;               // events per thread (a work-group's are consecutive per round)
constexpr int kGainThreads = 1024;        // k_merge_total, k_merge_gain: k_project_compose's shape
constexpr int kGainMaxGroups = 512;
constexpr int kGainBatch = 4;             // trial planes loaded before the first ballot of a batch

__global__ __launch_bounds__(kGainThreads) void k_merge_total(const uint32_t* __restrict__ B, int K, long long P,
                                                              uint32_t* __restrict__ Nout, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_tot[2];   // sum, sum_sq: MergeBlock::total's order
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long t_sum = 0, t_sq = 0;
    for (long long p = (long long)blockIdx.x * kGainThreads + threadIdx.x; p < P; p += (long long)gridDim.x * kGainThreads) {
        uint32_t N = 0;
        for (int k = 0; k < K; ++k) N += B[(size_t)k * (size_t)P + (size_t)p];
        Nout[p] = N;
        t_sum += N;
        t_sq += (unsigned long long)N * N;
    }
    t_sum = wave_sum_u64(t_sum);
    t_sq = wave_sum_u64(t_sq);
    if ((threadIdx.x & 63) == 0) {
        if (t_sum) atomicAdd(&s_tot[0], t_sum);
        if (t_sq) atomicAdd(&s_tot[1], t_sq);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_tot[threadIdx.x])
        atomicAdd(out + MergeBlock::total(K, threadIdx.x), s_tot[threadIdx.x]);
}

// (blockIdx.y: the target model of the pass, a = a0 + blockIdx.y)
__global__ __launch_bounds__(kThreads) void k_merge_vote(AssignArgs a, int a0, uint32_t* __restrict__ T,
                                                         unsigned long long* __restrict__ out) {
    const size_t plane = (size_t)a.R * (size_t)a.C;
    const int K = a.K;
    const int target = a0 + (int)blockIdx.y;
    __shared__ uint32_t s_in[kAssignMaxModels];
    for (int w = threadIdx.x; w < K; w += kThreads) s_in[w] = 0u;
    __syncthreads();
    const WarpParams wp = sload(a.wp + target);
    uint32_t* Ta = T + (size_t)blockIdx.y * (size_t)K * plane;
#pragma unroll
    for (int j = 0; j < kMergeEv; ++j) {
        const long long i = ((long long)blockIdx.x * kMergeEv + j) * kThreads + threadIdx.x;
        int g = -1;   // the event's id when it is inside under the target, else -1
        if (i < a.n) {
            const uint32_t up = a.perm ? a.perm[i] : (uint32_t)i;
            const int id = a.prior[up];
            if ((unsigned)id < (unsigned)K && id != target) {   // (the target's own group: its base plane, not voted again)
                const int key = assign_pixel(wp, a.xy[i], a.t[i], a.scale, a.x_sh, a.y_sh, a.wsx, a.wsy, a.C);
                if (key >= 0) {
                    atomicAdd(Ta + (size_t)id * plane + key, 1u);
                    g = id;
                }
            }
        }
        // one LDS add per distinct id of the wave
        for_each_wave_key(g, [&](int k0, unsigned long long same) {
            if ((threadIdx.x & 63) == 0) atomicAdd(&s_in[k0], (uint32_t)__popcll(same));
        });
    }
    __syncthreads();
    for (int w = threadIdx.x; w < K; w += kThreads) {
        const uint32_t c = s_in[w];
        if (c) atomicAdd(out + MergeBlock::inside(K, w, target), (unsigned long long)c);
    }
}

// (blockIdx.y: the target model of the pass; T: the pass's trial planes, box-summed when scale > 1; B: the base planes)
__global__ __launch_bounds__(kGainThreads) void k_merge_gain(const uint32_t* __restrict__ T, const uint32_t* __restrict__ B,
                                                             const uint32_t* __restrict__ Nin, int K, int a0, long long P,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_gain[kAssignMaxModels];
    for (int w = threadIdx.x; w < K; w += kGainThreads) s_gain[w] = 0ull;
    __syncthreads();
    const bool leader = (threadIdx.x & 63) == 0;
    const int target = a0 + (int)blockIdx.y;
    const uint32_t* Ta = T + (size_t)blockIdx.y * (size_t)K * (size_t)P;
    // (`base` is the same in every lane of the work-group: the ballots and reductions below are wave-uniform)
    for (long long base = (long long)blockIdx.x * kGainThreads; base < P; base += (long long)gridDim.x * kGainThreads) {
        const long long p = base + threadIdx.x;
        const bool live = p < P;
        const unsigned long long N = live ? Nin[p] : 0u;
        for (int b0 = 0; b0 < K; b0 += kGainBatch) {
            uint32_t t[kGainBatch];
#pragma unroll
            for (int j = 0; j < kGainBatch; ++j) {
                const int b = b0 + j;   // (the diagonal: T[a][a] is the base plane B_a)
                t[j] = (live && b < K) ? (b == target ? B : Ta)[(size_t)b * (size_t)P + (size_t)p] : 0u;
            }
#pragma unroll
            for (int j = 0; j < kGainBatch; ++j) {
                if (!__ballot(t[j] > 0)) continue;
                const int b = b0 + j;   // (< K: a plane beyond K has no non-zero word)
                unsigned long long term = 0;
                if (t[j]) {   // (then live)
                    const unsigned long long own = B[(size_t)b * (size_t)P + (size_t)p];
                    term = (unsigned long long)t[j] * (2ull * (N - own) + (unsigned long long)t[j]);
                }
                term = wave_sum_u64(term);
                if (leader) atomicAdd(&s_gain[b], term);
            }
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < K; w += kGainThreads)
        if (s_gain[w]) atomicAdd(out + MergeBlock::gain(K, w, target), s_gain[w]);
}

unsigned pixel_groups(long long P) {
    const long long groups = (P + kGainThreads - 1) / kGainThreads;
    return (unsigned)(groups < kGainMaxGroups ? groups : kGainMaxGroups);
}

}  // namespace

void launch_merge_total(const uint32_t* B, int K, int R, int C, uint32_t* N, unsigned long long* out, hipStream_t s) {
    const long long P = (long long)R * C;
    hipLaunchKernelGGL(k_merge_total, dim3(pixel_groups(P)), dim3(kGainThreads), 0, s, B, K, P, N, out);
}

void launch_merge_vote(const AssignArgs& a, int a0, int targets, uint32_t* T, unsigned long long* out, hipStream_t s) {
    if (a.n <= 0) return;
    const long long per = (long long)kThreads * kMergeEv;
    hipLaunchKernelGGL(k_merge_vote, dim3((unsigned)((a.n + per - 1) / per), (unsigned)targets), dim3(kThreads), 0, s, a, a0, T, out);
}

void launch_merge_gain(const uint32_t* T, const uint32_t* B, const uint32_t* N, int K, int a0, int targets, int R, int C,
                       unsigned long long* out, hipStream_t s) {
    const long long P = (long long)R * C;
    hipLaunchKernelGGL(k_merge_gain, dim3(pixel_groups(P), (unsigned)targets), dim3(kGainThreads), 0, s, T, B, N, K, a0, P, out);
}

}  // namespace bf
