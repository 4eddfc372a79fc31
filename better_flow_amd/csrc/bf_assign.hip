// bf_assign.hip -- the assignment step of motion segmentation by motion compensation: every event to the one of K candidate models
// under which it lands on the largest pile of other events.  The definitions are in include/bf_accel.h ("event groups:
// assignment") and DESIGN.md section 15; the C-ABI around these kernels is in bf_assign_abi.cpp.  After an event's pixel
// everything is an integer count, a maximum or a smallest index, so no result depends on the order work-groups or waves run in.
//
//   A1 k_assign_vote   four events per thread, the K warps read on the scalar unit.  Per (event, model): the warp from the reset
//                      state, the scatter kernel's own pixel and window test, the vote test, one atomic add without a return
//                      value on the model's vote plane.  (Folding equal keys of neighbouring lanes into one add was measured and
//                      did not pay: DESIGN section 15.)
//   A2 k_assign_box    (scale > 1) B_k = the s x s box sum of V_k: box_sum_tile (bf_device_fns.h) with a halo of at most
//                      kMaxHalfScale, planes x tiles as the grid.  Every word of B is written.
//   A3 k_assign_pick   four events per thread: the K pixels again (recomputed, not stored), the gathers, leave-one-out, the
//                      smallest model with the largest score; id and score through perm; the counts per distinct id of the
//                      wave (for_each_wave_key, bf_device_fns.h) into LDS, `changed` and `max_score` likewise, then one global
//                      atomic per work-group and non-zero word.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr int kAssignEv = 4;                      // events per thread (a work-group's are consecutive per round)

// What a thread keeps of its events: address word, time, prior id (-1: votes under every model; -2: no event in this slot).
struct AssignEv {
    uint32_t v[kAssignEv];
    int32_t t[kAssignEv];
    int pri[kAssignEv];
    uint32_t up[kAssignEv];
};
__device__ __forceinline__ void assign_load(const AssignArgs& a, AssignEv& e) {
#pragma unroll
    for (int j = 0; j < kAssignEv; ++j) {
        const long long i = ((long long)blockIdx.x * kAssignEv + j) * kThreads + threadIdx.x;
        e.v[j] = 0; e.t[j] = 0; e.pri[j] = -2; e.up[j] = 0;
        if (i < a.n) {
            e.up[j] = a.perm ? a.perm[i] : (uint32_t)i;
            e.v[j] = a.xy[i];
            e.t[j] = a.t[i];
            e.pri[j] = a.prior ? a.prior[e.up[j]] : -1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_assign_vote(AssignArgs a, uint32_t* __restrict__ V) {
    const size_t plane = (size_t)a.R * (size_t)a.C;
    AssignEv e;
    assign_load(a, e);
    for (int k = 0; k < a.K; ++k) {   // (wave-uniform)
        const WarpParams wp = sload(a.wp + k);
        uint32_t* Vk = V + (size_t)k * plane;
#pragma unroll
        for (int j = 0; j < kAssignEv; ++j) {
            if (e.pri[j] != k && e.pri[j] != -1) continue;   // (-2, no event in this slot, among them)
            const int key = assign_pixel(wp, e.v[j], e.t[j], a.scale, a.x_sh, a.y_sh, a.wsx, a.wsy, a.C);
            if (key >= 0) atomicAdd(Vk + key, 1u);
        }
    }
}

// (planes x tiles as the grid: blockIdx.z the plane, .y and .x the tile's row and column)
__global__ __launch_bounds__(kThreads) void k_assign_box(const uint32_t* __restrict__ V, uint32_t* __restrict__ B, int R, int C, int hs) {
    const size_t base = (size_t)blockIdx.z * (size_t)R * (size_t)C;
    box_sum_tile<kMaxHalfScale>(V + base, B + base, R, C, hs, blockIdx.y * kBoxTR, blockIdx.x * kBoxTC);
}

__global__ __launch_bounds__(kThreads) void k_assign_pick(AssignArgs a, const uint32_t* __restrict__ B, int min_score,
                                                          int32_t* __restrict__ gid, int32_t* __restrict__ score,
                                                          uint32_t* __restrict__ out) {
    const size_t plane = (size_t)a.R * (size_t)a.C;
    AssignEv e;
    assign_load(a, e);
    int best[kAssignEv], arg[kAssignEv];
#pragma unroll
    for (int j = 0; j < kAssignEv; ++j) { best[j] = 0; arg[j] = 0; }
    for (int k = 0; k < a.K; ++k) {   // (wave-uniform)
        const WarpParams wp = sload(a.wp + k);
        const uint32_t* Bk = B + (size_t)k * plane;
#pragma unroll
        for (int j = 0; j < kAssignEv; ++j) {
            int key = -1;
            if (e.pri[j] != -2) key = assign_pixel(wp, e.v[j], e.t[j], a.scale, a.x_sh, a.y_sh, a.wsx, a.wsy, a.C);
            int s = 0;
            // leave-one-out: a voter's own vote is in the box sum of its pixel
            if (key >= 0) s = (int)Bk[key] - ((e.pri[j] == k || e.pri[j] == -1) ? 1 : 0);
            if (s > best[j]) { best[j] = s; arg[j] = k; }   // (strictly larger: ties stay with the smaller k)
        }
    }
    // The counts, `changed` and `max_score` of the work-group in LDS, then one global atomic per work-group and non-zero word: a
    // wave's events carry interleaved ids, so a per-wave flush on every change of id (k_seg_events' scheme, where consecutive
    // rounds name one component) issued ~3 same-address global atomics per wave and round -- 407 us of this kernel's time at K = 2
    // and 1.5 ms at K = 8 on 1M events.
    __shared__ uint32_t s_out[AssignBlock::size(kAssignMaxModels)];   // (the block is unstrided: the table is its image)
    const int nout = AssignBlock::size(a.K);
    for (int w = threadIdx.x; w < nout; w += kThreads) s_out[w] = 0u;
    __syncthreads();
    int changed = 0, top = 0;
#pragma unroll
    for (int j = 0; j < kAssignEv; ++j) {
        int slot = -1;   // the word of `out` this event counts in (AssignBlock::count): its id, K for -1; -1: no event
        if (e.pri[j] != -2) {
            const int g = best[j] >= min_score ? arg[j] : -1;
            gid[e.up[j]] = g;
            score[e.up[j]] = best[j];
            slot = g < 0 ? a.K : g;
            changed += g != e.pri[j];
            top = max(top, best[j]);
        }
        // one LDS add per distinct id of the wave
        for_each_wave_key(slot, [&](int k0, unsigned long long same) {
            if ((threadIdx.x & 63) == 0) atomicAdd(&s_out[k0], (uint32_t)__popcll(same));
        });
    }
    changed = (int)wave_sum((long long)changed);
    top = wave_max(top);
    if ((threadIdx.x & 63) == 0) {
        if (changed) atomicAdd(&s_out[AssignBlock::changed(a.K)], (uint32_t)changed);
        if (top) atomicMax(&s_out[AssignBlock::max_score(a.K)], (uint32_t)top);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < nout; w += kThreads) {
        const uint32_t v = s_out[w];
        if (!v) continue;
        if (w == AssignBlock::max_score(a.K)) atomicMax(out + w, v);
        else atomicAdd(out + w, v);
    }
}

unsigned event_blocks(long long n) {
    const long long per = (long long)kThreads * kAssignEv;
    return (unsigned)((n + per - 1) / per);
}

}  // namespace

void launch_assign_vote(const AssignArgs& a, uint32_t* V, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_assign_vote, dim3(event_blocks(a.n)), dim3(kThreads), 0, s, a, V);
}

void launch_assign_box(const uint32_t* V, uint32_t* B, int K, int R, int C, int scale, hipStream_t s) {
    const dim3 grid((unsigned)((C + kBoxTC - 1) / kBoxTC), (unsigned)((R + kBoxTR - 1) / kBoxTR), (unsigned)K);
    hipLaunchKernelGGL(k_assign_box, grid, dim3(kThreads), 0, s, V, B, R, C, scale / 2);
}

void launch_assign_pick(const AssignArgs& a, const uint32_t* B, int min_score, int32_t* gid, int32_t* score, uint32_t* out,
                        hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_assign_pick, dim3(event_blocks(a.n)), dim3(kThreads), 0, s, a, B, min_score, gid, score, out);
}

}  // namespace bf
