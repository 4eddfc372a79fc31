// bf_project.hip -- the slice with every event warped by its OWN group's model: the picture and the objective of motion
// segmentation by motion compensation.  The definitions are in include/bf_accel.h ("event groups: projection") and DESIGN.md
// section 17; the C-ABI around these kernels is in bf_assign_abi.cpp.  After an event's pixel everything is an integer count, a
// sum, a maximum or a smallest index, so no result depends on the order work-groups or waves run in.  The per-id tallies are
// for_each_wave_key's and the wave reductions bf_device_fns.h's.
//
//   P1 k_project_vote     four events per thread.  The model differs per event (ids are interleaved in upload order), so the K
//                         warps sit in LDS and each lane reads its group's (a loop over the wave's distinct ids with the warp on
//                         the scalar unit measured the same and was dropped: DESIGN section 17); bf_assign_groups' pixel and window test; one atomic
//                         add without a return value on the event's own group's plane.  events / inside per group and the
//                         unassigned count: per distinct id of the wave with ballots into LDS, then one global atomic per
//                         work-group and non-zero word.
//      (bf_assign.hip)    k_assign_box: B_k = the s x s box sum of V_k (scale > 1).
//   P2 k_project_compose  a grid-stride loop over the pixels in work-groups of 1024, one pixel per thread and round: one pass over the K planes for N and the
//                         owner, then the colour.  Per plane that has a non-zero word in the wave: pixels_hit by ballot, max and
//                         the 64-bit sum of squares by wave reductions, into an LDS table; pixels_owned per distinct label of
//                         the wave; the totals in registers until the loop ends.  One global atomic per work-group and non-zero
//                         word.
#include <hip/hip_runtime.h>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr int kProjectEv = 4;             // events per thread (a work-group's are consecutive per round)
// k_project_compose: at most 512 work-groups of 1024 threads (two per CU), each flushes its table once.  As many threads in
// work-groups of 256 took 82 us instead of 17 at K = 2 on 1M events: four times the flushes
constexpr int kComposeThreads = 1024;
constexpr int kComposeMaxGroups = 512;

__constant__ uint8_t c_palette[BF_PROJECT_PALETTE_SIZE][3] = BF_PROJECT_PALETTE;

__global__ __launch_bounds__(kThreads) void k_project_vote(AssignArgs a, uint32_t* __restrict__ V,
                                                           unsigned long long* __restrict__ out) {
    const size_t plane = (size_t)a.R * (size_t)a.C;
    const int K = a.K;
    __shared__ uint32_t s_cnt[2 * kAssignMaxModels + 1];   // events[K], unassigned, inside[K]
    __shared__ WarpParams s_wp[kAssignMaxModels];
    {   // (32-bit words, not stage_warps_lds' 8-byte form: this kernel's measured code is kept as it is)
        constexpr int kWords = (int)(sizeof(WarpParams) / sizeof(uint32_t));
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.wp);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_wp);
        for (int w = threadIdx.x; w < K * kWords; w += kThreads) dst[w] = src[w];
    }
    for (int w = threadIdx.x; w < 2 * K + 1; w += kThreads) s_cnt[w] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kProjectEv; ++j) {
        const long long i = ((long long)blockIdx.x * kProjectEv + j) * kThreads + threadIdx.x;
        int slot = -1;   // the word of s_cnt this event counts in: its id, K for -1; -1: no event
        int key = -1;
        uint32_t v = 0;
        int32_t t = 0;
        if (i < a.n) {
            const uint32_t up = a.perm ? a.perm[i] : (uint32_t)i;
            const int g = a.prior[up];
            slot = (unsigned)g < (unsigned)K ? g : K;
            v = a.xy[i];
            t = a.t[i];
        }
        if (slot >= 0 && slot < K) {
            const WarpParams wp = s_wp[slot];
            key = assign_pixel(wp, v, t, a.scale, a.x_sh, a.y_sh, a.wsx, a.wsy, a.C);
            if (key >= 0) atomicAdd(V + (size_t)slot * plane + key, 1u);
        }
        // one round per distinct id of the wave
        for_each_wave_key(slot, [&](int k0, unsigned long long same) {
            const unsigned long long in = __ballot(slot == k0 && key >= 0);
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(&s_cnt[k0], (uint32_t)__popcll(same));
                if (in) atomicAdd(&s_cnt[K + 1 + k0], (uint32_t)__popcll(in));   // (k0 < K: an unassigned event has no key)
            }
        });
    }
    __syncthreads();
    for (int w = threadIdx.x; w < 2 * K + 1; w += kThreads) {
        const uint32_t c = s_cnt[w];
        if (!c) continue;
        atomicAdd(out + ProjectBlock::vote_word(K, w), (unsigned long long)c);
    }
}

__global__ __launch_bounds__(kComposeThreads) void k_project_compose(const uint32_t* __restrict__ B, int K, long long P, int gain,
                                                                     uint32_t* __restrict__ count, int32_t* __restrict__ label,
                                                                     uint8_t* __restrict__ bgr,
                                                                     unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_sq[kAssignMaxModels];
    __shared__ uint32_t s_hit[kAssignMaxModels], s_own[kAssignMaxModels], s_max[kAssignMaxModels];
    __shared__ unsigned long long s_tot[3];   // pixels, sum, sum_sq: ProjectBlock::total's order
    for (int w = threadIdx.x; w < K; w += kComposeThreads) { s_sq[w] = 0ull; s_hit[w] = 0u; s_own[w] = 0u; s_max[w] = 0u; }
    if (threadIdx.x < 3) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const bool leader = (threadIdx.x & 63) == 0;
    unsigned long long t_px = 0, t_sum = 0, t_sq = 0;
    // (`base` is the same in every lane of the work-group: the ballots and reductions below are wave-uniform)
    for (long long base = (long long)blockIdx.x * kComposeThreads; base < P; base += (long long)gridDim.x * kComposeThreads) {
        const long long p = base + threadIdx.x;
        const bool live = p < P;
        uint32_t N = 0, best = 0;
        int arg = -1;
        for (int k = 0; k < K; ++k) {
            const uint32_t b = live ? B[(size_t)k * (size_t)P + (size_t)p] : 0u;
            const unsigned long long hit = __ballot(b > 0);
            if (!hit) continue;
            N += b;
            if (b > best) { best = b; arg = k; }   // (strictly larger: ties stay with the smaller k)
            const uint32_t m = wave_max_u32(b);
            const unsigned long long sq = wave_sum_u64((unsigned long long)b * b);
            if (leader) {
                atomicAdd(&s_hit[k], (uint32_t)__popcll(hit));
                atomicMax(&s_max[k], m);
                atomicAdd(&s_sq[k], sq);
            }
        }
        if (live) {
            count[p] = N;
            label[p] = arg;
            uint32_t level = 0;
            int col = 0;
            if (arg >= 0) {
                const unsigned long long x = (unsigned long long)best * (unsigned long long)gain;
                level = x > 255ull ? 255u : (uint32_t)x;
                col = arg % BF_PROJECT_PALETTE_SIZE;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) bgr[3 * (size_t)p + c] = (uint8_t)((uint32_t)c_palette[col][c] * level / 255u);
        }
        for_each_wave_key(arg, [&](int k0, unsigned long long same) {   // one LDS add per distinct label of the wave
            if (leader) atomicAdd(&s_own[k0], (uint32_t)__popcll(same));
        });
        t_px += N > 0;
        t_sum += N;
        t_sq += (unsigned long long)N * N;
    }
    t_px = wave_sum_u64(t_px);
    t_sum = wave_sum_u64(t_sum);
    t_sq = wave_sum_u64(t_sq);
    if (leader) {
        if (t_px) atomicAdd(&s_tot[0], t_px);
        if (t_sum) atomicAdd(&s_tot[1], t_sum);
        if (t_sq) atomicAdd(&s_tot[2], t_sq);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < K; w += kComposeThreads) {
        if (s_hit[w]) atomicAdd(out + ProjectBlock::pixels_hit(K, w), (unsigned long long)s_hit[w]);
        if (s_own[w]) atomicAdd(out + ProjectBlock::pixels_owned(K, w), (unsigned long long)s_own[w]);
        if (s_max[w]) atomicMax(out + ProjectBlock::max(K, w), (unsigned long long)s_max[w]);
        if (s_sq[w]) atomicAdd(out + ProjectBlock::sum_sq(K, w), s_sq[w]);
    }
    if (threadIdx.x < 3 && s_tot[threadIdx.x])
        atomicAdd(out + ProjectBlock::total(K, threadIdx.x), s_tot[threadIdx.x]);
}

}  // namespace

void launch_project_vote(const AssignArgs& a, uint32_t* V, unsigned long long* out, hipStream_t s) {
    if (a.n <= 0) return;
    const long long per = (long long)kThreads * kProjectEv;
    hipLaunchKernelGGL(k_project_vote, dim3((unsigned)((a.n + per - 1) / per)), dim3(kThreads), 0, s, a, V, out);
}

void launch_project_compose(const uint32_t* B, int K, int R, int C, int gain, uint32_t* count, int32_t* label, uint8_t* bgr,
                            unsigned long long* out, hipStream_t s) {
    const long long P = (long long)R * C;
    const long long groups = (P + kComposeThreads - 1) / kComposeThreads;
    hipLaunchKernelGGL(k_project_compose, dim3((unsigned)(groups < kComposeMaxGroups ? groups : kComposeMaxGroups)), dim3(kComposeThreads), 0,
                       s, B, K, P, gain, count, label, bgr, out);
}

}  // namespace bf
