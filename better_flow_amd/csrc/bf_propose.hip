// bf_propose.hip -- candidate models from the modes of the per-event best flow the exhaustive search leaves behind.  The
// definitions are in include/bf_accel.h ("event groups: candidate models") and DESIGN.md section 16; the C-ABI around these
// kernels is in bf_propose_abi.cpp.  After an event's lattice index everything is an integer count, a maximum or a lowest index,
// so no result depends on the order work-groups or waves run in.
//
//   P1 k_propose_vote  four events per thread and round, the work-groups striding over the slice.  Per event: max_score > 0,
//                      then the two indices by a binary search over the value tables and one exact comparison each.  Two forms,
//                      chosen on the host by the lattice (propose_fits_lds):
//                        LDS     the tables and a histogram of the whole lattice in the work-group's LDS, one LDS atomic per
//                                vote, one global atomic per work-group and non-zero bin at its end;
//                        global  the tables read from memory, one global atomic without a return value per vote.
//                      (Folding the lanes that share the wave's most frequent bins into one add each is the BF_PROPOSE_FOLD
//                      build: DESIGN section 16 has the A/B.)
//   P2 k_propose_box   B = the (2 r + 1)^2 box sum of H: box_sum_tile (bf_device_fns.h), k_assign_box's routine, with a halo of
//                      at most kProposeMaxRadius and all tiles on one grid axis.  Every word of B is written.
//   P3 k_propose_pick  one work-group of 1024 threads, max_models rounds over B: per thread the largest (B, lowest index) of its
//                      words that no earlier pick suppresses (the list of picks is in LDS; a word is tested against it only when
//                      it would beat the thread's best), then a wave and a work-group maximum of the 64-bit key.  A lattice of at
//                      most 16 384 points is read once, into registers; a larger one again in every round.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"

namespace bf {

namespace {

constexpr int kProposeEv = 4;                     // events per thread and round
constexpr int kProposeBlocks = 512;               // at most: the work-groups stride over the slice
constexpr int kPickThreads = 1024;
constexpr int kPickRegs = 16;                     // words of B a thread of k_propose_pick keeps in registers (small lattices)

// The index of v in the strictly increasing table, or -1: a lower bound, then the one exact comparison (NaN: -1).
template <class Tab>
__device__ __forceinline__ int propose_index(Tab tab, int m, double v) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (lo < m && tab[lo] == v) ? lo : -1;
}

// What a thread keeps of one round's events: the bin, or -1 unscored, -2 off the lattice, -3 no event in this slot.
template <class Tab>
__device__ __forceinline__ void propose_keys(const ProposeArgs& a, Tab tab_x, Tab tab_y, long long base, int key[kProposeEv]) {
    double ms[kProposeEv], bx[kProposeEv], by[kProposeEv];
#pragma unroll
    for (int j = 0; j < kProposeEv; ++j) {
        const long long e = base + (long long)j * kThreads + threadIdx.x;
        ms[j] = -1.0; bx[j] = 0.0; by[j] = 0.0;
        if (e < a.n) { ms[j] = a.max_score[e]; bx[j] = a.best_nx[e]; by[j] = a.best_ny[e]; }
    }
#pragma unroll
    for (int j = 0; j < kProposeEv; ++j) {
        const long long e = base + (long long)j * kThreads + threadIdx.x;
        if (e >= a.n) { key[j] = -3; continue; }
        if (!(ms[j] > 0.0)) { key[j] = -1; continue; }
        const int i = propose_index(tab_x, a.n_x, bx[j]);
        const int k = i < 0 ? -1 : propose_index(tab_y, a.n_y, by[j]);
        key[j] = (i < 0 || k < 0) ? -2 : i * a.n_y + k;
    }
}

// The three counts of the work-group into out[0 .. 3): wave sums, LDS, one global atomic per non-zero word.
__device__ __forceinline__ void propose_counts(int voted, int unscored, int off, uint32_t* s_cnt, uint32_t* out) {
    voted = (int)wave_sum((long long)voted);
    unscored = (int)wave_sum((long long)unscored);
    off = (int)wave_sum((long long)off);
    if ((threadIdx.x & 63) == 0) {
        if (voted) atomicAdd(&s_cnt[0], (uint32_t)voted);
        if (unscored) atomicAdd(&s_cnt[1], (uint32_t)unscored);
        if (off) atomicAdd(&s_cnt[2], (uint32_t)off);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(out + threadIdx.x, s_cnt[threadIdx.x]);
}

template <class Hist>
__device__ __forceinline__ void propose_add(Hist h, int key) {
#ifdef BF_PROPOSE_FOLD
    // the lanes that share the bin of the wave's first voter, twice, as one add each; the others one by one.  The ballots are
    // the same in all 64 lanes: every lane of the wave is here (the callers do not branch around this)
    int left = key;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long pending = __ballot(left >= 0);
        if (!pending) break;
        const int lead = __ffsll((long long)pending) - 1;
        const int k0 = __shfl(left, lead, 64);
        const unsigned long long same = __ballot(left == k0);
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(h + k0, (uint32_t)__popcll(same));
        if (left == k0) left = -1;
    }
    if (left >= 0) atomicAdd(h + left, 1u);
#else
    if (key >= 0) atomicAdd(h + key, 1u);
#endif
}

__global__ __launch_bounds__(kThreads) void k_propose_vote(ProposeArgs a, uint32_t* __restrict__ H, uint32_t* __restrict__ out) {
    extern __shared__ double s_dyn[];   // n_x + n_y table values, then the n_x * n_y words of the histogram
    __shared__ uint32_t s_cnt[3];
    double* s_tab = s_dyn;
    uint32_t* s_h = reinterpret_cast<uint32_t*>(s_tab + a.n_x + a.n_y);
    const int bins = a.n_x * a.n_y;
    for (int w = threadIdx.x; w < a.n_x + a.n_y; w += kThreads) s_tab[w] = a.tab[w];
    for (int w = threadIdx.x; w < bins; w += kThreads) s_h[w] = 0u;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    int voted = 0, unscored = 0, off = 0;
    const long long per = (long long)kThreads * kProposeEv;
    for (long long base = (long long)blockIdx.x * per; base < a.n; base += (long long)gridDim.x * per) {   // (uniform per work-group)
        int key[kProposeEv];
        propose_keys(a, (const double*)s_tab, (const double*)(s_tab + a.n_x), base, key);
#pragma unroll
        for (int j = 0; j < kProposeEv; ++j) {
            voted += key[j] >= 0; unscored += key[j] == -1; off += key[j] == -2;
            propose_add(s_h, key[j]);
        }
    }
    propose_counts(voted, unscored, off, s_cnt, out);   // (its barrier also orders the histogram's adds before the flush)
    for (int w = threadIdx.x; w < bins; w += kThreads) {
        const uint32_t v = s_h[w];
        if (v) atomicAdd(H + w, v);
    }
}

__global__ __launch_bounds__(kThreads) void k_propose_vote_global(ProposeArgs a, uint32_t* __restrict__ H, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    int voted = 0, unscored = 0, off = 0;
    const long long per = (long long)kThreads * kProposeEv;
    for (long long base = (long long)blockIdx.x * per; base < a.n; base += (long long)gridDim.x * per) {
        int key[kProposeEv];
        propose_keys(a, a.tab, a.tab + a.n_x, base, key);
#pragma unroll
        for (int j = 0; j < kProposeEv; ++j) {
            voted += key[j] >= 0; unscored += key[j] == -1; off += key[j] == -2;
            propose_add(H, key[j]);
        }
    }
    propose_counts(voted, unscored, off, s_cnt, out);
}

__global__ __launch_bounds__(kThreads) void k_propose_box(const uint32_t* __restrict__ H, uint32_t* __restrict__ B, int R, int C, int hs) {
    // (the tiles as one grid axis, row of tiles major: a lattice of 2^22 x 1 has more tile rows than a grid's second axis takes)
    const int tiles_c = (C + kBoxTC - 1) / kBoxTC;
    box_sum_tile<kProposeMaxRadius>(H, B, R, C, hs, (int)(blockIdx.x / (unsigned)tiles_c) * kBoxTR,
                                    (int)(blockIdx.x % (unsigned)tiles_c) * kBoxTC);
}

// The key of a word: the larger B wins, among equals the lower index; 0: nothing (an index is below 2^22, so a key never is 0).
__device__ __forceinline__ unsigned long long pick_key(uint32_t b, int idx) {
    return ((unsigned long long)b << 32) | (unsigned long long)(0xffffffffu - (uint32_t)idx);
}

// One word of B against the thread's best so far: it replaces it when its key is larger and none of the p picks suppresses it.
__device__ __forceinline__ void pick_consider(uint32_t b, int idx, int n_y, int suppress, int p, const int* s_pi, const int* s_pj,
                                              unsigned long long& best) {
    const unsigned long long k = pick_key(b, idx);
    if (k <= best) return;
    const int i = idx / n_y, j = idx - i * n_y;
    for (int q = 0; q < p; ++q) {
        const int di = i - s_pi[q], dj = j - s_pj[q];
        if (di <= suppress && di >= -suppress && dj <= suppress && dj >= -suppress) return;
    }
    best = k;
}

// CACHED: the lattice has at most kPickThreads * kPickRegs points (the default one has 14 400), and a thread keeps its words of B
// in registers over the rounds; otherwise every round reads B again.
template <bool CACHED>
__global__ __launch_bounds__(kPickThreads) void k_propose_pick(const uint32_t* __restrict__ H, const uint32_t* __restrict__ B,
                                                               int n_x, int n_y, int suppress, int max_models, int min_votes,
                                                               uint32_t* __restrict__ out) {
    __shared__ int s_pi[kProposeMaxModels], s_pj[kProposeMaxModels];
    __shared__ unsigned long long s_wave[kPickThreads / 64];
    __shared__ unsigned long long s_best;
    const int bins = n_x * n_y;
    uint32_t mine[kPickRegs];
    if (CACHED) {
#pragma unroll
        for (int r = 0; r < kPickRegs; ++r) {
            const int idx = r * kPickThreads + (int)threadIdx.x;
            mine[r] = idx < bins ? B[idx] : 0u;
        }
    }
    int picked = 0;
    for (int p = 0; p < max_models; ++p) {   // (uniform: every thread sees the same s_best)
        unsigned long long best = 0ull;
        if (CACHED) {
#pragma unroll
            for (int r = 0; r < kPickRegs; ++r) {
                const int idx = r * kPickThreads + (int)threadIdx.x;
                if (idx < bins) pick_consider(mine[r], idx, n_y, suppress, p, s_pi, s_pj, best);
            }
        } else {
            for (int idx = threadIdx.x; idx < bins; idx += kPickThreads) pick_consider(B[idx], idx, n_y, suppress, p, s_pi, s_pj, best);
        }
        best = wave_max_u64(best);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long m = 0ull;
            for (int w = 0; w < kPickThreads / 64; ++w) m = s_wave[w] > m ? s_wave[w] : m;
            s_best = m;
            if (m != 0ull && (uint32_t)(m >> 32) >= (uint32_t)min_votes) {
                const int idx = (int)(0xffffffffu - (uint32_t)m);
                s_pi[p] = idx / n_y;
                s_pj[p] = idx - (idx / n_y) * n_y;
                out[kProposeOutHead + 3 * p] = (uint32_t)idx;
                out[kProposeOutHead + 3 * p + 1] = (uint32_t)(m >> 32);
                out[kProposeOutHead + 3 * p + 2] = H[idx];
            }
        }
        __syncthreads();
        const unsigned long long m = s_best;
        if (m == 0ull || (uint32_t)(m >> 32) < (uint32_t)min_votes) break;
        ++picked;
    }
    if (threadIdx.x == 0) out[3] = (uint32_t)picked;
}

}  // namespace

int launch_propose_vote(const ProposeArgs& a, uint32_t* H, uint32_t* out, hipStream_t s) {
    if (a.n <= 0) return 0;
    const long long per = (long long)kThreads * kProposeEv;
    const unsigned blocks = (unsigned)std::min((long long)kProposeBlocks, (a.n + per - 1) / per);
    if (propose_fits_lds(a.n_x, a.n_y)) {
        const size_t lds = (size_t)(a.n_x + a.n_y) * sizeof(double) + (size_t)a.n_x * (size_t)a.n_y * sizeof(uint32_t);
        hipLaunchKernelGGL(k_propose_vote, dim3(blocks), dim3(kThreads), lds, s, a, H, out);
        return 1;
    }
    hipLaunchKernelGGL(k_propose_vote_global, dim3(blocks), dim3(kThreads), 0, s, a, H, out);
    return 2;
}

void launch_propose_box(const uint32_t* H, uint32_t* B, int n_x, int n_y, int radius, hipStream_t s) {
    const dim3 grid((unsigned)((n_y + kBoxTC - 1) / kBoxTC) * (unsigned)((n_x + kBoxTR - 1) / kBoxTR));
    hipLaunchKernelGGL(k_propose_box, grid, dim3(kThreads), 0, s, H, B, n_x, n_y, radius);
}

void launch_propose_pick(const uint32_t* H, const uint32_t* B, int n_x, int n_y, int suppress, int max_models, int min_votes,
                         uint32_t* out, hipStream_t s) {
    if ((long long)n_x * n_y <= (long long)kPickThreads * kPickRegs)
        hipLaunchKernelGGL(k_propose_pick<true>, dim3(1), dim3(kPickThreads), 0, s, H, B, n_x, n_y, suppress, max_models, min_votes, out);
    else
        hipLaunchKernelGGL(k_propose_pick<false>, dim3(1), dim3(kPickThreads), 0, s, H, B, n_x, n_y, suppress, max_models, min_votes, out);
}

}  // namespace bf
