// bf_segment.hip -- connected-component labelling of the compensated time image, its component table and the per-event
// cluster ids; the definitions are in include/bf_accel.h ("moving-object segmentation") and DESIGN.md section 13.  The C-ABI
// around these kernels is in bf_segment_abi.cpp.  Everything is integer arithmetic with order-free operations (sums, minima,
// maxima), and a component's root is its smallest pixel index, so no result depends on the order work-groups or waves run in.
//
//   S1 k_seg_reduce   Q and n1 of step 2: per-thread i64 sums, wave shuffles, LDS, then ONE 64-bit atomic each per work-group.
//   S2 k_seg_mean     one thread: mu = floor_div(Q, n1) (a 64-bit division nobody else should repeat per pixel).
//   S3 k_seg_tile     a 32 x 64 tile per work-group: the foreground test of step 3 (or the host mask), then union-find over the
//                     tile's 2048 label words in LDS (atomicMin links towards the smaller index), flattened and written to the
//                     global label plane as GLOBAL pixel indices: the smallest local index of a tile component is also its
//                     smallest global one, both orders being row-major.
//   S4 k_seg_border   one thread per pixel of a tile's top row, left column and right column: unites it with its backward
//                     neighbours (W, N; NW, NE for 8-connectivity) that lie in ANOTHER tile, on the global plane.  Of two
//                     adjacent pixels exactly one is the backward neighbour of the other, so every pair across a tile edge or
//                     corner is seen once.  The plane is read with agent-scope atomic loads and linked with atomicMin: the
//                     L2 slices of the eight dies are not coherent for plain loads inside a launch.
//   S5 k_seg_flatten  lab[p] = root(p), and the component sizes: 16 consecutive pixels per thread, runs of equal roots summed in
//                     registers, the lanes' last runs folded per root over the wave, then one atomic per distinct root.  (A
//                     concurrent reader sees an older or a newer ancestor; both lead to the same root.)
//   S6 k_seg_count / k_seg_scan / k_seg_assign   ordered compaction of the roots that pass the size filter: per-work-group
//                     counts, one work-group scans them, then every kept root gets its rank in pixel order -- ids ascend with
//                     the smallest pixel index.
//   S7 k_seg_table_init / k_seg_relabel / k_seg_stats   labels in place, first_pixel, and the per-component sums: runs of equal
//                     labels are summed in registers, the lanes' last runs are folded per component over the wave with
//                     shuffles, then integer atomics on the table row.
//   S8 k_seg_events   four events per thread: the scatter kernel's own pixel, cl_id through perm, the components' event counts --
//                     counted per distinct component of the wave with ballots, kept in registers while consecutive rounds name
//                     the same component, then one atomic.
// The three folds over a wave's distinct roots / components (S5, S7, S8) are for_each_wave_key's rounds (bf_device_fns.h).
#include <hip/hip_runtime.h>
#include <limits.h>

#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"
#include "bf_segment.h"

namespace bf {

namespace {

constexpr int kSegTR = 32, kSegTC = 64;           // tile of k_seg_tile
constexpr int kSegTilePx = kSegTR * kSegTC;
constexpr int kSegRun = 16;                       // consecutive pixels per thread in k_seg_flatten / k_seg_stats

__device__ __forceinline__ long long seg_q(float t) { return (long long)floor((double)t * 1073741824.0); }

// ---- union-find on an LDS label array (values: -1 background, else the index of a parent <= the own index) --------------------
__device__ __forceinline__ int lds_find(const volatile int* L, int a) {
    // finite: a parent index only ever decreases (L[x] <= x, links are made with atomicMin), so the walk strictly descends
    for (;;) {
        const int q = L[a];
        if (q == a) return a;
        a = q;
    }
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    // finite: every round either returns or replaces the larger root by a strictly smaller index (old < a)
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;   // a was still a root: linked
        a = old;                // somebody linked a to old (< a) first: old and b remain to be united
    }
}

// ---- the same on the global plane, across work-groups: agent-scope loads ----------------------------------------------------
__device__ __forceinline__ int g_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int32_t* L, int a) {
    // finite: a parent index only ever decreases, so the walk strictly descends
    for (;;) {
        const int q = g_load(L + a);
        if (q == a) return a;
        a = q;
    }
}
__device__ __forceinline__ void g_union(int32_t* L, int a, int b) {
    // finite: every round either returns or replaces the larger root by a strictly smaller index (old < a)
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// exclusive scan of one u64 per thread over a 256-thread work-group; *total: the sum.  (s_w: 4 words of LDS.)
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* s_w, unsigned long long* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();   // (s_w may still be read from a previous call)
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (int k = 0; k < kThreads / 64; ++k) {
        if (k < w) base += s_w[k];
        tot += s_w[k];
    }
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(kThreads) void k_seg_reduce(const float* __restrict__ T, const uint32_t* __restrict__ cnt, long long P,
                                                         SegDev* dev) {
    long long q = 0, n1 = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < P; i += (long long)gridDim.x * kThreads)
        if (cnt[i] >= 1u) { q += seg_q(T[i]); ++n1; }
    __shared__ long long s_q[kThreads / 64], s_n[kThreads / 64];
    q = wave_sum(q);
    n1 = wave_sum(n1);
    if ((threadIdx.x & 63) == 0) { s_q[threadIdx.x >> 6] = q; s_n[threadIdx.x >> 6] = n1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kThreads / 64; ++k) { q += s_q[k]; n1 += s_n[k]; }
        if (n1 > 0) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&dev->q_sum), (unsigned long long)q);
            atomicAdd(&dev->n1, (unsigned long long)n1);
        }
    }
}

__global__ void k_seg_mean(SegDev* dev) {
    const long long Q = dev->q_sum, n = (long long)dev->n1;
    long long mu = 0;
    if (n > 0) {
        mu = Q / n;
        if (Q % n != 0 && Q < 0) --mu;   // floor, not truncation
    }
    dev->mu = mu;
}

template <bool EIGHT>
__global__ __launch_bounds__(kThreads) void k_seg_tile(SegMask m, int R, int C, int32_t* __restrict__ lab, SegDev* dev) {
    __shared__ int s_L[kSegTilePx];
    __shared__ int s_fg[kThreads / 64];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * kSegTR, c0 = blockIdx.x * kSegTC;
    const long long mu = m.mask ? 0 : sload(&dev->mu);
    int nfg = 0;
#pragma unroll
    for (int j = 0; j < kSegTilePx / kThreads; ++j) {
        const int idx = j * kThreads + tid;
        const int gr = r0 + (idx >> 6), gc = c0 + (idx & 63);
        bool fg = false;
        if (gr < R && gc < C) {
            const size_t g = (size_t)gr * C + gc;
            if (m.mask) {
                fg = m.mask[g] != 0;
            } else if (m.cnt[g] >= m.min_count) {
                const long long q = seg_q(m.T[g]);
                fg = (!m.use_a && !m.use_b) || (m.use_a && q - mu > m.A) || (m.use_b && mu - q > m.B);
            }
        }
        s_L[idx] = fg ? idx : -1;
        nfg += fg;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSegTilePx / kThreads; ++j) {
        const int idx = j * kThreads + tid;
        if (s_L[idx] < 0) continue;   // (a foreground word never becomes negative)
        const int lr = idx >> 6, lc = idx & 63;
        if (lc > 0 && s_L[idx - 1] >= 0) lds_union(s_L, idx, idx - 1);
        if (lr > 0) {
            if (s_L[idx - kSegTC] >= 0) lds_union(s_L, idx, idx - kSegTC);
            if (EIGHT) {
                if (lc > 0 && s_L[idx - kSegTC - 1] >= 0) lds_union(s_L, idx, idx - kSegTC - 1);
                if (lc < kSegTC - 1 && s_L[idx - kSegTC + 1] >= 0) lds_union(s_L, idx, idx - kSegTC + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSegTilePx / kThreads; ++j) {
        const int idx = j * kThreads + tid;
        const int gr = r0 + (idx >> 6), gc = c0 + (idx & 63);
        if (gr >= R || gc >= C) continue;
        int out = -1;
        if (s_L[idx] >= 0) {
            const int root = lds_find(s_L, idx);
            out = (r0 + (root >> 6)) * C + (c0 + (root & 63));
        }
        lab[(size_t)gr * C + gc] = out;
    }
    nfg = (int)wave_sum((long long)nfg);
    if ((tid & 63) == 0) s_fg[tid >> 6] = nfg;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kThreads / 64; ++k) nfg += s_fg[k];
        if (nfg) atomicAdd(&dev->fg, (uint32_t)nfg);
    }
}

// threads 0 .. 63: the tile's top row; 64 .. 95: its left column; 96 .. 127: its right column
template <bool EIGHT>
__global__ __launch_bounds__(128) void k_seg_border(int32_t* lab, int R, int C) {
    const int r0 = blockIdx.y * kSegTR, c0 = blockIdx.x * kSegTC;
    const int t = threadIdx.x;
    int r, c;
    if (t < kSegTC) { r = r0; c = c0 + t; }
    else if (t < kSegTC + kSegTR) { r = r0 + (t - kSegTC); c = c0; }
    else { r = r0 + (t - kSegTC - kSegTR); c = c0 + kSegTC - 1; }
    if (r >= R || c >= C) return;
    const int p = r * C + c;
    if (g_load(lab + p) < 0) return;
    const bool top = (r == r0) && r > 0, left = (c == c0) && c > 0, right = (c == c0 + kSegTC - 1) && c + 1 < C;
    // a backward neighbour is in another tile iff the step to it leaves the tile's rows or columns
    if (left && g_load(lab + p - 1) >= 0) g_union(lab, p, p - 1);
    if (top && g_load(lab + p - C) >= 0) g_union(lab, p, p - C);
    if (EIGHT && r > 0) {
        if (c > 0 && (top || left) && g_load(lab + p - C - 1) >= 0) g_union(lab, p, p - C - 1);
        if (c + 1 < C && (top || right) && g_load(lab + p - C + 1) >= 0) g_union(lab, p, p - C + 1);
    }
}

__global__ __launch_bounds__(kThreads) void k_seg_flatten(int32_t* lab, int32_t* sz, long long P) {
    const long long base = ((long long)blockIdx.x * kThreads + threadIdx.x) * kSegRun;
    int cur = -1, run = 0;
    for (int j = 0; j < kSegRun; ++j) {
        const long long p = base + j;
        if (p >= P) break;
        int a = lab[p];
        if (a < 0) continue;   // (background does not end a run: the pixels beyond a gap mostly have the same root)
        // finite: a parent index only ever decreases, so the walk strictly descends
        for (;;) {
            const int q = lab[a];
            if (q == a) break;
            a = q;
        }
        lab[p] = a;
        if (a != cur) {
            if (cur >= 0) atomicAdd(&sz[cur], run);
            cur = a;
            run = 0;
        }
        ++run;
    }
    // the last run of every lane, folded per root over the wave: one atomic per distinct root.  (No lane has left the kernel.)
    for_each_wave_key(cur, [&](int k0, unsigned long long) {
        const long long n = wave_sum((long long)(cur == k0 ? run : 0));
        if ((threadIdx.x & 63) == 0) atomicAdd(&sz[k0], (int)n);
    });
}

// (found << 32 | kept) of the 8 consecutive pixels of a thread
__device__ __forceinline__ unsigned long long seg_rank_flags(const int32_t* lab, const int32_t* sz, long long base, long long P,
                                                            int min_pixels, uint32_t* keep_bits) {
    unsigned long long v = 0;
    uint32_t bits = 0;
    for (int j = 0; j < kSegRankPx / kThreads; ++j) {
        const long long p = base + j;
        if (p < P && lab[p] == (int)p) {
            v += 1ull << 32;
            if (sz[p] >= min_pixels) { v += 1; bits |= 1u << j; }
            bits |= 0x100u << j;
        }
    }
    *keep_bits = bits;
    return v;
}

__global__ __launch_bounds__(kThreads) void k_seg_count(const int32_t* __restrict__ lab, const int32_t* __restrict__ sz, long long P,
                                                        int min_pixels, unsigned long long* __restrict__ bc) {
    __shared__ unsigned long long s_w[kThreads / 64];
    const long long base = (long long)blockIdx.x * kSegRankPx + (long long)threadIdx.x * (kSegRankPx / kThreads);
    uint32_t bits;
    unsigned long long total;
    (void)block_excl_scan(seg_rank_flags(lab, sz, base, P, min_pixels, &bits), s_w, &total);
    if (threadIdx.x == 0) bc[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_seg_scan(unsigned long long* bc, int nb, SegDev* dev) {
    __shared__ unsigned long long s_w[kThreads / 64];
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kThreads) {
        const int i = b0 + threadIdx.x;
        const unsigned long long v = i < nb ? bc[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_excl_scan(v, s_w, &total);
        if (i < nb) bc[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        dev->found = (uint32_t)(carry >> 32);
        dev->kept = (uint32_t)carry;
    }
}

__global__ __launch_bounds__(kThreads) void k_seg_assign(const int32_t* __restrict__ lab, const int32_t* __restrict__ sz, long long P,
                                                         int min_pixels, const unsigned long long* __restrict__ bc,
                                                         int32_t* __restrict__ nid) {
    __shared__ unsigned long long s_w[kThreads / 64];
    const long long base = (long long)blockIdx.x * kSegRankPx + (long long)threadIdx.x * (kSegRankPx / kThreads);
    uint32_t bits;
    unsigned long long total;
    const unsigned long long ex = block_excl_scan(seg_rank_flags(lab, sz, base, P, min_pixels, &bits), s_w, &total);
    int next = (int)(uint32_t)(bc[blockIdx.x] + ex);   // (the low word: kept roots before this thread's pixels)
    for (int j = 0; j < kSegRankPx / kThreads; ++j) {
        if (!(bits & (0x100u << j))) continue;
        nid[base + j] = (bits & (1u << j)) ? next++ : -1;
    }
}

__global__ __launch_bounds__(kThreads) void k_seg_table_init(bf_component* table, int K) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= K) return;
    bf_component c;
    c.id = k; c.first_pixel = 0; c.pixels = 0; c.events = 0;
    c.row_min = INT_MAX; c.row_max = INT_MIN; c.col_min = INT_MAX; c.col_max = INT_MIN;
    c.row_sum = 0; c.col_sum = 0; c.q_sum = 0;
    table[k] = c;
}

// (in place: a thread reads lab only at its own pixel)
__global__ __launch_bounds__(kThreads) void k_seg_relabel(int32_t* lab, const int32_t* __restrict__ nid, long long P,
                                                          bf_component* table) {
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int l = lab[p];
    if (l < 0) return;
    const int k = nid[l];
    if (k >= 0 && l == (int)p) table[k].first_pixel = (int32_t)p;
    lab[p] = k;
}

struct SegAcc {
    int pixels, rmin, rmax, cmin, cmax;
    long long rsum, csum, qsum;
};
__device__ __forceinline__ void seg_acc_clear(SegAcc& a) {
    a.pixels = 0; a.rmin = INT_MAX; a.rmax = INT_MIN; a.cmin = INT_MAX; a.cmax = INT_MIN;
    a.rsum = 0; a.csum = 0; a.qsum = 0;
}
__device__ __forceinline__ void seg_acc_flush(bf_component* row, const SegAcc& a) {
    atomicAdd(&row->pixels, a.pixels);
    atomicMin(&row->row_min, a.rmin);
    atomicMax(&row->row_max, a.rmax);
    atomicMin(&row->col_min, a.cmin);
    atomicMax(&row->col_max, a.cmax);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->row_sum), (unsigned long long)a.rsum);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->col_sum), (unsigned long long)a.csum);
    if (a.qsum) atomicAdd(reinterpret_cast<unsigned long long*>(&row->q_sum), (unsigned long long)a.qsum);
}

__global__ __launch_bounds__(kThreads) void k_seg_stats(const int32_t* __restrict__ labels, const float* __restrict__ T, long long P,
                                                        int C, bf_component* table) {
    const long long base = ((long long)blockIdx.x * kThreads + threadIdx.x) * kSegRun;
    int r = 0, c = 0;
    if (base < P) { r = (int)(base / C); c = (int)(base - (long long)r * C); }
    int cur = -1;
    SegAcc a;
    seg_acc_clear(a);
    for (int j = 0; j < kSegRun; ++j) {
        const long long p = base + j;
        if (p >= P) break;
        const int k = labels[p];
        if (k >= 0) {   // (background does not end a run)
            if (k != cur) {
                if (cur >= 0) seg_acc_flush(table + cur, a);
                seg_acc_clear(a);
                cur = k;
            }
            ++a.pixels;
            a.rmin = min(a.rmin, r); a.rmax = max(a.rmax, r);
            a.cmin = min(a.cmin, c); a.cmax = max(a.cmax, c);
            a.rsum += r; a.csum += c;
            if (T) a.qsum += seg_q(T[p]);
        }
        if (++c == C) { c = 0; ++r; }
    }
    // the last run of every lane, folded per component over the wave with shuffles: one set of atomics per distinct component
    // (one inside a large one).  No lane has left the kernel.
    for_each_wave_key(cur, [&](int k0, unsigned long long) {
        SegAcc b;
        seg_acc_clear(b);
        if (cur == k0) b = a;
        b.pixels = (int)wave_sum((long long)b.pixels);
        b.rmin = wave_min(b.rmin); b.rmax = wave_max(b.rmax);
        b.cmin = wave_min(b.cmin); b.cmax = wave_max(b.cmax);
        b.rsum = wave_sum(b.rsum); b.csum = wave_sum(b.csum); b.qsum = wave_sum(b.qsum);
        if ((threadIdx.x & 63) == 0) seg_acc_flush(table + k0, b);
    });
}

constexpr int kSegEvPerThread = 4;   // events per thread of k_seg_events (a work-group's are consecutive per round)

__global__ __launch_bounds__(kThreads) void k_seg_events(SegEvents e, const int32_t* __restrict__ labels, int32_t* __restrict__ cl_id,
                                                         bf_component* table) {
    // counts of the wave, kept in (wave-uniform) registers while consecutive rounds name the same component
    int acc_key = -1, acc_cnt = 0;
    for (int j = 0; j < kSegEvPerThread; ++j) {
        const long long i = ((long long)blockIdx.x * kSegEvPerThread + j) * kThreads + threadIdx.x;
        int k = -1;
        if (i < e.n) {
            const uint32_t up = e.perm ? e.perm[i] : (uint32_t)i;
            if (!(e.noise && e.noise[up])) {
                const uint32_t v = e.xy[i];
                const float2 q = e.p[i];
                // accel_lib.h:154-158, as the scatter kernel forms it (bf_kernels.hip: event_body)
                const int X = trunc_scatter(pr_from_p(v & 0xffffu, q.x) * (double)e.scale + (double)e.x_sh);
                const int Y = trunc_scatter(pr_from_p(v >> 16, q.y) * (double)e.scale + (double)e.y_sh);
                const int hs = e.scale / 2;
                if (!((X >= e.wsx + hs) || (X < hs) || (Y >= e.wsy + hs) || (Y < hs))) k = labels[(size_t)X * (size_t)e.C + (size_t)Y];
            }
            cl_id[up] = k;
        }
        if (!table) continue;
        // one count per distinct component of the wave (`table` is a kernel argument: the whole wave is here or skipped it)
        for_each_wave_key(k, [&](int k0, unsigned long long same) {
            if (k0 != acc_key) {
                if (acc_cnt && (threadIdx.x & 63) == 0) atomicAdd(&table[acc_key].events, acc_cnt);
                acc_key = k0;
                acc_cnt = 0;
            }
            acc_cnt += __popcll(same);
        });
    }
    if (table && acc_cnt && (threadIdx.x & 63) == 0) atomicAdd(&table[acc_key].events, acc_cnt);
}

}  // namespace

void launch_seg_mean(const float* T, const uint32_t* cnt, long long P, SegDev* dev, hipStream_t s) {
    long long nb = (P + kThreads * 8 - 1) / (kThreads * 8);
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_seg_reduce, dim3((unsigned)nb), dim3(kThreads), 0, s, T, cnt, P, dev);
    hipLaunchKernelGGL(k_seg_mean, dim3(1), dim3(1), 0, s, dev);
}

void launch_seg_label(const SegMask& m, int R, int C, int connectivity, int32_t* lab, int32_t* sz, SegDev* dev, hipStream_t s) {
    const dim3 grid((unsigned)((C + kSegTC - 1) / kSegTC), (unsigned)((R + kSegTR - 1) / kSegTR));
    const long long P = (long long)R * C;
    if (connectivity == 8) {
        hipLaunchKernelGGL(k_seg_tile<true>, grid, dim3(kThreads), 0, s, m, R, C, lab, dev);
        hipLaunchKernelGGL(k_seg_border<true>, grid, dim3(128), 0, s, lab, R, C);
    } else {
        hipLaunchKernelGGL(k_seg_tile<false>, grid, dim3(kThreads), 0, s, m, R, C, lab, dev);
        hipLaunchKernelGGL(k_seg_border<false>, grid, dim3(128), 0, s, lab, R, C);
    }
    const long long per = (long long)kThreads * kSegRun;
    hipLaunchKernelGGL(k_seg_flatten, dim3((unsigned)((P + per - 1) / per)), dim3(kThreads), 0, s, lab, sz, P);
}

void launch_seg_rank(const int32_t* lab, const int32_t* sz, int32_t* nid, long long P, int min_pixels, unsigned long long* scratch,
                     SegDev* dev, hipStream_t s) {
    const int nb = seg_rank_blocks(P);
    hipLaunchKernelGGL(k_seg_count, dim3((unsigned)nb), dim3(kThreads), 0, s, lab, sz, P, min_pixels, scratch);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kThreads), 0, s, scratch, nb, dev);
    hipLaunchKernelGGL(k_seg_assign, dim3((unsigned)nb), dim3(kThreads), 0, s, lab, sz, P, min_pixels, scratch, nid);
}

void launch_seg_table(int32_t* lab, const int32_t* nid, const float* T, bf_component* table, int K, int R, int C, hipStream_t s) {
    const long long P = (long long)R * C;
    if (K > 0) hipLaunchKernelGGL(k_seg_table_init, dim3((unsigned)((K + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, table, K);
    hipLaunchKernelGGL(k_seg_relabel, dim3((unsigned)((P + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, lab, nid, P, table);
    if (K > 0) {
        const long long per = (long long)kThreads * kSegRun;
        hipLaunchKernelGGL(k_seg_stats, dim3((unsigned)((P + per - 1) / per)), dim3(kThreads), 0, s, lab, T, P, C, table);
    }
}

void launch_seg_events(const SegEvents& e, const int32_t* labels, int32_t* cl_id, bf_component* table, hipStream_t s) {
    if (e.n <= 0) return;
    const long long per = (long long)kThreads * kSegEvPerThread;
    hipLaunchKernelGGL(k_seg_events, dim3((unsigned)((e.n + per - 1) / per)), dim3(kThreads), 0, s, e, labels, cl_id, table);
}

}  // namespace bf
