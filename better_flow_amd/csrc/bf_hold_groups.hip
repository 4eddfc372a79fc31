// bf_hold_groups.hip -- the objects' per-event flow: the held flow of a grouping and its K models (bf_hold_groups) and the
// per-group median of a held flow (bf_group_flow_medians).  The definitions are in include/bf_accel.h ("the held flow of a
// grouping") and DESIGN.md section 19; the C-ABI around these kernels is in bf_global_search.cpp, next to the other holds.
// Plain launches on the context's stream; no work-group waits for another; the only atomics are integer adds without a return
// value, so no result depends on the order work-groups or waves run in.
//
//   H1 k_hold_groups   one thread per slot of the context's order: the id through perm, the K warps staged once per work-group
//                      in LDS and selected per lane, ONE warp from the reset state (warp_products, the scatter kernel's own),
//                      the products and the slot order kept per slot, (nx, ny) and uv_from_n of them at the upload index.
//   M1 k_median_count  one pass of an exact radix select over the 64-bit order keys of u and of v: per (group, axis) two targets,
//                      the ranks c/2 - 1 and c/2 (an odd count: c/2 twice).  Pass p counts digit p (8 bits, most significant
//                      first) of every value whose key matches its target's prefix so far: per work-group in LDS, one LDS add
//                      per distinct (target, digit) of the wave (for_each_wave_key), then one global add per non-zero word.
//                      The second target counts only once its prefix has left the first's: until then the first's table
//                      serves both.  A work-group's LDS holds the tables of kMedianChunk groups; blockIdx.y names the chunk.
//   M2 k_median_pick   one work-group, one wave per (group, axis) in turn: the digit under which each target's rank falls, the
//                      rank narrowed to that digit's values, the prefix extended.  The first pass yields the counts and sets
//                      the ranks; the last writes the medians.  The host enqueues the eight pairs and waits once.
#include <hip/hip_runtime.h>

#include "bf_assign.h"
#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_hold_groups.h"
#include "bf_kernels.h"

namespace bf {

namespace {

__global__ __launch_bounds__(kThreads) void k_hold_groups(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                          const uint32_t* __restrict__ perm, const int32_t* __restrict__ gid,
                                                          const WarpParams* __restrict__ wps, int K, long long n, GlobalHeld h) {
    __shared__ WarpParams s_wp[kAssignMaxModels];
    stage_warps_lds(s_wp, wps, K);
    __syncthreads();
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long e = perm ? (long long)perm[i] : i;
    const int g = gid[e];
    const uint32_t v = xy[i];
    float2 q = make_float2(0.0f, 0.0f);   // (an event of no group: zero flow, zero products, pr = fr)
    double2 nn = make_double2(0.0, 0.0);
    if (g >= 0 && g < K) {
        // Event::reset (pr = fr), then set_model's warp_reinit of the event's own model
        warp_products(s_wp[g], (double)(v & 0xffffu), (double)(v >> 16), t[i], q, nn.x, nn.y);
    }
    h.p[i] = q;
    h.xy[i] = v;
    h.idx[i] = (uint32_t)e;
    h.nxny[e] = nn;
    h.uv[e] = uv_from_n(nn);
}

// The total order of the doubles as unsigned keys: negative values reversed below the positive ones, -0.0 below +0.0.
__device__ __forceinline__ unsigned long long median_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double median_value(unsigned long long key) {
    const unsigned long long b = (key >> 63) ? key ^ (1ull << 63) : ~key;
    return __longlong_as_double((long long)b);
}

constexpr int kMedianEv = 16;   // events per thread: a work-group's are consecutive per round

__global__ __launch_bounds__(kThreads) void k_median_count(const double2* __restrict__ uv, const int32_t* __restrict__ gid,
                                                           long long n, int K, int pass, MedianState st) {
    __shared__ uint32_t s_hist[kMedianChunk * 4 * 256];
    __shared__ unsigned long long s_prefix[kMedianChunk * 4];
    const int g0 = (int)blockIdx.y * kMedianChunk;
    const int gn = min(K - g0, kMedianChunk);   // groups of this chunk (>= 1: the grid has ceil(K / chunk) rows)
    const int words = gn * 4 * 256;
    for (int w = threadIdx.x; w < words; w += kThreads) s_hist[w] = 0u;
    for (int w = threadIdx.x; w < gn * 4; w += kThreads) s_prefix[w] = st.prefix[g0 * 4 + w];
    __syncthreads();
    const int shift = 56 - 8 * pass;
    for (int r = 0; r < kMedianEv; ++r) {   // (wave-uniform: every lane reaches every for_each_wave_key)
        const long long i = ((long long)blockIdx.x * kMedianEv + r) * kThreads + threadIdx.x;
        int lg = -1;
        if (i < n) {
            const int g = gid[i];
            if (g >= g0 && g < g0 + gn) lg = g - g0;
        }
        double2 f = make_double2(0.0, 0.0);
        if (lg >= 0) f = uv[i];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const unsigned long long key = median_key(a ? f.y : f.x);
            const int digit = (int)((key >> shift) & 255u);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int slot = -1;
                if (lg >= 0) {
                    const int T = (lg * 2 + a) * 2 + j;
                    const unsigned long long pf = s_prefix[T];
                    // (the high `8 * pass` bits of the key against the target's; pass 0: every value matches)
                    const bool match = pass == 0 || ((key ^ pf) >> (shift + 8)) == 0;
                    const bool own = j == 0 || pf != s_prefix[T - 1];
                    if (match && own) slot = T * 256 + digit;
                }
                for_each_wave_key(slot, [&](int k0, unsigned long long same) {
                    if ((threadIdx.x & 63) == 0) atomicAdd(&s_hist[k0], (uint32_t)__popcll(same));
                });
            }
        }
    }
    __syncthreads();
    uint32_t* hist = st.hist + (size_t)g0 * 4 * 256;
    for (int w = threadIdx.x; w < words; w += kThreads) {
        const uint32_t c = s_hist[w];
        if (c) atomicAdd(hist + w, c);
    }
}

// The digit of one table (256 counts) under which rank r falls, by the whole wave: lane l holds digits 4 l .. 4 l + 3.  Returns
// the digit and narrows r to the rank among that digit's values; `total` gets the table's sum.  A table of zeros gives digit 0.
__device__ __forceinline__ int median_pick_digit(const uint32_t* __restrict__ table, uint32_t& r, uint32_t& total) {
    const int lane = threadIdx.x & 63;
    const uint4 c = reinterpret_cast<const uint4*>(table)[lane];
    const uint32_t mine = c.x + c.y + c.z + c.w;
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    total = __shfl(incl, 63, 64);
    const unsigned long long above = __ballot(r < incl);
    if (!above) return 0;
    const int L = __ffsll((long long)above) - 1;
    uint32_t below = incl - mine;   // values under this lane's first digit
    int d = 4 * lane;
    const uint32_t q[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (d == 4 * lane + k && r >= below + q[k]) { below += q[k]; ++d; }
    d = __shfl(d, L, 64);
    r -= (uint32_t)__shfl((int)below, L, 64);
    return d;
}

constexpr int kPickThreads = 1024;

__global__ __launch_bounds__(kPickThreads) void k_median_pick(int K, int pass, MedianState st) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int shift = 56 - 8 * pass;
    for (int pair = wave; pair < 2 * K; pair += kPickThreads / 64) {   // pair = group * 2 + axis (wave-uniform)
        const int T0 = pair * 2, T1 = T0 + 1;
        const unsigned long long p0 = st.prefix[T0], p1 = st.prefix[T1];
        uint32_t r0 = st.rank[T0], r1 = st.rank[T1];
        uint32_t c = st.count[pair];
        if (pass == 0) {   // the first table of the pair holds every value of the group: its sum is the count
            uint32_t zero = 0;
            (void)median_pick_digit(st.hist + (size_t)T0 * 256, zero, c);
            r1 = c / 2;
            r0 = (c & 1u) ? r1 : (c ? r1 - 1 : 0u);
        }
        uint32_t unused;
        const int d0 = median_pick_digit(st.hist + (size_t)T0 * 256, r0, unused);
        const int d1 = median_pick_digit(st.hist + (size_t)(p0 == p1 ? T0 : T1) * 256, r1, unused);
        const unsigned long long n0 = p0 | ((unsigned long long)d0 << shift), n1 = p1 | ((unsigned long long)d1 << shift);
        if (lane == 0) {
            st.prefix[T0] = n0; st.prefix[T1] = n1;
            st.rank[T0] = r0; st.rank[T1] = r1;
            if (pass == 0) st.count[pair] = c;
            if (pass == 7) {
                const double a = median_value(n0), b = median_value(n1);
                // (an odd count: both targets are the element c / 2)
                st.median[pair] = c == 0 ? 0.0 : ((c & 1u) ? b : 0.5 * (a + b));
            }
        }
    }
}

}  // namespace

void launch_hold_groups(const uint32_t* xy, const int32_t* t, const uint32_t* perm, const int32_t* gid, const WarpParams* wp,
                        int K, long long n, const GlobalHeld& h, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_hold_groups, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, xy, t, perm, gid, wp,
                       K, n, h);
}

void launch_median_pass(const double2* uv, const int32_t* gid, long long n, int K, int pass, const MedianState& st, hipStream_t s) {
    if (n > 0) {
        const long long per = (long long)kThreads * kMedianEv;
        const dim3 grid((unsigned)((n + per - 1) / per), (unsigned)((K + kMedianChunk - 1) / kMedianChunk));
        hipLaunchKernelGGL(k_median_count, grid, dim3(kThreads), 0, s, uv, gid, n, K, pass, st);
    }
    hipLaunchKernelGGL(k_median_pick, dim3(1), dim3(kPickThreads), 0, s, K, pass, st);
}

}  // namespace bf
