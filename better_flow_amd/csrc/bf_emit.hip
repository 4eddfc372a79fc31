// bf_emit.hip -- the -o table accumulated on the device (DVS_flow::get_accumulated, dvs_flow.h:351-389; the host
// restatement is StreamEngine::get_accumulated, stream_flow.h): the rows a solved slice contributes, in upload order,
// from the context's committed slice and its per-event flow.  The C-ABI and the state it keeps are in bf_emit_abi.cpp.
//
// One slice is M = lead + n elements: element 0 is the slice's lead event when it has one (the ring's oldest element,
// left out of the slice, never in a slice before), element lead + i is upload index i.  Five launches on the context stream:
//   k_emit_decide  per element: logical timestamp, address, and the decision -- emitted iff not covered as of before this
//                  slice (covered plane, or the per-pixel tail of an earlier slice) and not the slice-local t == -1 mark;
//                  the lead is always emitted.  Writes a sort key (pixel << jbits | element: only the bits that vary).
//   radix sort     of the keys: the same-pixel chains of the slice in arrival order, one run per pixel (rocPRIM).
//   k_emit_cover   per element: covered after this slice = covered before, or emitted, or an emitted element of its run
//                  within the host rule's reach -- a later one less than 0.1 ms after it, or an earlier one at the same
//                  instant (the host walks the chains the other way; see below).  Writes the covered plane of the slice's
//                  ring positions and the tail of the pixels emitted at the slice's newest timestamp.
//   scan + k_emit_rows  output positions of the emitted elements, and their rows (t, row, col, u, v) -- written straight into
//                  the pinned output ring on the host, from the running row offset the previous slice left on the device.
// The covered plane is read only in k_emit_decide and written only in k_emit_cover, a launch later: every decision of a
// slice sees the state from before the slice, whatever order its threads run in.
//
// Why pulling the marks is the host's pushing: for non-decreasing timestamps, an emitted g marks the same-pixel c with
// c < g and t(g) - t(c) < 0.1 ms (the prev chain stops at the first one out of reach, and every one before it is further
// away) and c > g with t(c) == t(g) (the next chain stops at the first later timestamp).  So c is marked by the emitted
// elements of its run that lie after it while the time difference stays below 0.1 ms, and before it while the timestamp
// is equal -- exactly what k_emit_cover walks.  Marks on events after the slice's end can only hit events at the slice's
// newest timestamp T (t(g) <= T <= t(c) = t(g)), the timestamp of its last element: the per-pixel tail (T, last event of
// the slice) stands for them.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "bf_device.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr unsigned long long kNone = ~0ull;
constexpr unsigned long long kReach = 100000ull;   // Event::operator== (event.h:39-45): |dt| < 0.1 ms

__global__ __launch_bounds__(kThreads) void k_emit_decide(EmitSlice a) {
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k == 0 && a.lead) {
        const bool inside = a.lead_row < (uint32_t)a.rows && a.lead_col < (uint32_t)a.cols;
        const uint32_t pix = inside ? a.lead_row * (uint32_t)a.cols + a.lead_col : 0;
        if (!inside) atomicOr(a.err, 1u);
        a.t[0] = a.lead_t;
        a.rc[0] = (a.lead_row & 0xffffu) | (a.lead_col << 16);
        a.flag[0] = 1;   // emitted, never written to the plane (it is older than the slice)
        a.keys[0] = (unsigned long long)pix << a.jbits;
    }
    if (k >= a.n) return;
    const uint32_t up = a.perm ? a.perm[k] : (uint32_t)k;   // slot k of the live set holds upload index perm[k]
    const uint32_t xy = a.xy[k];
    const uint32_t row = xy & 0xffffu, col = xy >> 16;
    const int32_t tl = a.tloc[k];
    const unsigned long long t = a.start_time + (unsigned long long)(long long)tl;   // Event::set_local_time undone
    const unsigned long long g = a.first + up;
    uint32_t pix = 0;
    bool cov = false;
    if (row >= (uint32_t)a.rows || col >= (uint32_t)a.cols) {
        atomicOr(a.err, 1u);
    } else {
        pix = row * (uint32_t)a.cols + col;
        if (g < a.prev_end) cov = a.plane[g % a.cap] != 0;
        const unsigned long long ta = a.tail_g[pix];
        if (ta != kNone && g > ta && t == a.tail_t[pix]) cov = true;
    }
    const uint32_t j = up + (uint32_t)a.lead;
    a.t[j] = t;
    a.rc[j] = xy;
    a.flag[j] = (uint8_t)((cov || tl == -1 ? 0 : 1) | (cov ? 2 : 0));
    a.keys[j] = ((unsigned long long)pix << a.jbits) | j;
}

__global__ __launch_bounds__(kThreads) void k_emit_cover(EmitSlice a, const unsigned long long* __restrict__ sorted) {
    const long long s = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long m = a.n + a.lead;
    if (s >= m) return;
    const unsigned long long key = sorted[s];
    const unsigned long long jmask = (1ull << a.jbits) - 1;
    const uint32_t j = (uint32_t)(key & jmask), pix = (uint32_t)(key >> a.jbits);
    const unsigned long long t = a.t[j];
    const uint8_t f = a.flag[j];
    if ((f & 1) && t == a.t[m - 1]) {   // marks beyond the slice's end: the tail of this pixel (an older tail at the same T covers more)
        if (a.tail_g[pix] == kNone || a.tail_t[pix] != t) { a.tail_t[pix] = t; a.tail_g[pix] = a.last; }
    }
    if (j < (uint32_t)a.lead) return;   // the lead's ring position is never read again
    bool cov = f != 0;
    for (long long q = s + 1; !cov && q < m; ++q) {   // later arrivals at this pixel, less than 0.1 ms after it
        const unsigned long long kq = sorted[q];
        if ((uint32_t)(kq >> a.jbits) != pix) break;
        const uint32_t jq = (uint32_t)(kq & jmask);
        if (a.t[jq] - t >= kReach) break;
        cov = (a.flag[jq] & 1) != 0;
    }
    for (long long q = s - 1; !cov && q >= 0; --q) {   // earlier arrivals at this pixel, same instant
        const unsigned long long kq = sorted[q];
        if ((uint32_t)(kq >> a.jbits) != pix) break;
        const uint32_t jq = (uint32_t)(kq & jmask);
        if (a.t[jq] != t) break;
        cov = (a.flag[jq] & 1) != 0;
    }
    a.plane[(a.first + (j - (uint32_t)a.lead)) % a.cap] = cov ? 1 : 0;
}

struct EmittedBit {
    __device__ __host__ uint32_t operator()(uint8_t f) const { return f & 1u; }
};

__global__ __launch_bounds__(kThreads) void k_emit_rows(EmitSlice a) {
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long m = a.n + a.lead;
    if (j >= m) return;
    const unsigned long long base = *a.off_in;
    const uint8_t f = a.flag[j];
    if (j == m - 1) {   // (off_in and off_out are two words: nobody reads what this writes before the next slice)
        const unsigned long long rows = a.pos[j] + (f & 1u);
        *a.off_out = base + rows;
        a.rec[0] = base; a.rec[1] = rows; a.rec[2] = *a.err;
    }
    if (!(f & 1)) return;
    const unsigned long long r = (base + a.pos[j]) % a.out_rows;
    const uint32_t rc = a.rc[j];
    a.out_t[r] = a.t[j];
    a.out_row[r] = (uint16_t)(rc & 0xffffu);
    a.out_col[r] = (uint16_t)(rc >> 16);
    double u = 0.0, v = 0.0;   // the lead: the zero flow of a fresh Event; a slice without a warp: Event::reset
    if (j >= a.lead && a.uv) {
        const double2 w = a.uv[j - a.lead];
        u = w.x; v = w.y;
    }
    a.out_u[r] = u;
    a.out_v[r] = v;
}

}  // namespace

size_t emit_temp_bytes(long long m) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_keys(nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned int)m);
    (void)rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator((const uint8_t*)nullptr, EmittedBit()), (uint32_t*)nullptr,
                                  0u, (size_t)m, rocprim::plus<uint32_t>());
    return a > b ? a : b;
}

hipError_t launch_emit(const EmitSlice& a, unsigned long long* keys_sorted, void* temp, size_t temp_bytes, hipStream_t s) {
    const long long m = a.n + a.lead;
    const unsigned grid = (unsigned)((m + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_emit_decide, dim3(grid), dim3(kThreads), 0, s, a);
    hipError_t e = rocprim::radix_sort_keys(temp, temp_bytes, a.keys, keys_sorted, (unsigned int)m, 0, (unsigned)a.kbits, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_emit_cover, dim3(grid), dim3(kThreads), 0, s, a, (const unsigned long long*)keys_sorted);
    e = rocprim::exclusive_scan(temp, temp_bytes, rocprim::make_transform_iterator((const uint8_t*)a.flag, EmittedBit()), a.pos, 0u,
                                (size_t)m, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_emit_rows, dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace bf
