// bf_groups_wide.hip -- bf_run_groups, "groups_wide": the two copies around the chip-wide loop of a group whose window does not
// fit one work-group's LDS.  The group's events are one bucket of the sorted set (slots beg .. beg + n); the loop itself is
// bf_run on the inner context (bf_tiles_abi.cpp: run_wide_group), which takes the bucket as its slice -- upload index j is
// bucket slot beg + j.  The definition is in include/bf_accel.h ("wide groups") and DESIGN.md section 21.
// Plain launches on the context's stream, vector stores only, no atomics; no work-group waits for another.
//
//   W1 k_group_gather        one thread per kWideEv consecutive slots of the bucket: the address word unpacked into the int32 row
//                            and column, the time copied -- the three staging columns k_prepare reads (16-byte stores: the
//                            columns start aligned and a thread's first slot is a multiple of four).
//   W2 k_group_scatter_back  one thread per kWideEv consecutive slots of the INNER context's order: through the inner permutation
//                            to the bucket slot, the products to the outer set's slot, (nx, ny) through the outer permutation to
//                            the event's upload index.  The inner (nx, ny) are read where the inner run left them: in slot order
//                            behind its final warp, else in its upload order; none (no warp ran): zeros.
#include <hip/hip_runtime.h>

#include "bf_device.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr int kWideEv = 4;   // consecutive slots per thread

__global__ __launch_bounds__(kThreads) void k_group_gather(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                           uint32_t beg, uint32_t n, int32_t* __restrict__ ox,
                                                           int32_t* __restrict__ oy, int32_t* __restrict__ ot) {
    const uint32_t j0 = ((uint32_t)blockIdx.x * kThreads + threadIdx.x) * kWideEv;
    if (j0 >= n) return;
    if (j0 + kWideEv <= n) {
        int32_t x[kWideEv], y[kWideEv], tt[kWideEv];
#pragma unroll
        for (int k = 0; k < kWideEv; ++k) {
            const uint32_t v = xy[beg + j0 + k];
            x[k] = (int32_t)(v & 0xffffu);
            y[k] = (int32_t)(v >> 16);
            tt[k] = t[beg + j0 + k];
        }
        *reinterpret_cast<int4*>(ox + j0) = make_int4(x[0], x[1], x[2], x[3]);
        *reinterpret_cast<int4*>(oy + j0) = make_int4(y[0], y[1], y[2], y[3]);
        *reinterpret_cast<int4*>(ot + j0) = make_int4(tt[0], tt[1], tt[2], tt[3]);
    } else {
        for (uint32_t j = j0; j < n; ++j) {
            const uint32_t v = xy[beg + j];
            ox[j] = (int32_t)(v & 0xffffu);
            oy[j] = (int32_t)(v >> 16);
            ot[j] = t[beg + j];
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_group_scatter_back(WideBack a) {
    const uint32_t k0 = ((uint32_t)blockIdx.x * kThreads + threadIdx.x) * kWideEv;
#pragma unroll
    for (int e = 0; e < kWideEv; ++e) {
        const uint32_t k = k0 + e;
        if (k >= a.n) return;
        const uint32_t j = a.in_perm ? a.in_perm[k] : k;
        if (j >= a.n) continue;   // (cannot be: the inner permutation is one of 0 .. n - 1)
        const uint32_t slot = a.beg + j;
        a.out_p[slot] = a.in_p[k];
        double2 nn = make_double2(0.0, 0.0);
        if (a.in_nxny) nn = a.in_nxny[a.in_nxny_by_slot ? k : j];
        a.out_nxny[a.out_perm[slot]] = nn;
    }
}

}  // namespace

void launch_group_gather(const uint32_t* xy, const int32_t* t, uint32_t beg, uint32_t n, int32_t* ox, int32_t* oy, int32_t* ot,
                         hipStream_t s) {
    if (n == 0) return;
    const uint32_t per = (uint32_t)kThreads * kWideEv;
    hipLaunchKernelGGL(k_group_gather, dim3((n + per - 1) / per), dim3(kThreads), 0, s, xy, t, beg, n, ox, oy, ot);
}

void launch_group_scatter_back(const WideBack& a, hipStream_t s) {
    if (a.n == 0) return;
    const uint32_t per = (uint32_t)kThreads * kWideEv;
    hipLaunchKernelGGL(k_group_scatter_back, dim3((a.n + per - 1) / per), dim3(kThreads), 0, s, a);
}

}  // namespace bf
