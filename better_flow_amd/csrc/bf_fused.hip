// bf_fused.hip -- the one-kernel iteration (k_fused_pass): warp + scatter + stencil + moments of one image tile per work-group.
#include <atomic>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <limits.h>
#include <cstdlib>

#include "bf_fused_tile.h"

namespace bf {

// ---- the one-kernel iteration -----------------------------------------------------------------------------------------
// K1 and K3 in ONE launch for a slice context that has the GPU to itself (the latency regime: one iteration is a chain of
// two dependent launches there, ~20 us at 346x260 however few events the slice holds).  One work-group per image tile of
// TSR x 64 scaled pixels (TSR = 16 NSUB):
//   head     the pending model / loop update, by every work-group for itself (as k_bin_warp_scatter);
//   scatter  the tile's own events AND those of the neighbouring tiles' edge strips that face it (FusedTab: ten ranges of
//            the arrays sorted by (tile, zone)) are warped and added to an LDS tile with halo H = scale / 2 + 1.  Only the
//            owner of an event stores its new products -- into the OTHER product array (EvSetPtrs::p2, hot.pp), so that
//            the neighbours read the previous positions whatever the order the work-groups run in;
//   stencil  each 256-thread sub-group takes one 16 x 64 sub-tile -- the tile of k_stencil_binned, same thread -> pixel
//            mapping, same reduction tree: the f64 partial of a sub-tile, and with it the exact accumulators, carry the
//            bits of the two-kernel loop.
// No slabs, no overflow planes.  Exactness rests on every event that lands inside a tile's halo window being in that
// tile's ranges: true while no event has moved more than D since the sort.  The owner of an event CHECKS that from the
// zone it was sorted into and where it lands now; a violation raises `lost`, the next pass (or the re-bin, whichever comes
// first) sees it, the sums of that pass are dropped, and the pass is repeated on fresh bins (hot.redo) before the update
// runs -- late, never wrong.  The predictive re-bin (drift_limit) keeps that path rare.
// Packing: the scan sizes count << tbits | time sum for the fullest list; when even that does not fit 64 bits
// (hot.bin_ok == 0) the tile keeps separate u64 time sums and u32 counts.
// (pre_*: what the head's loads go through, as leading scalar arguments the command processor preloads -- see k_bin_warp_scatter)
template <int HS, int NSUB, int U>
__global__ __launch_bounds__(256 * NSUB) void k_fused_pass(const uint32_t* __restrict__ pre_ftab, const DevState* pre_st_in, MomentAcc* pre_acc_in,
                                                           const uint32_t* pre_lost, int pre_j, FusedArgs a) {
    using T = FusedTile<HS, NSUB>;   // the tile pass itself: bf_fused_tile.h
    constexpr int THREADS = T::THREADS, TR = T::TR, TC = T::TC, H = T::H, TSR = T::TSR;
    __shared__ unsigned long long s_rpart[NSUB][kSumFields * 4];
    __shared__ DevState s_state;
    const int b = blockIdx.x, tid = threadIdx.x;
    tl_stamp(a.tl, a.j, 0);
    // scalar loads first (see k_bin_warp_scatter), then the vector loads of the head, nothing consumed in between
    const HotState h0 = sload(&pre_st_in->hot);
    // (`lost`: three words by launch number mod 3 -- this pass reads its predecessor's, raises its own, clears its
    // successor's.  One shared word was read by late work-groups of a pass AFTER early ones of the same pass had raised it.)
    const uint32_t lost_prev = sload(pre_lost + (pre_j + 2) % 3);
    const FusedTab ft = sload(reinterpret_cast<const FusedTab*>(pre_ftab) + b);
    const FusedIndex index_of(ft);
    unsigned long long accv[kAccPerLane];
    if (tid < 64) acc_load_wave<false, false>(pre_acc_in, tid, accv);
    unsigned long long state_word = 0;
    if (tid < kStateWords) state_word = reinterpret_cast<const unsigned long long*>(pre_st_in)[tid];
    auto store_state = [&]() {   // work-group 0, after a barrier
        if (b == 0 && tid < kStateWords) {
            const unsigned long long v = reinterpret_cast<const unsigned long long*>(&s_state)[tid];
            reinterpret_cast<unsigned long long*>(a.st_out)[tid] = v;
            if (a.snap) reinterpret_cast<unsigned long long*>(a.snap)[tid] = v;
        }
    };
    auto clear_next_acc = [&]() {   // the accumulators the NEXT pass adds to (last read two passes ago), and its `lost` word
        if (b == 0 && tid < 64) {
            for (int i = tid; i < kAccGroups * 16; i += 64) (&a.acc_zero[0].f[0])[i] = 0ull;
            if (tid == 0) a.lost[(a.j + 1) % 3] = 0u;
        }
    };
    // A pass that does nothing: the loop is over, or it waits for a re-bin (need_rebin == 2), or the previous pass has
    // lost events -- then this one raises the request.
    const bool stalled = h0.need_rebin == 2;
    const bool trip = !h0.done && !stalled && lost_prev != 0u;
    if (h0.done || stalled || trip) {
        if (b != 0) return;
        if (tid < kStateWords) reinterpret_cast<unsigned long long*>(&s_state)[tid] = state_word;
        __syncthreads();
        if (tid == 0) {
            if (trip) { s_state.hot.need_rebin = 2; s_state.hot.redo = 1; s_state.hot.pend = 0; s_state.ovf_total += 1; }
            s_state.last_j = a.j;
        }
        __syncthreads();
        store_state();
        clear_next_acc();
        return;
    }
    const bool redo = h0.redo != 0;
    const bool pending = !redo && h0.pend != 0;
    const bool do_warp = a.warp && !redo;
    const EvSetPtrs ev = a.sets.s[h0.cs ^ h0.flip];
    const uint32_t* __restrict__ xy = ev.xy;
    const int32_t* __restrict__ t = ev.t;
    const float2* __restrict__ p_in = h0.pp ? ev.p2 : ev.p;
    float2* __restrict__ p_out = h0.pp ? ev.p : ev.p2;
    const int br = b / a.nbc, bc = b - br * a.nbc;
    const int X0 = br * TSR - H, Y0 = bc * TC - H;
    const uint32_t M = ft.total, own = ft.pre[1];
    uint32_t vxy[U], vi[U];
    int32_t vt[U];
    float2 vp[U];
    uint32_t base = 0;
    auto load_pass = [&]() {
#pragma unroll
        for (int k = 0; k < U; ++k) {
            uint32_t v = base + k * THREADS + tid;
            v = v < M ? v : 0u;
            const uint32_t i = index_of(ft, v);
            vi[k] = i;
            vxy[k] = xy[i];
            vt[k] = t[i];
            vp[k] = p_in[i];
        }
    };
    if (M) load_pass();
    asm volatile("" ::: "memory");
    T::clear(tid, THREADS, !h0.bin_ok);
    if (tid < kStateWords) reinterpret_cast<unsigned long long*>(&s_state)[tid] = state_word;
    double ppx[U], ppy[U];
    auto previous_positions = [&]() {
#pragma unroll
        for (int k = 0; k < U; ++k) {
            ppx[k] = pr_from_p(vxy[k] & 0xffffu, vp[k].x);
            ppy[k] = pr_from_p(vxy[k] >> 16, vp[k].y);
        }
    };
    tl_stamp(a.tl, a.j, 1);
    if (pending && tid < 64) {
        __builtin_amdgcn_s_setprio(3);
        const unsigned long long word = acc_reduce_wave(accv);
        __builtin_amdgcn_wave_barrier();
        tl_stamp(a.tl, a.j, 2);
        model_update_wave(&s_state, word, tid, 1);
        __builtin_amdgcn_s_setprio(0);
        tl_stamp(a.tl, a.j, 3);
    } else {
        previous_positions();
    }
    __syncthreads();
    tl_stamp(a.tl, a.j, 4);
    const ScatterHot hs = scatter_hot(&s_state);
    if (b == 0 && tid == 0) {   // bookkeeping only the stored state needs (fields the scatter does not read)
        if (pending) model_update_rest(&s_state, a.trace, 0, 0u);
        else if (s_state.hot.flip) { s_state.hot.cs ^= 1; s_state.hot.flip = 0; }   // (the commit model_update_rest would make)
        if (do_warp && !hs.done) s_state.hot.pp ^= 1;   // (a pass that finds the loop finished stores nothing)
        s_state.hot.redo = 0;
        s_state.hot.pend = hs.done ? 0 : 1;   // this pass's sums, unless the update has just ended the loop
        s_state.last_j = a.j;
    }
    if (hs.done) {
        __syncthreads();
        store_state();
        return;
    }
    if (pending && tid < 64) previous_positions();
    bool lost_here = false;
    for (;;) {
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t v = base + k * THREADS + tid;
            if (v >= M) continue;
            const bool mine = v < own;
            double px = ppx[k], py = ppy[k];
            if (do_warp) {
                float2 q;
                double nx, ny;
                warp_products(hs.wp, px, py, vt[k], q, nx, ny);
                if (mine)
                    __hip_atomic_store(reinterpret_cast<unsigned long long*>(&p_out[vi[k]]),
                                       ((unsigned long long)__float_as_uint(q.y) << 32) | (unsigned long long)__float_as_uint(q.x),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                px = pr_from_p(vxy[k] & 0xffffu, q.x);
                py = pr_from_p(vxy[k] >> 16, q.y);
            }
            lost_here |= T::scatter(px, py, vt[k], v, mine, ft, X0, Y0, hs);
        }
        base += THREADS * U;
        if (base >= M) break;
        load_pass();
        previous_positions();
    }
    if (lost_here) __hip_atomic_store(a.lost + a.j % 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tl_stamp(a.tl, a.j, 5);
    __syncthreads();
    tl_stamp(a.tl, a.j, 6);
    store_state();
    // ---- the stencil of k_stencil_binned, one 16 x 64 sub-tile per 256-thread sub-group, on the LDS tile ----
    const int g = tid >> 8, lt = tid & 255;
    const int R = a.R, C = a.C, hR = R / 2, hC = C / 2;
    const int r0 = br * TSR + g * TR, c0 = bc * TC;
    T::time_image(g, lt, r0, c0, R, C, hs);
    tl_stamp(a.tl, a.j, 7);
    __syncthreads();
    tl_stamp(a.tl, a.j, 8);
    const Sums sm = T::moments(g, lt, r0, c0, R, C);
    tl_stamp(a.tl, a.j, 9);
    block_reduce_publish<256, T::kPack>(sm, s_rpart[g], lt, r0 - hR, c0 - hC);
    tl_stamp(a.tl, a.j, 10);
    if (tid < 64) clear_next_acc();
    if (lt >= 64 || r0 >= R) return;   // (a sub-tile below the image has nothing to add)
    const Sums blk = block_reduce_total<256, T::kPack>(s_rpart[g], r0 - hR, c0 - hC);
    acc_add(a.acc_out, (b * NSUB + g) % kAccGroups, blk, lt);
    tl_stamp(a.tl, a.j, 11);
}

// One pass of the one-kernel iteration (k_fused_pass).
template <int HS, int NSUB>
static hipError_t launch_fused2(const FusedArgs& a, hipStream_t s) {
    constexpr int U = 4;
    using T = FusedTile<HS, NSUB>;
    if constexpr (T::kLds > 48 * 1024) {
        static std::atomic<unsigned long long> raised{0ull};
        const void* fns[1] = {reinterpret_cast<const void*>(&k_fused_pass<HS, NSUB, U>)};
        const hipError_t e = raise_dynamic_lds(raised, fns);
        if (e != hipSuccess) return e;
    }
    launch_timed(k_fused_pass<HS, NSUB, U>, dim3(a.nbr * a.nbc), dim3(T::THREADS), T::kLds, s, a.ftab, a.st_in, a.acc_in, a.lost, a.j, a);
    return hipSuccess;
}
// rows_per_tile: 32 or 64.
hipError_t launch_fused_pass(const FusedArgs& a, int half_scale, int rows_per_tile, hipStream_t s) {
    return dispatch_half_scale(half_scale, hipErrorInvalidValue, [&](auto hs) {
        constexpr int HS = decltype(hs)::value;
        return rows_per_tile == 64 ? launch_fused2<HS, 4>(a, s) : launch_fused2<HS, 2>(a, s);
    });
}

}  // namespace bf
