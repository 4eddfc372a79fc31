// bf_fused_tile.h -- the tile pass of the one-kernel iteration, ONCE: k_fused_pass (bf_fused.hip) and its persistent form
// k_fused_loop (bf_loop.hip) return the bits of the two-kernel loop because both run exactly this -- the LDS tile, the scatter
// of a warped event with the owner's check that no tile missed it, the time image and the moments of a sub-tile.  What the
// two kernels do around it (head update and accumulator atomics there; records, reducers and verdict here) stays with them.
#pragma once
#include <type_traits>

#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"

namespace bf {

// List entry v of a tile (its own events, then the neighbours' edge strips: FusedTab's ranges) -> global event index: off[0]
// plus the offset STEPS of the ranges the entry has passed.  (A chain of selects among the offsets themselves was turned into
// a select among ADDRESSES of a scratch copy of the table: a scratch load in front of every event load.)
struct FusedIndex {
    uint32_t step[kFusedRanges];
    __device__ __forceinline__ explicit FusedIndex(const FusedTab& ft) {
        step[0] = 0u;
#pragma unroll
        for (int r = 1; r < kFusedRanges; ++r) step[r] = ft.off[r] - ft.off[r - 1];
    }
    __device__ __forceinline__ uint32_t operator()(const FusedTab& ft, uint32_t v) const {
        uint32_t off = ft.off[0];
#pragma unroll
        for (int r = 1; r < kFusedRanges; ++r) off += v >= ft.pre[r] ? step[r] : 0u;
        return v + off;
    }
};

// One image tile of TSR x 64 scaled pixels (TSR = 16 NSUB) with halo H = HS + 1 in dynamic LDS, worked on by NSUB sub-groups
// of 256 threads: sub-group g owns the 16 x 64 sub-tile g -- the tile of k_stencil_binned, same thread -> pixel mapping.
template <int HS, int NSUB>
struct FusedTile {
    static constexpr int THREADS = 256 * NSUB;
    static constexpr int TR = kTileR, TC = kTileC;
    static constexpr int H = HS + 1;
    static constexpr int TSR = TR * NSUB;
    static constexpr int AR = TSR + 2 * H, AC = TC + 2 * H;   // the LDS tile
    static constexpr int TH = TR + 2, TW = TC + 2;            // a sub-tile's time image, with the Scharr ring
    static constexpr bool kPack = TR * TC <= 1024 && TR <= 64 && TC <= 64;   // (block_reduce_publish)
    // Dynamic LDS, the ONLY statement of its size: acc u64 [AR * AC] | time f32 [NSUB][TH * TW] | cnt u32 [AR * AC] (bin_ok == 0 only)
    static constexpr size_t kLds = (size_t)AR * AC * 12 + (size_t)NSUB * TH * TW * 4;
    static_assert(kLds + 4096 <= (size_t)kBinTileLdsMax, "the tile fits a CU");

    static __device__ __forceinline__ unsigned long long* acc() {
        extern __shared__ unsigned long long s_dyn[];   // (above 64 KiB for the 64-row tile: dynamic, see raise_dynamic_lds)
        return s_dyn;
    }
    static __device__ __forceinline__ float* time(int g) { return reinterpret_cast<float*>(acc() + AR * AC) + g * (TH * TW); }
    static __device__ __forceinline__ uint32_t* cnt() { return reinterpret_cast<uint32_t*>(time(NSUB)); }

    // zeroes the tile: threads i0, i0 + stride, ... of the work-group take part
    static __device__ __forceinline__ void clear(int i0, int stride, bool counts) {
        ulonglong2* z = reinterpret_cast<ulonglong2*>(acc());
        for (int i = i0; i < AR * AC / 2; i += stride) z[i] = make_ulonglong2(0ull, 0ull);
        if (counts)
            for (int i = i0; i < AR * AC; i += stride) cnt()[i] = 0u;
    }

    // Scatters list entry v, an event of time t that the warp left at (px, py), into the tile whose halo window starts at scaled
    // pixel (X0, Y0).  `mine`: this work-group owns the event -- then the answer is whether it was LOST: some tile whose halo
    // window holds its pixel does not read it.  The tile of its sort key does; the neighbours read the key's edge strips.
    static __device__ __forceinline__ bool scatter(double px, double py, int32_t t, uint32_t v, bool mine, const FusedTab& ft, int X0, int Y0,
                                                   const ScatterHot& hs) {
        const int hsc = hs.scale / 2;
        const int X = trunc_scatter(px * (double)hs.scale + (double)hs.x_sh);   // accel_lib.h:154-158
        const int Y = trunc_scatter(py * (double)hs.scale + (double)hs.y_sh);
        if ((X >= hs.wsx + hsc) || (X < hsc) || (Y >= hs.wsy + hsc) || (Y < hsc)) return false;
        const int lx = X - X0, ly = Y - Y0;
        if (lx >= 0 && lx < AR && ly >= 0 && ly < AC) {
            const unsigned long long dt = (unsigned long long)((long long)t - hs.tmin);
            if (hs.bin_ok) {   // packed: count << tbits | time sum
                atomicAdd(&acc()[lx * AC + ly], (1ull << hs.bin_tbits) + dt);
            } else {
                atomicAdd(&acc()[lx * AC + ly], dt);
                atomicAdd(&cnt()[lx * AC + ly], 1u);
            }
        }
        if (!mine) return false;
        const int dx = lx - H, dy = ly - H;   // the landing pixel relative to the key's tile
        if (!(dx < H || dx >= TSR - H || dy < H || dy >= TC - H)) return false;
        int z = 0;   // the zone the event was sorted into: C, TL, T, TR, R, BR, B, BL, L
#pragma unroll
        for (int q = 0; q < kFusedZones - 1; ++q) z += v >= ft.zone[q] ? 1 : 0;
        const bool top = (0x00eu >> z) & 1u, right = (0x038u >> z) & 1u, bottom = (0x0e0u >> z) & 1u, left = (0x182u >> z) & 1u;
        const bool ok = (dx >= H || top) && (dx < TSR - H || bottom) && dx >= H - TSR && dx < 2 * TSR - H &&
                        (dy >= H || left) && (dy < TC - H || right) && dy >= H - TC && dy < 2 * TC - H;
        return !ok;
    }

    // Time image of sub-tile g (image rows r0 .., columns c0 .., with a ring of one pixel) by its 256 threads, lt = 0 .. 255:
    // s x s box sum == the s x s splat of accel_lib.h:160-165 on integer planes, then time_from_sums.
    static __device__ __forceinline__ void time_image(int g, int lt, int r0, int c0, int R, int C, const ScatterHot& hs) {
        const bool packed = hs.bin_ok != 0;
        const int bt = hs.bin_tbits;
        const unsigned long long bm = (1ull << bt) - 1ull;
        const unsigned long long* win = acc() + (g * TR) * AC;   // rows r0 - H .. of this sub-tile
        const uint32_t* cwin = cnt() + (g * TR) * AC;
        for (int idx = lt; idx < TH * TW; idx += 256) {
            const int tr = idx / TW, tc = idx - tr * TW;
            const int gr = r0 - 1 + tr, gc = c0 - 1 + tc;
            float tv = 0.f;
            if (gr >= 0 && gr < R && gc >= 0 && gc < C) {
                unsigned long long pk = 0;
                uint32_t cacc = 0;
#pragma unroll
                for (int da = 0; da <= 2 * HS; ++da)
#pragma unroll
                    for (int db = 0; db <= 2 * HS; ++db) {
                        pk += win[(tr + da) * AC + (tc + db)];
                        if (!packed) cacc += cwin[(tr + da) * AC + (tc + db)];
                    }
                unsigned long long sum = pk;
                if (packed) { sum = pk & bm; cacc = (uint32_t)(pk >> bt); }
                tv = time_from_sums(cacc, (long long)sum, hs.tmin);
            }
            time(g)[idx] = tv;
        }
    }

    // Moments of sub-tile g from its time image (after a barrier): the stencil of k_stencil_binned, a thread's own pixels as
    // 32-bit integer sums (bf_device_fns.h).
    static __device__ __forceinline__ Sums moments(int g, int lt, int r0, int c0, int R, int C) {
        SumsT smt;
        sums_zero(smt);
        const int hR = R / 2, hC = C / 2;
#pragma unroll
        for (int k = 0; k < (TR * TC) / 256; ++k) {
            const int pidx = lt + k * 256;
            const int lr = pidx / TC, lc = pidx - lr * TC;
            const int gr = r0 + lr, gc = c0 + lc;
            if (gr < R && gc < C) {
                float gx, gy;
                stencil_px<TW>(&time(g)[(lr + 1) * TW + (lc + 1)], gr, gc, R, C, hR, hC, smt, gx, gy);
            }
        }
        return sums_widen(smt);
    }
};

// Calls f(std::integral_constant<int, HS>{}) for the compiled half scales 0 .. 4 (scales 1 .. 9: bf_plan.cpp); any other
// request is `bad`, never the nearest kernel.
template <class R, class F>
static inline R dispatch_half_scale(int half_scale, R bad, F&& f) {
    switch (half_scale) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return bad;
    }
}

}  // namespace bf
