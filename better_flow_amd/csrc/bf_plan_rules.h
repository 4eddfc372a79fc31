// bf_plan_rules.h -- the arithmetic that picks the kernel variants of the two-kernel tile-binned loop, as pure functions of plain
// numbers: no bf_ctx, no HIP, nothing but <cstddef> / <cstdint> and the ABI's constants.  bf_plan.cpp (plan_slice, plan_run), the launchers
// (launch_bin_warp_scatter, launch_stencil_binned) and bf_run's record of what it launched (bf_get_stat "k1_*" / "k3_*") all
// call these, so the plan, the dispatch and the report cannot disagree; tests/cpp/test_plan.cpp sweeps them on the host and
// holds the set of variants they can return to tests/variants_reachable.txt.  Why each threshold is what it is stands next to
// its caller in bf_plan.cpp -- the measurements stay there.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/bf_accel.h"   // BF_LOOP_*

namespace bf_rules {

// Margins of the tile-binned loops, in scaled pixels: how far an event may drift from where the counting sort found it before
// its bin must be re-sorted.  Swept flat over 4 .. 8 in rounds 3 and 4 (EXPERIMENTS: 195.9 / 195.1 / 193.1 Mevents/s at 8 / 6 / 4),
// so no longer an option.
constexpr int kBinMargin = 8;      // two-kernel loop: D of BinShape (capped at half the smaller tile side)
constexpr int kFusedMargin = 8;    // one-kernel loops: D on top of the stencil halo H = scale / 2 + 1
constexpr int kBinTileLdsMax = 156 * 1024;   // dynamic LDS of a scatter work-group (160 KiB per CU minus its static part)
constexpr int kMaxBins = 8192;
constexpr int kStencilTileR = 16, kStencilTileC = 64;   // (bf_device.h: kTileR, kTileC)

// the margin the bin grid is built with: kBinMargin, or the test hook's value rounded up to even
inline int bin_margin(int debug_margin) { return debug_margin > 0 ? ((debug_margin + 1) & ~1) : kBinMargin; }

// ---- tile shape -----------------------------------------------------------------------------------------------------------
struct BinShape {
    int TS = 64, TSR = 64;   // columns (a power of two) and rows of a bin
    int D = 0;               // margin, <= min(TS, TSR) / 2
    int nbr = 0, nbc = 0, nbins = 0;
    int L() const { return TS + 2 * D; }
    int LR() const { return TSR + 2 * D; }
};

// The cost model of plan_slice: n events on an image of R x C scaled pixels, one work-group per bin on n_cus CUs.
inline BinShape bin_shape(long long n, int R, int C, int n_cus, int margin) {
    BinShape g;
    if (n_cus > 0) {
        const double density = (double)n / ((double)R * (double)C);
        double best = -1.0;
        int best_area = 0;
        for (int cols = 16; cols <= 64; cols *= 2) {
            for (int rows = 32; rows <= 128; rows += 16) {
                const int d = margin > cols / 2 ? cols / 2 : margin;
                if ((size_t)(rows + 2 * d) * (cols + 2 * d) * 8 > 64 * 1024) continue;
                const int nb = ((R + rows - 1) / rows) * ((C + cols - 1) / cols);
                if (nb > kMaxBins) continue;
                const double cost = (double)((nb + n_cus - 1) / n_cus) * rows * cols * density * 1.7e-3 +
                                    (double)nb * (rows + 2 * d) * (cols + 2 * d) * 2.3e-6;
                if (best < 0 || cost < best * 0.999 || (cost <= best * 1.001 && rows * cols > best_area)) {
                    best = cost; best_area = rows * cols; g.TS = cols; g.TSR = rows;
                }
            }
        }
    }
    const int tmin = g.TS < g.TSR ? g.TS : g.TSR;
    g.D = margin > tmin / 2 ? tmin / 2 : margin;   // <= 2 x 2 bins per pixel
    g.nbc = (C + g.TS - 1) / g.TS;
    g.nbr = (R + g.TSR - 1) / g.TSR;
    g.nbins = g.nbr * g.nbc;
    return g;
}

// Can the two-kernel tile-binned loop run on this grid at all (plan_slice; the options, the noise mask and the event capacity aside)?
inline bool bin_grid_ok(const BinShape& g, int R) {
    return g.nbins <= kMaxBins && (size_t)g.LR() * g.L() * 8 <= (size_t)kBinTileLdsMax && R < (1 << 20);
}
// ... and can it carry this scatter format: 0 dense slabs, 2 event lists (16-bit tile-local pixel indices), 3 own pixels + margin
// plane (D a power of two >= 2)?
inline bool bin_format_ok(const BinShape& g, int fmt) {
    if (fmt == 0) return true;
    if (fmt == 2) return (size_t)g.LR() * (size_t)g.L() <= 65536;
    if (fmt == 3) return g.D >= 2 && (g.D & (g.D - 1)) == 0 && g.TS >= 4;
    return false;
}

// ---- scatter kernel (bf_scatter.hip: k_bin_warp_scatter / k_bin_warp_scatter_lean) -----------------------------------------
struct ScatterSize {
    int threads = 0;      // work-group size
    int per_thread = 0;   // events a thread keeps in flight, as launched
};

// `head`: the update runs at the head of the scatter launch (a context that has the GPU to itself), else the lean kernel.
inline ScatterSize scatter_size(int fmt, bool head, int nbins, long long n, int n_cus) {
    ScatterSize s;
    const double ev_per_bin = (double)n / (double)(nbins > 0 ? nbins : 1);
    const bool many_small_bins = fmt == 2 && n_cus > 0 && nbins >= 4 * n_cus && ev_per_bin < 1024.0;
    if (fmt == 2) s.threads = many_small_bins ? 256 : 512;
    else s.threads = (head && ev_per_bin >= 1536.0) ? 1024 : 512;
    const double per_bin = (fmt == 2 ? 1.0 : 1.1) * ev_per_bin / (double)s.threads;
    s.per_thread = per_bin <= 1 ? 1 : (per_bin <= 2.83 ? 2 : (per_bin <= 4 ? 4 : 8));
    if (fmt == 0 && s.threads == 512 && per_bin > 6.5) s.per_thread = per_bin <= 8.2 ? 10 : 12;
    if (fmt == 2 && !head && s.threads == 256 && per_bin > 2.0) s.per_thread = 4;
    return s;
}

// Is (head, threads, per_thread, fmt) one of the compiled instantiations?  These are exactly the tuples scatter_size can return
// (tests/variants_reachable.txt); launch_bin_warp_scatter refuses every other request with hipErrorInvalidValue.
//     event lists:                               256 threads x 1, 2, 4;  512 x 1, 2, 4, 8;              either form
//     dense slabs, own pixels + margin plane:    head 512 x 1, 2, 4;  head 1024 x 2, 4, 8;  lean 512 x 1, 2, 4, 8
//     dense slabs only:                          lean 512 x 10, 12
inline bool scatter_compiled(bool head, int threads, int per_thread, int fmt) {
    const int u = per_thread;
    const bool u124 = u == 1 || u == 2 || u == 4;
    if (fmt == 2) return (threads == 256 && u124) || (threads == 512 && (u124 || u == 8));
    if (fmt != 0 && fmt != 3) return false;
    if (head) return (threads == 512 && u124) || (threads == 1024 && (u == 2 || u == 4 || u == 8));
    return threads == 512 && (u124 || u == 8 || (fmt == 0 && (u == 10 || u == 12)));
}

// ---- stencil kernel (bf_stencil.hip: k_stencil_binned / k_stencil_binned_full) ---------------------------------------------
inline long long stencil_tiles(int R, int C) {
    return (long long)((C + kStencilTileC - 1) / kStencilTileC) * (long long)((R + kStencilTileR - 1) / kStencilTileR);
}
// the build with the scalar registers capped: a launch with more work-groups than the CUs hold at once
inline bool stencil_capped(long long tiles, int n_cus) { return n_cus > 0 && tiles >= 8ll * n_cus; }
// Which tile a work-group of the stencil launch takes: work-groups b, b + 8, b + 16, ... (one residue class mod kTileClasses --
// what has been observed to share an L2, never relied on for a result) take ONE contiguous run of row-major tile indices, i.e. a
// band of tile rows, so that the halo rows and columns two neighbouring tiles both read are fetched by work-groups of one class.
// A bijection on [0, ntiles) for every ntiles >= 1: class x holds per + (x < rem) tiles and starts at x per + min(x, rem).
// BF_RULES_HD: the stencil kernel calls it too (uniform: scalar unit; the division by 8 is a shift).
#if defined(__HIPCC__)
#define BF_RULES_HD __host__ __device__
#else
#define BF_RULES_HD
#endif
constexpr int kTileClasses = 8;
BF_RULES_HD inline int tile_of_block(int b, int ntiles) {
    const unsigned x = (unsigned)b % kTileClasses, j = (unsigned)b / kTileClasses;   // (0 <= b < ntiles: shifts and masks)
    const unsigned per = (unsigned)ntiles / kTileClasses, rem = (unsigned)ntiles % kTileClasses;
    return (int)(x * per + (x < rem ? x : rem) + j);
}
inline int stencil_half_scale(int scale) { return scale / 2 < 4 ? scale / 2 : 4; }   // HS
inline int stencil_mode(int fmt) { return fmt == 3 ? 2 : (fmt ? 1 : 0); }            // MODE: 0 dense slabs, 1 lists, 2 own pixels + margin plane

// ---- which loop a run takes, and where its model update runs ----------------------------------------------------------------
// One value each: a run has exactly one form and one home, and every question bf_run asks is answered from the two (RunPlan,
// bf_ctx.h).  The forms are bf_get_stat "loop_form"'s values.
enum class LoopForm : int {
    atomic = BF_LOOP_ATOMIC,           // global atomics into alternating plane buffers
    binned = BF_LOOP_BINNED,           // the two-kernel tile-binned loop
    one_kernel = BF_LOOP_ONE_KERNEL,   // the one-kernel iteration, one launch per iteration
    persistent = BF_LOOP_PERSISTENT,   // ... as the persistent loop kernel
    delta = BF_LOOP_DELTA,             // global atomics on ONE plane buffer that is kept up to date
};
enum class UpdateHome : int {
    tail,       // the stencil kernel's last work-group
    head,       // the head of the next scatter launch (the one-kernel loops have no other)
    separate,   // k_finish_update ahead of every scatter launch, the stencil kernel only accumulates
};
struct LoopChoice {
    LoopForm form;
    UpdateHome home;
};
// What the choice depends on.  The options: 0 never, 1 "auto", 2 whenever possible.
struct LoopFacts {
    int opt_binned = 1, opt_fused = 1, opt_persist = 1, opt_delta = 1, opt_sep_update = 1;
    bool co_schedule = false;     // the context shares the GPU with others
    double pixels = 0;            // of the scaled image
    long long n = 0;              // events
    int max_iter = -1;            // the run's cap (<= 0: none)
    bool has_noise = false, packed = true;
    bool warm = false;            // bf_set_model's warp is pending
    int live_ctx = 1;             // contexts of this process alive on the device
    // what plan_slice found possible: the two-kernel loop's grid, the one-kernel iteration's (and whether that loop is also the one
    // to take under "co_schedule"), the scatter format
    bool grid_ok = false, fused_ok = false, fused_shared = false;
    int fmt = 0;
    bool resident = true;         // every tile of the one-kernel grid can be resident at once (the persistent kernel)
};
inline bool one_kernel_ok(const LoopFacts& f) { return f.fused_ok && (!f.co_schedule || f.fused_shared); }
inline bool persistent_ok(const LoopFacts& f) {
    return one_kernel_ok(f) && !f.co_schedule && (f.opt_persist == 2 || (f.opt_persist == 1 && f.warm)) && f.live_ctx == 1 && f.resident;
}
inline bool delta_ok(const LoopFacts& f) {
    const bool pays = f.co_schedule && !f.warm && f.opt_binned == 1 && f.opt_fused != 2 && f.grid_ok && f.fmt == 0 && f.packed && !one_kernel_ok(f) &&
                      (double)f.n >= f.pixels && f.pixels < (double)(1u << 28) && (f.max_iter <= 0 || f.max_iter >= 200);
    return !f.has_noise && f.n > 0 && (f.opt_delta == 2 || (f.opt_delta == 1 && pays));
}
inline LoopChoice loop_choice(const LoopFacts& f) {
    if (delta_ok(f)) return {LoopForm::delta, UpdateHome::tail};
    if (persistent_ok(f)) return {LoopForm::persistent, UpdateHome::head};
    if (one_kernel_ok(f)) return {LoopForm::one_kernel, UpdateHome::head};
    if (!f.grid_ok) return {LoopForm::atomic, UpdateHome::tail};
    if (!f.co_schedule) return {LoopForm::binned, UpdateHome::head};
    const bool separate = f.opt_sep_update == 2 || (f.opt_sep_update == 1 && f.fmt == 2);
    return {LoopForm::binned, separate ? UpdateHome::separate : UpdateHome::tail};
}

}  // namespace bf_rules
