// bf_kernels.h -- launch interface between the C-ABI files (bf_context / bf_upload / bf_operators / bf_run / bf_tiles_abi / bf_local_abi .cpp) and
// bf_kernels.hip (gfx950 kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <atomic>

#include "bf_device.h"
#include "bf_plan_rules.h"

namespace bf {

constexpr int kHistCopies = 8;   // copies of the re-bin's global histogram (work-group b adds to copy b % 8: contention)
using bf_rules::kBinTileLdsMax;   // dynamic LDS of a scatter work-group
static_assert(bf_rules::kStencilTileR == kTileR && bf_rules::kStencilTileC == kTileC, "the rules count the stencil kernel's own tiles");
constexpr int kPrepBlocks = 1024;   // work-groups of k_prepare == SliceStats records it writes

// min / max / sum statistics of one staged slice (k_prepare), one record per work-group.
struct SliceStats {
    int32_t xmin, xmax, ymin, ymax, tmin, tmax;
    long long tsum;
};

struct WarpScatterArgs {
    const uint32_t* xy;
    const int32_t* t;
    float2* p;
    const uint8_t* noise;          // may be NULL
    double2* nxny;                 // written only by the final warp, at [perm[i]]
    double2* uv;                   // optional: Event::compute_uv fused into the final warp
    const uint32_t* perm;          // original index of slot i (NULL: identity)
    unsigned long long* plane;     // point-scatter accumulator (current buffer)
    uint32_t* cplane;              // SPLIT mode count plane (current buffer)
    const DevState* st;
    long long n;
    int check_done;                // 1 inside the fused loop: return at once if st->done; 2: run only if done
    EvSets sets;                   // pick_set: take xy / t / p / perm from sets.s[hot.cs ^ hot.flip] instead
    int pick_set;
    int sorted_out;                // write nxny / uv at the slot index (coalesced) instead of perm[slot]
    bool packed;
};

struct StencilArgs {
    const DevState* st;
    int check_done;
    int R, C, scale, tbits;
    long long tmin;
    const unsigned long long* plane;   // SRC 0 / 1
    const uint32_t* cplane;            // SRC 1
    const float* time_in;              // SRC 2
    float* time_out;                   // optional
    uint32_t* count_out;               // optional
    float* gx_out;                     // optional (gy_out must be set with it)
    float* gy_out;
    MomentAcc* acc;                    // optional: moment sums are added to these exact accumulators
    MomentAcc* acc_zero;               // tile-binned loop: the other parity's accumulators, cleared here
    const uint32_t* ovf_cur;           // tile-binned loop: overflow events of this / the previous iteration, and the
    const uint32_t* ovf_prev;          //   next iteration's counter (cleared here)
    uint32_t* ovf_next;
    unsigned long long* zero_plane;    // optional: the OTHER plane buffer, zeroed here
    uint32_t* zero_cplane;
    // tile-binned loop: one bit per image pixel that an overflow event of this iteration touched (set by the scatter kernel;
    // row pitch ovf_pitch words, column Y in word (Y >> 5) + 1), and the other buffer's bitmap, cleared with its planes
    const uint32_t* ovf_bits;
    uint32_t* zero_bits;
    int ovf_pitch;
    int zero_full;                     // clear every pixel of the other buffer, not only the flagged ones (its dirt may predate the bitmap: first launch of a run)
    // fused reduction + model / loop update by the last work-group (NULL ticket: accumulate only)
    unsigned int* ticket;
    DevState* st_rw;                   // where the updated state goes (tile-binned loop, update here: NOT the buffer `st` is read from)
    DevState* snap;                    // optional: pinned host copy of the updated state, polled by the host
    bf_trace_rec* trace;
    int update_mode;                   // 1: full iteration_step / run() update, 0: model only
    unsigned long long* tl;            // debug timeline (BF_TIMELINE builds), usually NULL
    int tl_launch;
    // SRC 3 (tile-binned): per-bin slabs + the overflow planes of buffer `cur`
    const unsigned long long* slabs;
    const uint16_t* cidx;              // compact lists (hot.fmt == 1): see BinScatterArgs
    const uint32_t* chdr;
    int compact;
    const unsigned long long* m_cur;   // interior + margin format (compact == 3): the margin plane of buffer `cur`
    BinGrid g;
    int cur;
    // SRC 3: which tile a work-group takes -- 0: launch order (row-major), 1: one band of tile rows per residue class mod 8 of the
    // launch id (bf_rules::tile_of_block).  Any value gives the same bits; bf_run picks by what was measured (enqueue_iteration).
    int tile_bands;
};

// Profiling hook: when armed (by ProfScope, bf_ctx.h), the next launch of a loop kernel goes through
// hipExtLaunchKernelGGL with these events, which then carry the kernel's own begin / end timestamps (what
// rocprofv3 reports) instead of bracketing the launch with two extra barrier packets (~1.5 us more).
struct LaunchTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    bool consumed = false;
};
LaunchTimer& launch_timer();   // thread local
// Plain launch, or (profiling armed) an extended launch whose events carry the kernel's own timestamps.
template <class K, class... A>
static inline void launch_timed(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    LaunchTimer& t = launch_timer();
    if (t.start && !t.consumed) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, t.start, t.stop, 0, args...);
        t.consumed = true;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    }
}

// LDS tiles above 64 KiB need the dynamic-LDS attribute raised (160 KiB per CU on gfx950).  The attribute belongs to the
// (function, device) pair, so it is raised once per device the functions of one launcher are launched on: `raised`, that
// launcher's own static word, holds a bit per device ordinal, set after the calls succeeded (two threads racing here both
// make the calls, which is harmless).  The launchers whose limit depends on the call's sizes set it per call instead.
template <size_t N>
static inline hipError_t raise_dynamic_lds(std::atomic<unsigned long long>& raised, const void* const (&fns)[N]) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    const unsigned long long dev_bit = 1ull << (dev & 63);
    if (raised.load(std::memory_order_acquire) & dev_bit) return hipSuccess;
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kBinTileLdsMax);
        if (e != hipSuccess) return e;
    }
    raised.fetch_or(dev_bit, std::memory_order_release);
    return hipSuccess;
}

void launch_set_state(DevState* st, const DevState& v, hipStream_t s);
void launch_project_dn(const uint32_t* xy, const int32_t* t, float2* p, double2* nxny, const uint32_t* perm, int have_n,
                       const DevState* st, long long n, hipStream_t s);
// the run's final warp with compute_uv fused (outputs in slot order): one event per thread
void launch_final_warp(const WarpScatterArgs& a, hipStream_t s);
void launch_warp_scatter(const WarpScatterArgs& a, bool warp, bool scatter, bool write_n,
                         hipStream_t s);
// delta scatter: warp, and move the events whose pixel changed on a plane that holds the image of the stored products
// (xy, t, p, plane, cplane, st, n, check_done, packed of `a`; no noise mask, no permutation)
void launch_warp_scatter_delta(const WarpScatterArgs& a, hipStream_t s);
void launch_prepare(const int32_t* fr_x, const int32_t* fr_y, const int32_t* t_in, uint32_t* xy,
                    int32_t* t_out, float2* p, long long n, long long n_pad, SliceStats* stats,
                    hipStream_t s);
void launch_local_time(const unsigned long long* ts, unsigned long long t0, int32_t* t_out, long long n, hipStream_t s);
// (ts32: `ts` holds 32-bit words, the low halves of the timestamps)
void launch_local_time16(const unsigned long long* ts, bool ts32, const uint16_t* row, const uint16_t* col, unsigned long long t0,
                         int32_t* x_out, int32_t* y_out, int32_t* t_out, long long n, hipStream_t s);
void stencil_grid(int R, int C, int* gx, int* gy);
// what a stencil launch reads: the first three are k_stencil's sources, the last two k_stencil_binned's
enum class StencilSrc {
    packed_plane,   // one u64 plane: count << tbits | time sum
    split_planes,   // a u64 sum plane and a u32 count plane
    time_image,     // an f32 time image (a.time_in)
    binned,         // the tile-binned scatter's slabs, lists or own pixels + margin plane
    plane_binned,   // the packed plane through k_stencil_binned (launch_stencil_plane)
};
void launch_stencil(const StencilArgs& a, StencilSrc src, hipStream_t s, int n_cus = 0);   // n_cus: lets the tile-binned form pick its build by how often the grid fills the GPU
// applies a pending update (sums in `acc`) to `st` in place: the tile-binned loop's update outside a warp+scatter launch
// (snap_seq / seq: after the snapshot has been stored and fenced, `seq` goes to the pinned word the host spins on)
void launch_finish_update(DevState* st, MomentAcc* acc, const uint32_t* ovf_prev, int j, int cur_prev, bf_trace_rec* trace,
                          DevState* snap, hipStream_t s, const uint32_t* lost = nullptr, unsigned long long* snap_seq = nullptr,
                          unsigned long long seq = 0);
void launch_compute_uv(const double2* nxny, double2* uv, long long n, hipStream_t s);
void launch_unpermute(const double2* src, const uint32_t* perm, double2* dst, long long n, hipStream_t s);
void launch_expand_pr(const uint32_t* xy, const float2* p, const uint32_t* perm, double2* pr, long long n,
                      hipStream_t s);

// bf_tiles.hip -- grid of independent per-tile optimizers (BASELINE config 4)
struct TileGrid {
    int32_t rows, cols, res_x, res_y;   // tile (r, c) = (fr_x * rows / res_x, fr_y * cols / res_y)
};
struct TileArgs {
    const uint32_t* xy;
    const int32_t* t;
    float2* p;
    const uint32_t* perm;
    double2* nxny;
    const uint32_t* tile_start;
    DevState* states;                  // one per tile: in = zero-model template, out = final state
    int32_t scale, seed_res_x, seed_res_y, guard_res_x, guard_res_y, min_events, max_px;
};
int launch_tile_sort(const uint32_t* xy, const int32_t* t, const uint32_t* perm_in, long long n, const TileGrid& g,
                     uint32_t* hist, uint32_t* start, uint32_t* cursor, uint32_t* oxy, int32_t* ot, float2* op,
                     uint32_t* operm, hipStream_t s);   // -1: the histograms' LDS cannot be configured
int launch_tile_optimizer(const TileArgs& a, int ntiles, hipStream_t s);
int launch_tile_optimizer_many(const TileArgs* slices, int nslices, int ntiles, int scale, int max_px, uint32_t* counter, int n_cus,
                               hipStream_t s);
void launch_fill_states(DevState* states, const DevState& tmpl, int nt, hipStream_t s);
// Event groups (bf_run_groups): the same counting sort keyed by gid[upload index] (-1 and anything outside 0 .. K-1: the
// trailing bucket K; hist / start / cursor hold K + 2 words), the groups' fr boxes (box: K x {x min, x max, y min, y max} of
// the SORTED events), the optimizers -- one work-group per group, claimed in `order` from `counter` (one zeroed word) -- and
// the (0, 0) of the trailing bucket.  warm: every group's state holds set_model's warp and model.
constexpr int kGroupLdsBudget = 156 * 1024;   // the planes of one group's window (16 bytes per pixel), as for a tile
int launch_group_sort(const uint32_t* xy, const int32_t* t, const uint32_t* perm_in, long long n, const int32_t* gid, int K,
                      uint32_t* hist, uint32_t* start, uint32_t* cursor, uint32_t* oxy, int32_t* ot, float2* op,
                      uint32_t* operm, hipStream_t s);
void launch_group_boxes(const uint32_t* xy, const uint32_t* perm, const int32_t* gid, const uint32_t* start, long long n, int K,
                        int32_t* box, hipStream_t s);
int launch_group_optimizer(const TileArgs& a, const uint32_t* order, int K, bool warm, uint32_t* counter, int n_cus,
                           hipStream_t s, int* per_cu_out);
void launch_group_rest(const uint32_t* perm, const uint32_t* start, int K, double2* nxny, hipStream_t s);
// bf_groups_wide.hip -- a group solved by the chip-wide loop ("groups_wide"): slots beg .. beg + n of the sorted set into the three
// int32 staging columns of the inner context (upload index j = slot beg + j), and the inner run's per-event results back.
struct WideBack {
    const uint32_t* in_perm;     // inner slot -> inner upload index (null: the identity)
    const float2* in_p;          // inner products, inner slot order
    const double2* in_nxny;      // inner (nx, ny): by inner slot (in_nxny_by_slot) or by inner upload index; null: zeros
    int32_t in_nxny_by_slot;
    uint32_t beg, n;             // the group's bucket of the outer set
    const uint32_t* out_perm;    // outer slot -> outer upload index
    float2* out_p;               // outer products, outer slot order
    double2* out_nxny;           // outer (nx, ny), outer upload order
};
void launch_group_gather(const uint32_t* xy, const int32_t* t, uint32_t beg, uint32_t n, int32_t* ox, int32_t* oy, int32_t* ot,
                         hipStream_t s);
void launch_group_scatter_back(const WideBack& a, hipStream_t s);

// bf_rebin.hip / bf_scatter.hip / bf_stencil.hip / bf_fused.hip (the tile-binned loops)
int bin_kernel_setup();
// k_stencil_binned on the packed image-linear plane `a.plane` (StencilSrc::plane_binned; R * C * 8 < 2^31: 32-bit byte offsets)
void launch_stencil_plane(const StencilArgs& a, dim3 grid, hipStream_t s);
void launch_stencil_binned(const StencilArgs& a, dim3 grid, hipStream_t s, int n_cus);   // (the build: bf_rules::stencil_capped)
// interior + margin format: clear what the bins' lists name in `mplane`, empty the lists (a run that cannot rely on the
// loop's own clean-up: the dirty margin plane is the one its first iteration adds to, or the bin grid changes)
void launch_margin_clean(unsigned long long* mplane, const uint32_t* mlist, uint32_t* mcount, int nbins, int mcap, hipStream_t s);
void launch_rebin(const EvSets& sets, int has_perm, long long n, DevState* st, const BinGrid& g,
                  uint16_t* binid, uint32_t* hist_cnt, uint32_t* bin_start,
                  uint32_t* cursor, uint32_t* armed, const WarpParams* prewarp, int pack_limit, hipStream_t s,
                  uint32_t* ftab = nullptr, uint32_t* lost = nullptr);   // (g.fz != 0: the one-kernel iteration's range table and flag)
struct BinScatterArgs {
    EvSets sets;
    const uint32_t* bin_start;
    unsigned long long* slabs;       // per bin: the dense tile, or the values of its compact list
    uint16_t* cidx;                  // compact lists: tile-local pixel index of every entry (per bin: L * LR slots)
    uint32_t* chdr;                  // compact lists: first entry of every tile row, per bin (LR + 1 words)
    int compact;                     // this slice's scatter writes compact lists (bf_set_cloud's choice)
    unsigned long long* ovf_plane;   // overflow planes of buffer `cur`
    uint32_t* ovf_cplane;
    uint32_t* ovf_bits;              // ... and its dirty bitmap (StencilArgs)
    int ovf_pitch;
    const DevState* st_in;           // state as of the previous launch ...
    DevState* st_out;                // ... and with the pending update applied (written by work-group 0)
    DevState* snap;                  // optional: pinned host copy of st_out, polled by the host
    MomentAcc* acc;                  // moment sums of the previous iteration (parity (j - 1) & 1)
    uint32_t* ovf_cur;               // this iteration's overflow counter
    const uint32_t* ovf_prev;        // the previous iteration's (final)
    bf_trace_rec* trace;
    BinGrid g;
    int cur, j;                      // plane buffer of this iteration; number of stencil launches completed before it
    unsigned long long* tl;
    // interior + margin format (compact == 3): the bin's own TSR x TS pixels go to `slabs` (plain stores, nothing shared), what
    // its events left in the margin of its LDS tile is ADDED to the margin plane of buffer `cur` and listed, and the pixels
    // this bin listed in its previous executed launch are cleared in the other buffer's margin plane
    unsigned long long* m_cur;
    unsigned long long* m_prev;
    uint32_t* mlist;                 // per bin: mcap linear pixel indices
    uint32_t* mcount;                // per bin: entries of its list
    int mcap;
};
// `threads`, `per_thread`: bf_rules::scatter_size()'s answer for this slice, taken as it is -- a tuple that is not one of the
// compiled instantiations (bf_rules::scatter_compiled) is refused with hipErrorInvalidValue, never rounded to a neighbour.
hipError_t launch_bin_warp_scatter(const BinScatterArgs& a, bool warp, int threads, int per_thread, hipStream_t s);
// The one-kernel iteration (k_fused_pass, bf_fused.hip): warp + scatter + stencil + moments of one image tile per work-group.
struct FusedArgs {
    EvSets sets;
    const uint32_t* ftab;            // FusedTab per tile (written by the counting sort's scan)
    const DevState* st_in;           // state as of the previous launch ...
    DevState* st_out;                // ... and with the pending update applied (written by work-group 0)
    DevState* snap;                  // optional: pinned host copy of st_out, polled by the host
    MomentAcc* acc_in;               // moment sums of the previous pass
    MomentAcc* acc_out;              // this pass adds here
    MomentAcc* acc_zero;             // cleared for the next pass
    uint32_t* lost;                  // [3], by launch number mod 3: raised by a pass that cannot vouch for its sums (an event moved
                                     // further than the bins allow)
    bf_trace_rec* trace;
    int nbr, nbc;                    // image tiles
    int R, C;
    int j;                           // launch number (the update of iteration j runs at the head of launch j + 1)
    int warp;                        // 0: scatter the events where their stored products put them (first pass of a cold run)
    unsigned long long* tl;          // debug timeline (`make tl` build only)
};
hipError_t launch_fused_pass(const FusedArgs& a, int half_scale, int rows_per_tile, hipStream_t s);
// The persistent form of the one-kernel iteration (k_fused_loop, bf_loop.hip): up to max_passes iterations per launch, the
// work-groups resident, the moment sums exchanged through tagged records in memory instead of a launch boundary.
struct FusedLoopArgs {
    EvSets sets;
    const uint32_t* ftab;            // FusedTab per tile
    DevState* st;                    // read at entry; written (with st_other and snap) by work-group 0 at exit
    DevState* st_other;
    DevState* snap;                  // pinned host copy: (done, it) after every pass, the whole state at exit
    unsigned long long* rec;         // [2][tiles * NSUB][16][2]: per-sub-tile records (payload, tag), by pass parity
    unsigned long long* red;         // [2][16][16][2]: the reducers' records
    float2* scratch[4];              // private product arrays (lists longer than a pass): the strips' readers' [0 .. 2], the owners' [3]
    bf_trace_rec* trace;
    int nbr, nbc, R, C;
    int max_passes;
    int first_warp;                  // 0: the first pass of the run scatters the stored products as they are
    unsigned long long* tl;          // debug timeline (`make tl` build only)
    int debug_abort;                 // >= 0: every work-group gives up at that pass (BF_DEBUG_PERSIST_ABORT: exercises the undo + fall-back)
    int debug_mute;                  // >= 0: from that pass on the LAST work-group publishes no records, as if it had never become
                                     // resident (BF_DEBUG_PERSIST_MUTE): one reducer really times out, the others do not
    int debug_split, debug_split_late;   // >= 0: the LAST work-group alone "times out" at that pass (BF_DEBUG_PERSIST_SPLIT=<pass>[,late];
                                     // the host makes it the launch's last pass): at once -- its ABORT decides --, or ~100 us late --
                                     // the others have committed and it catches up
    unsigned long long* verdict;     // one word per context: (launch id << 2) | COMMIT / ABORT, decided by compare-and-swap
    int* broken;                     // pinned host word, set if a committed launch's records cannot be read back (cannot happen)
};
hipError_t launch_fused_loop(const FusedLoopArgs& a, int half_scale, int rows_per_tile, int n_cus, hipStream_t s);
// can `ntiles` work-groups of that kernel be resident at once on this device (n_cus compute units)?
bool fused_loop_resident(int half_scale, int rows_per_tile, int n_cus, int ntiles);
void launch_run_init(DevState* st, const DevState& v, uint32_t* ovf, uint32_t prev_dirty, MomentAcc* acc, bool init_loop, hipStream_t s);

// bf_local.hip -- contrast-score evaluation of OptimizerLocal (optimizer_sampler.cpp:120-153)
struct LocalGeom {
    int32_t scale, wsx, wsy, R, C, pad;
    float kx, ky;              // float(n) / nz of Event::apply_project, the same for every event
    double x_shift, y_shift;   // -event_c.pr * scale + metric_wsize / 2.0 (optimizer_sampler.cpp:126-127)
};
void launch_local_project_count(const uint32_t* xy, const int32_t* t, long long n, const LocalGeom& g, uint32_t* plane,
                                hipStream_t s);
int launch_local_blur_score(const uint32_t* plane, uint32_t* zero_plane, const LocalGeom& g, unsigned long long* score,
                            uint8_t* img_out, hipStream_t s);

// a grid of OptimizerLocal windows, one work-group each (bf_local.hip); < 0: scale above 7 / kernel attributes / window too large for the LDS
int launch_local_tile_optimizer(const uint32_t* xy, const int32_t* t, const uint32_t* tile_start, bf_local_state* states, int32_t* rcs,
                                const TileGrid& g, int scale, int wsz, int guard_res_x, int guard_res_y, long long max_evaluations,
                                hipStream_t s);

// bf_global.hip -- the candidate sweep of OptimizerGlobal (optimizer_global.cpp:4-150)
struct GlobalGeom {
    int32_t scale, mw;        // scale, metric_wsize
    int32_t xs, ys;           // x_min * scale, y_min * scale (an int product, as at :17-18)
    int32_t sx, sy;           // scale_img_x / _y
    int32_t Rb, Cb;           // scale_bordered_img_x / _y
    long long plane;          // Rb * Cb: the stride of one candidate's planes
};
struct GlobalCand {
    double nx, ny, nz;
    float kx, ky;             // float(n) / nz of Event::apply_project (event.h:164-165)
};
struct GlobalEventState {     // per event, upload order
    double *max_score, *best_nx, *best_ny, *best_nz, *best_pr_x, *best_pr_y;
};
// The per-cell objective S(k, cell) (include/bf_accel.h): the slice in cell order, cut into runs of at most run_len
// consecutive events of ONE cell (one work-group each), and where the sums go.
constexpr int kGlobalCellStride = 32;   // candidates per cell in the batch block (>= the largest batch)
constexpr uint32_t kGlobalNoCand = 0xffffffffu;   // best_k of a cell before anything was evaluated
struct GlobalCellGrid {
    int32_t cell_rows, cell_cols, n_cell_y, n_cells;
};
struct GlobalCells {
    const uint32_t* xy; const int32_t* t;   // the slice's events, ordered by cell
    const uint32_t* idx;                    // ... and their upload indices (the order composed with perm)
    const uint32_t* cell_start;             // n_cells + 1 offsets into the three arrays above
    const uint32_t *run_cell, *run_start;   // n_runs each: run r holds events [run_start[r], min(+ run_len, end of its cell))
    int32_t n_runs, run_len;                // run_len 64 or 256: the fold's work-group size
    int32_t n_cells;
    unsigned long long* block;              // [n_cells][kGlobalCellStride] sums of one batch; all zero between batches
    unsigned long long* best_sum;           // per cell: the running largest S(k, cell) ...
    uint32_t* best_k;                       // ... and the lowest k that reached it (kGlobalNoCand: nothing evaluated yet)
    long long* surface;                     // null, or [n_cells][n_cand]
    long long n_cand, k0;                   // candidates of the sweep; the batch's first
    const uint32_t* ks;                     // the lattice k of each slot of the batch; null: slot b is candidate k0 + b
};
size_t global_tile_lds(int scale, int mw);
void launch_global_reset(const uint32_t* xy, const uint32_t* perm, long long n, const GlobalEventState& st, hipStream_t s);
// one batch of nb candidates; `pts` must be all zero (nb planes); < 0: scale above 7 / kernel attributes / LDS.
// cells null: k_global_fold adds S(k) into S[0 .. nb).  Otherwise k_global_fold_cells folds the same per-event state and
// k_global_cells_best leaves S(k) = the sum over the cells in S[0 .. nb) (which must be zero before), with cells->k0 the
// batch's first candidate and cells->ks its slots' lattice k; nb <= kGlobalCellStride, img_out and scores_out unused.
int launch_global_batch(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalGeom& g,
                        const GlobalCand* cands, int nb, uint32_t* pts, uint32_t* win, uint8_t* img_out,
                        const GlobalEventState& st, unsigned long long* S, float* scores_out, const GlobalCells* cells,
                        hipStream_t s);
// The projections over the cell runs (include/bf_accel.h): every event of the cell-ordered slice under a candidate of its own
// into ONE point plane `pts` (all zero before), G2 on it (win, img_out as above), then per event its score into scores_out (may
// be null) and its share of the objective into cell_sums[its cell] ([n_cells], zero before).  Only cells' xy / t / idx /
// cell_start / run_* fields are read; the per-event state, block, best_sum and best_k are not touched.  < 0 as
// launch_global_batch.  Where the candidate comes from:
struct GlobalCandTable {      // bf_global_project_cells: cell_cands[the event's cell]
    const GlobalCand* cell_cands;   // [n_cells] on the device; the entry of a cell without events is never read
};
struct GlobalCandField {      // bf_global_project_field: interpolated between the centres of the cells around the event's
    GlobalCellGrid cg;              // address (include/bf_global_field.h)
    uint32_t n_cell_x;
    const double *cell_nx, *cell_ny;   // [n_cells] on the device, ALL read (an empty cell is a corner for its neighbours)
    double nz;
    double *ev_nx, *ev_ny;          // null, or n doubles each: the interpolated (nx, ny) of every event at its upload index
};
int launch_global_runs(const GlobalCells& cells, const GlobalGeom& g, const GlobalCandTable& src, uint32_t* pts, uint32_t* win,
                       uint8_t* img_out, float* scores_out, unsigned long long* cell_sums, hipStream_t s);
int launch_global_runs(const GlobalCells& cells, const GlobalGeom& g, const GlobalCandField& src, uint32_t* pts, uint32_t* win,
                       uint8_t* img_out, float* scores_out, unsigned long long* cell_sums, hipStream_t s);
// The held flow (include/bf_accel.h, bf_global_hold_field / bf_global_hold_best): per event of the slice its (nx, ny) and
// (u, v) at its UPLOAD index, and the two f32 products (kx * float(t), ky * float(t)) of Event::apply_project at its position
// in the order of the arrays it was computed from (the cell order of GlobalCells::xy / idx, or the context's slot order).
struct GlobalHeld {
    double2 *nxny, *uv;   // n each, upload order
    float2* p;            // n, source order
    uint32_t *xy, *idx;   // launch_global_hold_best only: its own copy of the source order's address words and upload indices
};
// One launch over the cell runs (k_global_hold_runs): every event under the candidate launch_global_runs would project it
// under.  Nothing is rendered or scored; only cells' xy / t / idx / cell_start / run_* fields are read.
void launch_global_hold(const GlobalCells& cells, const GlobalCandTable& src, const GlobalHeld& h, hipStream_t s);
void launch_global_hold(const GlobalCells& cells, const GlobalCandField& src, const GlobalHeld& h, hipStream_t s);
// The per-event best state as a held flow: slot i (upload index perm[i]; null: i) under (best_nx, best_ny, best_nz) of its event.
// The slot order is copied into h.xy / h.idx: a later bf_run may re-bin the context's slots, the held flow stays what it was.
void launch_global_hold_best(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalEventState& st,
                             const GlobalHeld& h, hipStream_t s);
// counting sort of the slice by cell, in two launches around the host's scan of `count`: the events per cell, then the
// events into cell order (`cursor`: n_cells zeros; cells.xy / t / idx as mutable arrays of n)
void launch_global_cell_count(const uint32_t* xy, long long n, const GlobalCellGrid& cg, uint32_t* count, hipStream_t s);
void launch_global_cell_order(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalCellGrid& cg,
                              const uint32_t* cell_start, uint32_t* cursor, uint32_t* cxy, int32_t* ct, uint32_t* cidx,
                              hipStream_t s);
// The candidate set of one level of bf_global_search_cells_pyramid (include/bf_accel.h), decided on the device.  The
// lattice is n_x x n_y points, k = i * n_y + j; a bitmap holds one bit per k (bit k & 31 of word k >> 5).
struct GlobalLattice {
    long long n_x, n_y;
};
struct GlobalAxis {           // one axis value of the lattice: make_cand's n and k of it
    double n;
    float k, pad;
};
// level 0 without seeds: every (i, j) with i % stride == 0 and j % stride == 0 into `level`
void launch_global_stride_mark(const GlobalLattice& lt, long long stride, uint32_t* level, hipStream_t s);
// a window of (2 * radius + 1)^2 points, `stride` lattice steps apart and clipped to the lattice, around the centre of every
// cell that has events: its running best when best_sum > 0, else its seed (seed null or < 0: none).  Bits of `evaluated`
// are skipped.
void launch_global_seed_mark(const GlobalLattice& lt, long long stride, int radius, int n_cells, const uint32_t* cell_start,
                             const unsigned long long* best_sum, const uint32_t* best_k, const int32_t* seed,
                             const uint32_t* evaluated, uint32_t* level, hipStream_t s);
// The level's bitmap into the ascending list of its k, in two steps around the host's read of the count: offs[w] = the
// bits set below word w (offs has n_words + 1 entries: the last is the count; cnt the same size), then the list, with
// `evaluated` |= `level` and `level` left zero.  temp: global_scan_temp_bytes(n_words) bytes.
size_t global_scan_temp_bytes(long long n_words);
hipError_t launch_global_bitmap_scan(const uint32_t* level, long long n_words, uint32_t* cnt, uint32_t* offs, void* temp,
                                     size_t temp_bytes, hipStream_t s);
void launch_global_bitmap_list(uint32_t* level, uint32_t* evaluated, long long n_words, const uint32_t* offs, uint32_t* list,
                               hipStream_t s);
// cands[m] = the candidate at lattice point list[m], from the two axis tables (the bits make_cand gives)
void launch_global_cands_from_lattice(const GlobalLattice& lt, const uint32_t* list, long long m, const GlobalAxis* tab_x,
                                      const GlobalAxis* tab_y, double nz, GlobalCand* cands, hipStream_t s);

void launch_proj_count(const uint32_t* xy, const float2* p, const uint8_t* noise, long long n, int scale, int res_x,
                       int res_y, int show_final, uint32_t* plane, hipStream_t s);
void launch_proj_scale(uint8_t* img, long long n, const unsigned long long* score, hipStream_t s);

// EventFile::color_time_img (event_file.h:649-747)
struct ColorGeom {
    int32_t scale, show_final, mx, my, R, C;   // mx = scale * res_x (:668-669), R = mx + scale (:670-671)
    long long t_min, t_range;                  // min t; max(t_max, 0) - t_min (:659-662)
    double x_shift, y_shift;                   // :677-678
};
void launch_color_time(const uint32_t* xy, const int32_t* t, const float2* p, const uint8_t* noise, long long n,
                       const ColorGeom& g, uint32_t* cnt, unsigned long long* pc, unsigned long long* ps, uint8_t* bgr,
                       hipStream_t s);

void launch_copy(const void* src, void* dst, long long bytes, int blocks, bool nontemporal, hipStream_t s);
void launch_eval_sincos(const double* x, long long n, int table, double* sn, double* cs, hipStream_t s);

// bf_emit.hip -- the -o table accumulated on the device (bf_emit_slice).  One slice: M = lead + n elements, element 0 the
// lead (if any), element lead + i upload index i; every array below holds M entries.
struct EmitSlice {
    // the committed slice (live event set, slot order) and its flow (upload order; null: zero flow)
    const uint32_t* xy; const int32_t* tloc; const uint32_t* perm; const double2* uv;
    long long n; int lead;
    unsigned long long first, cap, start_time, prev_end, last;   // ring positions / logical ns
    unsigned long long lead_t; uint32_t lead_row, lead_col;
    int rows, cols;
    // persistent state: covered plane (cap bytes), per-pixel tail (rows * cols)
    uint8_t* plane; unsigned long long *tail_t, *tail_g;
    // scratch; sort key = pixel << jbits | element (jbits: enough bits for the elements, kbits: for the whole key)
    unsigned long long* t; uint32_t* rc; uint8_t* flag; unsigned long long* keys; uint32_t* pos;
    int jbits, kbits;
    uint32_t* err;
    // rows out: a ring of out_rows rows in pinned, device-mapped host memory (row r at r % out_rows); the slice's rows start at
    // *off_in, and *off_out = *off_in + rows afterwards; rec[0..2] = first row, rows, error bits (pinned)
    unsigned long long* out_t; uint16_t *out_row, *out_col; double *out_u, *out_v;
    unsigned long long out_rows;
    const unsigned long long* off_in; unsigned long long* off_out;
    unsigned long long* rec;
};
size_t emit_temp_bytes(long long m);
hipError_t launch_emit(const EmitSlice& a, unsigned long long* keys_sorted, void* temp, size_t temp_bytes, hipStream_t s);

// bf_frame.hip -- the 2 x 2 frame mosaic of --img / --video (bf_frame_render): tiles of R x C (grey) and CR x CC BGR (colour,
// CR = R + 3, CC = C + 3), index 0 the compensated tiles (top row), 1 the raw ones; the colour resize's taps (row0 / row1 / row_w:
// R entries, col0 / col1 / col_w: C entries).  Out: the PPM payload (ppm_dwords dwords) and / or the AVI payload (avi_dwords
// dwords, rows of `stride` bytes); a null destination is skipped.
struct FrameCompose {
    const uint8_t* gray[2];
    const uint8_t* colour[2];
    int R, C, CR, CC;
    const int32_t *row0, *row1, *col0, *col1;
    const float *row_w, *col_w;
    uint8_t *ppm, *avi;
    long long ppm_dwords, avi_dwords;
    int stride;
};
void launch_frame_compose(const FrameCompose& a, hipStream_t s);

// bf_flowimg.hip -- the per-pixel flow field and EventFile::color_flow_img (event_file.h:318-350) of a slice on a res_x x res_y
// sensor (pixel (x, y) at x * res_y + y).  The event sources are plain pointers: address word and f32 products in slot order,
// `perm` the upload index of a slot (null: the identity), `noise` flags and `nxny` in upload order (null: no flag / zero flow).
struct FlowSources {
    const uint32_t* xy; const float2* p; const uint32_t* perm; const uint8_t* noise; const double2* nxny;
    long long n;
};
// owner: res_x * res_y words, every one 0xffffffff ("none") on entry; first != 0: the smallest upload index that lands on a
// pixel owns it, else the largest
void launch_flow_owner(const FlowSources& e, int res_x, int res_y, int first, uint32_t* owner, hipStream_t s);
// per pixel, every destination optional: owner index or -1, (u, v) of the owner (0 without one), the .flo pair (float v, float
// u; 1e9 twice without an owner), the H and S bytes, the B, G, R bytes
struct FlowFieldOut {
    int32_t* owner; double *u, *v; float2* flo; uint8_t *hs, *bgr;
};
void launch_flow_field(const uint32_t* owner, const double2* nxny, long long px, const FlowFieldOut& o, hipStream_t s);
// the same per pixel from a flow that is (u, v) already, in upload order (the held flow of the exhaustive search: its nz is
// the candidate's own, not the constant of uv_from_n); null: zero flow
void launch_flow_field_uv(const uint32_t* owner, const double2* uv, long long px, const FlowFieldOut& o, hipStream_t s);
// The flow frame: three R x C tiles side by side -- grey | B, G, R | grey -- as PPM payload (top-down RGB, ppm_dwords dwords
// cover its 9 R C bytes) and / or AVI payload (bottom-up BGR rows of `stride` bytes, zero padding); a null destination is skipped.
struct FlowFrameCompose {
    const uint8_t *left, *flow, *right;
    int R, C;
    uint8_t *ppm, *avi;
    long long ppm_dwords, avi_dwords;
    int stride;
};
void launch_flow_frame_compose(const FlowFrameCompose& a, hipStream_t s);

}  // namespace bf
