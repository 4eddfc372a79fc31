// bf_ctx.h -- private to the C-ABI implementation files (bf_ctx.cpp, bf_context.cpp, bf_upload.cpp, bf_operators.cpp, bf_plan.cpp, bf_run.cpp,
// bf_tiles_abi.cpp, bf_local_abi.cpp, bf_global_search.cpp, bf_emit_abi.cpp, bf_frame_abi.cpp, bf_flow_abi.cpp, bf_segment_abi.cpp, bf_assign_abi.cpp,
// bf_propose_abi.cpp, bf_track_abi.cpp): the context structure behind `bf_ctx` and the declarations of the small helpers they share (error text,
// profiling brackets, kernel-argument builders, the buffers allocated on first use; defined in bf_ctx.cpp, but for the few that
// bf_run.cpp calls once per kernel launch, which are inline here).  What the context knows about its slice -- the flags every
// entry reads -- is the base struct bf_state::SliceState (bf_ctx_state.h), changed through its named transitions only.  Every HIP resource of a
// context lives in a handle of bf_mem.h; the raw pointers left below are aliases into those and say so.  The asynchronous
// uploads keep all their state in one member, `up`: the copy stream and two staging slots, each FREE, RECORDED, ISSUED or EARLY
// (bf_ctx::UploadSlot); the entries on the K models' vote planes keep their scratch in one member, `vote`, and what they share on
// the host is declared in bf_vote_planes.h.  Nothing here is part of the ABI (include/bf_accel.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <string>
#include <thread>
#include <vector>

#include "bf_assign.h"
#include "bf_ctx_state.h"
#include "bf_device.h"
#include "bf_group_rules.h"
#include "bf_kernels.h"
#include "bf_mem.h"
#include "bf_segment.h"

using namespace bf;
using bf_mem::DevArray;
using bf_mem::Event;
using bf_mem::HostArray;
using bf_mem::MappedArray;
using bf_mem::Stream;

// Contexts alive per device in this process (defined in bf_context.cpp): the persistent loop kernel is for a context alone on its
// device (bf_rules::persistent_ok).
extern std::atomic<int> g_live_ctx[64];

struct GlobalSearch;   // bf_global_search.cpp: the exhaustive search's window, scratch and per-event state
struct GlobalSearchFree { void operator()(GlobalSearch* g) const; };   // (defined where the type is complete)

struct ProfRec {
    Event a, b;
    int cat;
    long long nev;
};

// Margins of the tile-binned loops (bf_plan_rules.h).  The tile shape, the scatter work-groups' size and their events per thread
// are chosen per slice (bf_plan.cpp, by the rules of bf_plan_rules.h): the options that overrode them went in round 5.
using bf_rules::kBinMargin;
using bf_rules::kFusedMargin;

struct bf_ctx : bf_state::SliceState {
    int device = 0;
    Stream stream;                   // created, or the caller's (bf_create)

    long long cap_events = 0;   // padded
    long long n = 0, n_pad = 0;
    size_t cap_px = 0;
    int cap_blocks = 0;

    // two event sets: the tile-binned mode ping-pongs between them on every re-bin
    struct EvSet { DevArray<uint32_t> xy; DevArray<int32_t> t; DevArray<float2> p; DevArray<uint32_t> perm; DevArray<float2> p2; };
    EvSet set[2];                    // (SliceState: cs is the set holding the live events, has_perm says it is permuted)
    DevArray<uint8_t> d_noise;
    // tile-binned scatter
    int opt_binned = 1;              // 0 never, 1 when it pays (dense enough), 2 whenever possible
    bool opt_bin_predict = true;
    bool opt_co_schedule = false;    // several slice contexts share the GPU: the update runs in the stencil kernel's last work-group
    int opt_bin_pack_limit = 64;     // bits available to the per-bin packing (lower only to test the fallback)
    int n_cus = 0;
    BinGrid grid;                    // the slice's bin grid where plan_slice chose the loop (SliceState::use_binned)
    // one-kernel iteration (k_fused_pass): the loop of a context that has the GPU to itself
    int opt_fused = 1;               // 0 never, 1 where it is the faster loop (small slices on small images; sparser ones only when
                                     // the context is co-scheduled with others), 2 whenever possible
    BinGrid fgrid;                   // its sort grid, keys = (tile, zone), where plan_slice allows the loop (SliceState::fused_ok)
    DevArray<uint32_t> d_ftab;       // FusedTab per tile
    // persistent form of that loop (k_fused_loop, bf_loop.hip): a context ALONE on the GPU keeps the work-groups resident
    bool counted = false;            // in g_live_ctx
    int opt_persist = 1;             // 0 never, 1 for warm-started runs of the one-kernel loop on a context that is not co-scheduled, 2 cold runs too
    DevArray<unsigned long long> d_xrec, d_xred;   // exchange records of the sub-tiles / of the reducers (two parities each)
    DevArray<unsigned long long> d_verdict;   // (launch id << 2) | COMMIT / ABORT of the persistent kernel's current launch (bf_loop.hip)
    HostArray<int> h_broken;         // set by the device if a committed launch could not be read back (never observed)
    DevArray<float2> d_xscratch[4];  // private product arrays of the strips' readers
    // a launch that gave up (something else holds part of the GPU) costs 0.2 s: the context then leaves the persistent kernel
    // alone for persist_backoff runs (1, 2, 4, ... 64; a launch that completes resets it)
    int persist_skip = 0, persist_backoff = 0;
    long long persist_giveups = 0;   // bf_get_stat "persist_giveups"
    // test hooks, read from the environment ONCE at bf_create (BF_DEBUG_PERSIST_ABORT / _MUTE / _SPLIT=<pass>[,late])
    int dbg_persist_abort = -1, dbg_persist_mute = -1, dbg_persist_split = -1, dbg_persist_split_late = 0;
    int dbg_margin = 0;              // BF_DEBUG_MARGIN=<n>: both loops' margin (tests: margins of 1 .. 4 pixels make events outrun their bins)
    DevArray<uint16_t> d_binid;
    DevArray<uint32_t> d_hist_cnt, d_bin_start, d_cursor;
    DevArray<uint32_t> d_armed;
    DevArray<unsigned long long> d_slabs;
    DevArray<uint16_t> d_cidx;       // compact lists: pixel index per entry (same slot count as d_slabs)
    DevArray<uint32_t> d_chdr;       // compact lists: entries per bin
    int fmt = 0;                     // what this slice's scatter hands to the stencil: 0 dense slabs, 2 event lists, 3 own pixels + margin plane (plan_slice)
    int opt_bin_compact = 1;         // 0 never, 1 when the image is sparse (decided per iteration on the device), 2 always
    // interior + margin format of a dense slice (fmt 3, bf_scatter.hip: flush_split): 0 never, 1 when it is the faster one, 2 always
    int opt_bin_split = 1;
    DevArray<unsigned long long> d_mplane[2];   // margin planes (cap_px words each), double buffered like d_plane
    DevArray<uint32_t> d_mlist;      // per bin: the pixels of the margin plane it added to in its last executed launch
    DevArray<uint32_t> d_mcount;     // per bin: entries of that list
    int m_nbins = 0, m_cap = 0;      // geometry the lists were written with
    int m_dirty_plane = -1;          // the margin plane the lists describe (-1: both planes are clean, the lists empty)
    bool m_unknown = false;          // a run did not complete: clear everything before the next use
    DevArray<uint32_t> d_ovf_bits[2];   // per plane buffer: one bit per image pixel an overflow event touched (tile-binned loop)
    int ovf_pitch = 0;               // words per image row: ceil(C / 32) + 3 (one spare word left, two right: the stencil tile's window)
    bool bin_setup_done = false;
    // per-tile optimizers (bf_run_tiles)
    DevArray<uint32_t> d_tile_hist, d_tile_start, d_tile_cursor;
    DevArray<DevState> d_tile_states;
    DevArray<uint8_t> d_ltile;       // bf_local_run_tiles: the windows' states, then their return codes
    DevArray<uint8_t> d_many_args;   // bf_run_tiles_many (lead context): the slices' launch arguments + the claim counter
    HostArray<TileArgs> h_many_args; // ... and their pinned staging copy
    // event groups (bf_set_groups / bf_set_groups_from_segments / bf_run_groups): the group id per event in upload order, the
    // groups' fr boxes (x min, x max, y min, y max), the claim order (descending event count) and the claim counter
    DevArray<int32_t> d_group_id, d_group_box;
    DevArray<uint32_t> d_group_order, d_group_counter;
    int groups_lds = 0, groups_per_cu = 0;   // what the last bf_run_groups launched: dynamic LDS bytes, work-groups per CU (bf_get_stat)
    // wide groups ("groups_wide", bf_group_rules.h): a group whose window does not fit the LDS runs the chip-wide loop on an inner
    // context of this one's capacity on this one's stream, created at the first such group and released by bf_destroy.  It is not
    // counted in g_live_ctx (it never runs beside its owner) and its "persist" is 0.
    int max_rows = 0, max_cols = 0;          // bf_create's image capacity, per axis
    bool opt_groups_wide = false;            // read by bf_run_groups
    int groups_wide = 0;                     // groups the last bf_run_groups solved wide (bf_get_stat)
    bf_ctx* wide_inner = nullptr;            // owned
    // The scratch of the entries on the K models' vote planes (bf_assign_abi.cpp, bf_track_abi.cpp; bf_hold_groups borrows the
    // staged warps), everything grown on first use.  Who owns what reads off the type; what an entry takes from `shared` or from
    // another entry's part, it takes through the helpers of bf_vote_planes.h.
    struct VoteScratch {
        // the window's options as every entry takes them (its opts struct's scale, sensor_res_x / _y and margin)
        struct Window {
            int scale, res_x, res_y, margin;
            bool operator==(const Window& o) const { return scale == o.scale && res_x == o.res_x && res_y == o.res_y && margin == o.margin; }
        };
        // shared: the K vote planes and their box sums (K x R x C words each), the K warps and their pinned staging copy
        struct Shared { DevArray<uint32_t> votes, box; DevArray<WarpParams> d_wp; HostArray<WarpParams> h_wp; } shared;
        // bf_assign_groups: the ids and scores in upload order, the result block (AssignBlock)
        struct Assign { DevArray<int32_t> gid, score; DevArray<uint32_t> d_out; HostArray<uint32_t> h_out; } assign;
        // the base pass (bf_project_groups, bf_merge_scores, bf_track_keep): per pixel N, the owner (bf_project_groups alone:
        // bf_track_keep directs it into its kept plane) and the colour, and the result block (ProjectBlock)
        struct Project {
            DevArray<uint32_t> count; DevArray<int32_t> label; DevArray<uint8_t> bgr;
            DevArray<unsigned long long> d_out; HostArray<unsigned long long> h_out;
        } project;
        // bf_merge_scores: the N plane, the trial planes of one pass and their box sums (A x K x R x C words each), the result
        // block (MergeBlock)
        struct Merge { DevArray<uint32_t> n, votes, box; DevArray<unsigned long long> d_out; HostArray<unsigned long long> h_out; } merge;
        // bf_track_keep / bf_track_overlap: the kept owner plane (R x C labels), a buffer of its own that no other entry writes,
        // what it was kept under, and the overlap's result block (TrackBlock).  The kept plane is NOT slice state: an upload leaves
        // it, bf_track_keep replaces it, bf_track_drop and bf_destroy release it -- so its validity is here and not in SliceState.
        struct TrackKept {
            bool valid = false;
            int Kp = 0;          // the groups of the kept grouping
            Window win{};        // the window's options ...
            int R = 0, C = 0;    // ... and its planes
        };
        struct Track { DevArray<int32_t> plane; TrackKept kept; DevArray<uint32_t> d_out; HostArray<uint32_t> h_out; } track;
    } vote;
    // candidate models (bf_propose_models): the lattice's value tables (n_x doubles, then n_y), the vote plane H and its box
    // sums B (n_x * n_y words each), the result block (counts, proposals); grown on first use
    DevArray<double> d_propose_tab;
    DevArray<uint32_t> d_propose_hist, d_propose_box, d_propose_out;
    HostArray<uint32_t> h_propose_out;
    int propose_form = 0;            // what the last bf_propose_models launched: 1 the LDS histogram, 2 global atomics (bf_get_stat)
    // One staging slot of the asynchronous uploads (bf_upload.cpp).  Its state:
    //   FREE      not taken;
    //   RECORDED  taken, `src` describes what to copy, no HIP call issued yet ("defer_uploads");
    //   ISSUED    the copies are on the copy stream; the staging kernels run on the compute stream at the commit;
    //   EARLY     the copies and, behind them on the copy stream, the staging kernels (widening, k_prepare) into the slot's own
    //             event arrays and pinned statistics record -- under the previous slice's solve.  The commit then only swaps
    //             those arrays with set[0]'s and makes the compute stream wait for `prepared`: no staging kernel and no
    //             statistics round trip on a warm-started chain's critical path (~35 us of a ~230 us slice at 346x260).
    struct UploadSlot {
        enum State { FREE, RECORDED, ISSUED, EARLY };
        // what the host columns hold: int32 addresses and slice-local int32 times / int32 addresses and absolute 64-bit
        // nanoseconds / 16-bit addresses and absolute nanoseconds / 16-bit addresses and the low 32 bits of those
        enum Format { LOCAL32, TS64, ADDR16_TS64, ADDR16_TS32 };
        struct Source {                   // [first, first + n) of host rings of cap entries (a flat array: first 0, cap n)
            const void *x, *y, *ts;
            const uint8_t* noise;         // Event::noise ring, or null
            long long cap, first, n;
            unsigned long long t0;        // slice start of the absolute timestamps
            Format fmt;
        };
        State state = FREE;
        Source src{};
        DevArray<int32_t> x, y, t;        // what k_prepare reads (slot 0's: also the blocking upload's, allocated at bf_create)
        DevArray<unsigned long long> ts;  // absolute timestamps (the 32-bit form uses half)
        DevArray<uint16_t> in16;          // 16-bit addresses: row[cap_events] then col[cap_events]
        DevArray<uint8_t> noise;
        EvSet inc;                        // EARLY: xy, t, p of the slice
        HostArray<SliceStats> stats;      // EARLY: k_prepare's per-work-group records
        Event copy_done;                  // the copies have landed (copy stream)
        Event staged;                     // the staging kernels that read x / y / t have run (compute stream)
        Event prepared;                   // EARLY: the staging kernels have run (copy stream)
        Event inc_free;                   // the arrays swapped INTO inc at a commit are free (compute stream is past that commit)
        bool staged_valid = false, inc_free_valid = false;
    };
    // Everything an uploading second thread touches (bf_accel.h: threading) -- and, through fold_stats, the statistics.
    struct Uploads {
        Stream stream;                    // the copy stream
        UploadSlot slot[2];
        int head = 0, count = 0;          // FIFO of taken slots: the k-th oldest is slot[(head + k) & 1]
        UploadSlot& at(int k) { return slot[(head + k) & 1]; }
    } up;
    // "defer_uploads": an asynchronous upload only takes its slot and records what to copy; its HIP calls (three copies, the
    // staging kernels, the events: ~25 us of host time) are issued by the next bf_run once that run's first batch of kernels is in
    // the queue -- or by whoever needs the slot sooner (bf_commit_upload, bf_wait_uploads).  For a single-threaded caller
    // driving one warm-started chain those 25 us otherwise sit between two runs, with the GPU idle.
    // delta scatter (bf_kernels.hip: k_warp_scatter_delta): the global-atomic loop on ONE plane buffer that is kept from launch
    // to launch -- 0 never, 1 where it is the faster loop (bf_plan.cpp: plan_run), 2 whenever the slice has no noise mask
    int opt_delta = 1;
    int last_loop = -1;              // the loop form of the last bf_run (bf_get_stat "loop_form": BF_LOOP_*; -1: no run yet)
    int opt_sep_update = 1;          // co-scheduled contexts: the update as a kernel of its own -- 0 never, 1 for event lists, 2 always (plan_run)
    bool opt_defer_uploads = false;
    std::mutex stats_mu;                          // fold_stats: bf_set_cloud's thread and an uploading thread (stage_early) may both fold
    const SliceStats* stats_src = nullptr;        // where fold_stats reads (h_stats, or the committed slot's record)
    hipEvent_t stats_event = nullptr;             // ... once this event has completed (null: the compute stream); a slot's `prepared`, not owned
    DevArray<double2> d_nxny, d_uv;
    DevArray<unsigned long long> d_plane[2];
    DevArray<uint32_t> d_cplane[2];
    DevArray<float> d_time, d_gx, d_gy, d_img;
    DevArray<uint32_t> d_count;
    DevArray<MomentAcc> d_acc;       // 3 x kAccGroups exact moment accumulators (two-kernel loop: parity of the iteration in the
                                     // first two; one-kernel loop: launch number mod 3) + one line whose first word is `lost`
    bool acc_dirty = false;          // a head-update loop leaves its last iteration's sums behind: whoever uses the
                                     // accumulators next without a loop_init of its own (a ticket-mode stencil) clears them
    DevArray<uint32_t> d_ovf;        // tile-binned loop: overflow events of iteration j in slot j % 3
    DevArray<unsigned int> d_ticket;
    DevArray<unsigned long long> d_tl;    // debug timeline (BF_TIMELINE=<file>, `make tl` build)
    const char* tl_path = nullptr;
    DevArray<DevState> d_state;      // 2 buffers: the tile-binned loop ping-pongs, everything else uses [0]
    SliceStats* d_stats = nullptr;   // = h_stats (not owned)
    DevArray<bf_trace_rec> d_trace;
    int trace_valid = 0;

    // contrast-score optimiser (bf_local.hip)
    DevArray<uint32_t> d_lplane[2];               // point planes, double buffered
    DevArray<unsigned long long> d_lscore;        // non-zero sum / count of the blurred image
    DevArray<uint8_t> d_limg;                     // project_img
    DevArray<uint8_t> d_col_planes;               // colour time image: sum cos, sum sin (i64), count (u32) point planes
    DevArray<uint8_t> d_col_img;                  // ... and its B, G, R bytes
    DevArray<uint8_t> d_flow;                     // flow field / colour-coded flow / flow frame scratch (bf_flow_abi.cpp: FlowScratch)
    HostArray<unsigned long long> h_lscore;
    bf_local_window lwin;
    int lcur = 0;
    // exhaustive search (bf_global.hip / bf_global_search.cpp)
    std::unique_ptr<GlobalSearch, GlobalSearchFree> glob;
    // segmentation (bf_segment.hip / bf_segment_abi.cpp): label, size and id planes of the image, the scan's per-work-group words,
    // the scalars, the component table (seg_K rows) and the per-event ids; grown on first use, sized from the image / the slice
    DevArray<int32_t> d_seg_lab, d_seg_sz, d_seg_nid, d_seg_cl;
    DevArray<unsigned long long> d_seg_scan;
    DevArray<SegDev> d_seg_dev;
    HostArray<SegDev> h_seg_dev;
    DevArray<bf_component> d_seg_table;
    DevArray<uint8_t> d_seg_mask;    // bf_label_image: the host mask
    int seg_K = 0;
    SliceStats stats;                // folded k_prepare statistics of the uploaded slice

    HostArray<DevState> h_state;     // D2H target only: 2 slots (pipelined polling), then h_seq
    unsigned long long* h_seq = nullptr;   // in h_state (not owned): "snapshot complete" sequence number of a warm start's batch (k_finish_update)
    unsigned long long seq_counter = 0;
    Event poll_ev[2];
    double opt_watchdog_s = 40.0;    // a cold run whose device iteration counter stands still this long is declared hung
    HostArray<SliceStats> h_stats;   // D2H target only

    DevState hst;                    // authoritative host mirror outside bf_run
    bf_window win;
    bool has_noise = false;
    bool packed = true;
    bool force_split = false;
    uint32_t run_counter = 0;
    int warm_iters_hint = 6;         // iterations the previous warm-started run needed
    DevArray<double2> d_out_tmp;     // second buffer for un-permuting outputs left in slot order (SliceState::out_sorted)
    int cur = 0;                     // plane buffer that is guaranteed all-zero
    bool planes_unknown = true;      // both buffers must be cleared before use
    int last_R = 0, last_C = 0;

    // What the last bf_run launched of the two-kernel tile-binned loop (bf_get_stat "k1_*" / "k3_*"; -1: that run launched no
    // such kernel): the scatter kernel's work-group size, events per thread and form, the stencil kernel's HS, MODE and build.
    // Host integers written next to the launches they describe (bf_run.cpp: enqueue_iteration).
    struct Launched {
        int k1_threads = -1, k1_per_thread = -1, k1_head = -1;
        int k3_half_scale = -1, k3_mode = -1, k3_capped = -1;
    } launched;

    int prof_mode = 0;
    std::vector<ProfRec> prof_pending;
    std::vector<Event> ev_pool;
    bf_profile prof;

    char err[512];
    std::mutex err_mu;   // fail() may be called from the uploading thread and the solving thread at once (see bf_accel.h: threading)
};

// the live slice's per-event flow in upload order on the device, or null (bf_operators.cpp)
extern "C" int ctx_device_uv(bf_ctx* c, const double2** uv);

// the live slice's per-event (nx, ny) in upload order on the device, a pending bf_set_model warp applied first; null when no
// warp has run (Event::reset: n = 0) or the window is degenerate (bf_operators.cpp)
extern "C" int ctx_device_nxny(bf_ctx* c, const double2** nxny);

// The held flow of the exhaustive search (bf_global_search.cpp; include/bf_accel.h, bf_global_hold_field / bf_global_hold_best)
// as the renderers and the -o table read it: address words and f32 products in the order the hold computed them in, `idx` the
// upload index of a position, (nx, ny) and (u, v) in upload order; every pointer null when n == 0.  BF_ERR_STATE (message
// set, `who` the entry point's name) when there is none for the slice uploaded now.
struct GlobalHeldFlow {
    const uint32_t* xy; const float2* p; const uint32_t* idx; const double2 *nxny, *uv;
    long long n;
};
int global_held_flow(bf_ctx* c, const char* who, GlobalHeldFlow* out);

// The per-event best state of the exhaustive search (bf_global_search.cpp) for bf_propose_models, behind the checks of a sweep
// in their order: `lattice` validated (null: the defaults), the window ready (BF_ERR_ARG without one, BF_ERR_STATE after an
// upload), then the sweep's own candidate values into xs / ys.  The three arrays are n doubles each in upload order on the
// device (null when n == 0).  global_cand_uv: Event::compute_uv as bf_global_get_events evaluates it.
struct GlobalBestState {
    const double *max_score, *best_nx, *best_ny;
    long long n;
    double nz;
};
int global_best_state(bf_ctx* c, const bf_global_search_opts* lattice, std::vector<double>& xs, std::vector<double>& ys,
                      GlobalBestState* out);
void global_cand_uv(double nx, double ny, double nz, double* u, double* v);

// The two frame tiles of the live slice (bf_local_abi.cpp, bf_frame_abi.cpp), ENQUEUED on the context stream into device memory: the 8-bit projection
// image, (scale res_x) x (scale res_y), and the colour-coded time image, (scale res_x + scale) x (scale res_y + scale) BGR.  A
// pending bf_set_model warp is applied first.  bf_projection_img / bf_color_time_img are these, a copy and a sync; bf_frame_render
// runs them into its own tiles.
extern "C" int render_projection_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_img);
// render_projection_img of n events given as arrays (address words, f32 products, noise flags or null, all in one order)
// instead of the live slice: no pending warp is applied, nothing of the live slice is read.
extern "C" int render_projection_img_of(bf_ctx* c, const uint32_t* xy, const float2* p, const uint8_t* noise, long long n,
                                        int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_img);
extern "C" int render_color_time_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_bgr);

// The launches of bf_get_time_img without its read-back (bf_operators.cpp): a pending warp applied, the current window's time and
// count images left in d_time / d_count.  BF_ERR_STATE (message set, `who` the entry point's name) without a usable window.
int ctx_time_img_pass(bf_ctx* c, const char* who);

// Which loop a slice runs (bf_plan.cpp): plan_slice once per slice, plan_run once per run; nothing else decides it.
struct SlicePlan {
    BinGrid grid{}, fgrid{};         // the tile-binned loop's bin grid (zw aside), the one-kernel iteration's sort grid
    bool binned = false, fused_ok = false, fused_shared = false;   // bf_ctx: use_binned, fused_ok, fused_shared
    int fmt = 0, zw = 0;             // bf_ctx: fmt, grid.zw
};
struct RunPlan {
    using Form = bf_rules::LoopForm;
    using Home = bf_rules::UpdateHome;
    Form form = Form::atomic;        // the loop, picked with the home of its model update by bf_rules::loop_choice
    Home home = Home::tail;
    // What the driver asks of the two, each said once.  (The scatter format stays in bf_ctx::fmt.)
    bool kept_plane() const { return form == Form::delta; }             // delta scatter: one plane buffer, kept up to date
    bool loop_kernel() const { return form == Form::persistent; }       // the persistent loop kernel
    bool one_kernel() const { return form == Form::one_kernel || form == Form::persistent; }   // (a persistent launch that gives up goes on one launch at a time)
    bool two_kernel() const { return form == Form::binned; }
    bool bin_grid() const { return one_kernel() || two_kernel(); }      // the events are sorted by tile: bf_ctx::fgrid / grid
    bool accumulate_only() const { return home != Home::tail; }          // the stencil kernel leaves the update to the next launch
    bool head() const { return home == Home::head; }
    bool separate() const { return home == Home::separate; }
    bool one_state() const { return separate() || !bin_grid(); }         // one state buffer (else launch j reads [j & 1], writes the other)
    bool acc_ring3() const { return one_kernel(); }                      // moment accumulators: the launch number mod 3 (else its parity)
    bool snapshot_a_launch_early() const { return one_kernel() || !accumulate_only(); }   // iteration count L shows in launch L - 1's snapshot, not L's
    int bin_threads = 0, ev_per_thread = 8;   // the scatter kernel's work-group size and events per thread
    bool warm_start = false, prewarp = false, first_warp = false;   // bf_set_model's warp: by the first counting sort / iteration
    bool quick_warm = false, snap_polled = false;   // polled batch by batch (a warm start expected to converge soon) / from the pinned snapshot
    double drift_limit = 1e300;      // tile-binned loops: the drift since the sort that asks for a re-bin
};
SlicePlan plan_slice(const bf_ctx* c, const bf_window& w);
// What bf_rules::loop_choice decides on, read off the context; max_iter: the run's.  (bf_get_stat "one_kernel" / "persistent" ask
// the same rules of the same facts as plan_run, with for_run = false, without taking a run of the back-off after a launch gave up.)
bf_rules::LoopFacts loop_facts(const bf_ctx* c, int max_iter, bool for_run);
RunPlan plan_run(bf_ctx* c, const bf_run_opts& o);   // (takes one run of that back-off)

// The asynchronous uploads (bf_upload.cpp): the copy stream, the slots' events and arrays (on first use); the HIP side of the
// RECORDED uploads, oldest first (one that fails is dropped with every upload behind it); every taken slot from FIFO position k
// on returned to FREE.
int streaming_setup(bf_ctx* c);
int issue_deferred_uploads(bf_ctx* c);
void drop_uploads(bf_ctx* c, int k);

// The inner context of `owner`'s wide groups (bf_context.cpp): created on first use with the owner's device, event and image
// capacity on the owner's stream, uncounted, "persist" 0.  A failure leaves the message in the owner.
int ensure_wide_inner(bf_ctx* owner);

// ---- shared helpers (bf_ctx.cpp) ----

// stores the message in the context (c may be null) and returns `code`
int fail(bf_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                      \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail((c), BF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

int prof_fold(bf_ctx* c);                     // the pending ProfScope brackets into bf_ctx::prof (synchronises the stream)
long long pad_events(long long n);            // n events padded to whole k_prepare work-groups (the event arrays' granule)
int bit_length(unsigned long long v);
// a warp by (dnx, dny) about (cx, cy), divergence div, rotation `angle` (cos / sin evaluated on the host: event.h:91-92,102-103)
void set_warp(WarpParams& w, double dnx, double dny, double cx, double cy, double div, double angle);
// set_model's warp (optimizer_rolling.h:289-299): the ONE place a bf_model becomes a warp (bf_set_model, a tile's warm start,
// the K models of bf_assign_groups / bf_project_groups)
void set_model_warp(WarpParams& w, const bf_model& m);
WarpParams identity_warp();
// OptimizerRolling::set_cloud's window (optimizer_rolling.h:263-282) of a bounding box in sensor pixels: the ONE place this
// arithmetic lives on the host (bf_set_cloud on the events' seeded box, bf_assign_groups on the widened sensor box).
bf_window window_of_box(int scale, int x_min, int x_max, int y_min, int y_max);

// Buffers allocated on first use.  The second event set and both permutations are shared by the tile-binned loops and
// bf_run_tiles: whichever comes first allocates them, and the other finds them (with the slice's events possibly IN the second set).
int ensure_cplanes(bf_ctx* c);
int ensure_ovf_bits(bf_ctx* c, int R, int C);   // dirty bitmaps of the overflow planes for an R x C image
int ensure_second_set(bf_ctx* c);
int ensure_bin_buffers(bf_ctx* c, const BinGrid& g);
int ensure_margin_buffers(bf_ctx* c, const BinGrid& g);   // margin planes and per-bin lists of the interior + margin format
int clear_planes(bf_ctx* c);
int margin_reset(bf_ctx* c);
// grow(n), and zero the array on the context's stream when that allocated it (instantiated in bf_ctx.cpp for the element types in use)
template <class T> hipError_t grow_zeroed(bf_ctx* c, DevArray<T>& a, size_t n);

// Device-conditional counting sort of the live events by the image tile of their current target (runs only when hot.need_rebin
// is set); no host synchronisation.
int enqueue_rebin(bf_ctx* c, DevState* st, bool has_perm_at_start, const WarpParams* prewarp = nullptr, bool fused = false, int launch_no = 0);
int flush_pending(bf_ctx* c);                 // applies the warp bf_set_model left pending (optimizer_rolling.h:294-298)
// Waits for an event without occupying a host core: query, sleep ~20 us (+ the kernel's timer slack), repeat.
int wait_event_sleeping(bf_ctx* c, hipEvent_t ev);
// Folds the per-work-group min / max / sum records k_prepare wrote for the uploaded slice (one device-to-host copy per slice,
// cached).  With `overwritten`, a record about to be reused: only if the slice's statistics are still unread in that record.
int fold_stats(bf_ctx* c, const SliceStats* overwritten = nullptr);
// Installs n group ids (n = c->n; `src` on the host or on the device, as `kind` says; not read when the slice is empty) as the
// held grouping of K groups: the context's own plane, held until the next upload.  A host source is free again on return.
int install_grouping(bf_ctx* c, const int32_t* src, hipMemcpyKind kind, int K);

// ---- what bf_run.cpp calls once per kernel launch: inline, the host's launch time is on a warm-started chain's critical path ----

inline Event get_event(bf_ctx* c) {
    Event e;
    if (c->ev_pool.empty()) {
        (void)e.create();
    } else {
        e = std::move(c->ev_pool.back());
        c->ev_pool.pop_back();
    }
    return e;
}

// Brackets one kernel launch with events when profiling is on.
struct ProfScope {
    bf_ctx* c;
    ProfRec r;
    bool on;
    ProfScope(bf_ctx* c_, int cat, long long nev = 0) : c(c_), on(c_->prof_mode == 1) {
        if (!on) return;
        r.a = get_event(c);
        r.b = get_event(c);
        r.cat = cat;
        r.nev = nev;
        (void)hipEventRecord(r.a, c->stream);
        // the loop kernels' launchers pick these up and time the kernel itself (bf_kernels.h: LaunchTimer)
        LaunchTimer& t = launch_timer();
        t.start = r.a; t.stop = r.b; t.consumed = false;
    }
    ~ProfScope() {
        if (!on) return;
        LaunchTimer& t = launch_timer();
        if (!t.consumed) (void)hipEventRecord(r.b, c->stream);
        t.start = t.stop = nullptr;
        t.consumed = false;
        c->prof_pending.push_back(std::move(r));
    }
};

inline EvSets ev_sets(const bf_ctx* c) {
    EvSets e;
    for (int i = 0; i < 2; ++i) {
        e.s[i].xy = c->set[i].xy; e.s[i].t = c->set[i].t; e.s[i].p = c->set[i].p; e.s[i].perm = c->set[i].perm;
        e.s[i].p2 = c->set[i].p2;
    }
    return e;
}

inline WarpScatterArgs ws_args(bf_ctx* c, int buf, int check_done) {
    WarpScatterArgs a;
    const bf_ctx::EvSet& e = c->set[c->cs];
    a.xy = e.xy; a.t = e.t; a.p = e.p;
    a.noise = c->has_noise ? c->d_noise : nullptr;
    a.nxny = c->d_nxny;
    a.uv = nullptr;
    a.perm = c->has_perm ? e.perm : nullptr;
    a.plane = c->d_plane[buf];
    a.cplane = c->d_cplane[buf];
    a.st = c->d_state;
    a.n = c->n;
    a.check_done = check_done;
    a.packed = c->packed;
    a.sets = ev_sets(c);
    a.pick_set = 0;
    a.sorted_out = 0;
    return a;
}

inline StencilArgs st_args(bf_ctx* c, int buf, int check_done) {
    StencilArgs a;
    memset(&a, 0, sizeof(a));
    a.st = c->d_state;
    a.check_done = check_done;
    a.R = c->win.scale_img_x; a.C = c->win.scale_img_y;
    a.scale = c->win.scale;
    a.tbits = c->hst.hot.tbits;
    a.tmin = c->hst.hot.tmin;
    a.plane = c->d_plane[buf];
    a.cplane = c->d_cplane[buf];
    a.zero_plane = c->d_plane[buf ^ 1];
    a.zero_cplane = (c->packed && !c->use_binned) ? nullptr : c->d_cplane[buf ^ 1];
    a.slabs = c->d_slabs;
    a.cidx = c->d_cidx; a.chdr = c->d_chdr;
    a.compact = c->fmt;
    a.m_cur = c->d_mplane[buf];
    a.g = c->grid;
    a.ovf_cur = a.ovf_prev = c->d_ovf;   // (the tile-binned loop sets the three counters per launch)
    a.cur = buf;
    return a;
}

// which k_stencil instantiation reads the plane buffers of the current slice
inline StencilSrc plane_src(const bf_ctx* c) { return c->packed ? StencilSrc::packed_plane : StencilSrc::split_planes; }

// the word behind the moment accumulators that the one-kernel loops set when an event is lost
inline uint32_t* lost_flag(const bf_ctx* c) { return reinterpret_cast<uint32_t*>(c->d_acc.get() + 3 * kAccGroups); }

