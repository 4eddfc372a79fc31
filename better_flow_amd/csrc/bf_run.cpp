// bf_run.cpp -- C-ABI: the fused OptimizerRolling::set_model / run (optimizer_rolling.h:48-125,289-347): the host side of the device loops
// (two-kernel tile-binned loop, one-kernel iteration, persistent loop kernel, global-atomic fallback and its delta-scatter form; plan_run picks one), bf_run_many,
// and bf_get_trace of the last run's per-iteration records.
#include "bf_ctx.h"

namespace {

// Debug build, BF_HOST_TIMING set: where the host thread's time goes -- launching or waiting --, printed at the end of a run.
struct HostTiming {
#ifdef BF_DEBUG_HOOKS
    bool on = [] { static const bool e = getenv("BF_HOST_TIMING") != nullptr; return e; }();
#else
    static constexpr bool on = false;
#endif
    double launch = 0, wait = 0, mark = on ? now() : 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void lap(double& into) { if (on) { const double t = now(); into += t - mark; mark = t; } }
};

// What changes while a run goes on: where the loop is, and what the host has seen of it.
struct RunLoop {
    bf_ctx* c;
    const RunPlan& p;
    // Tile-binned loop: the update of iteration j runs at the head of warp+scatter launch j + 1, so the state ping-pongs between
    // two buffers (launch j reads [j & 1], writes [(j + 1) & 1]; update in k_finish_update: ONE buffer), the moment accumulators alternate with the
    // iteration's parity (one-kernel loop: the launch number mod 3), and the overflow events of iteration j are counted in slot
    // j % 3 (slot 2 stands for "iteration -1": is plane buffer b0 ^ 1 still dirty from an earlier operator?).
    // The plane buffers alternate: an iteration scatters into `buf`, its stencil launch clears the other one, the next iteration takes
    // that one.  Delta scatter keeps b0: its first launch is the plain loop's (the other buffer may be dirty from earlier), every later
    // one moves the events that changed pixel and its stencil launch clears nothing.  The one-kernel loops touch neither buffer.
    int b0 = 0, buf = 0;             // plane buffer of the first iteration / of the next one
    bool first = true;               // no iteration launched yet
    bool delta_step() const { return p.kept_plane() && !first; }
    void next_buf() { if (!p.kept_plane()) buf ^= 1; }
    int cur_after(int it) const {    // the clean buffer after `it` executed iterations: where the next scatter goes
        if (p.one_kernel()) return b0;
        return p.kept_plane() ? (it > 0 ? b0 ^ 1 : b0) : b0 ^ (it & 1);
    }
    int launched_iters = 0;
    bool prewarp_done = false;       // a persistent round has fused the warm start's warp into its counting sort
    bf_trace_rec* trace = nullptr;
    bool want_rebin = false;         // a snapshot asked for a re-bin
    int last_rebin_at = 0;           // launched_iters when the last re-bin was enqueued
    int skip_rebin_checks = 0;       // snapshots still to come that predate it (one batch behind)
    int stall_allowance = 0;         // launches that may have been spent waiting for a re-bin (one-kernel iteration)
    unsigned long long seq_wait = 0;   // sequence number the current quick-warm batch's k_finish_update will publish (0: none)
    bool snap_polled = false;        // progress is read from the pinned snapshot (wait_snapshot)
    bool done = false;               // the device loop is over ...
    bool final_done = false;         // ... and the gated final warp already ran
    DevState fin;                    // the final state (snapshot-polled: read by run_end)
    bf_run_info inf{0, 0, 1.0f, 1.0f, 10000.0f, 10000.0f};   // (rc, iterations, the four dividers)
    HostTiming ht;
    bool split() const { return p.two_kernel() && c->fmt == 3; }   // own pixels + margin plane
    DevState* state_of(int j) const { return c->d_state + (p.one_state() ? 0 : (j & 1)); }
    MomentAcc* acc_of(int j) const { return c->d_acc + (size_t)(p.acc_ring3() ? ((j % 3) + 3) % 3 : (j & 1)) * kAccGroups; }
    uint32_t* ovf_of(int j) const { return c->d_ovf + (((j % 3) + 3) % 3) * kOvfSlotWords; }
    int finish(const DevState& s, bool warped) { fin = s; done = true; final_done = warped; return BF_OK; }   // the loop is over
};

// The run's start: the state reset on the host and (one launch) on the device, the margin planes, the persistent kernel's buffers.
int run_begin(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L) {
    DevState& h = c->hst;
    L.b0 = L.buf = c->cur;
    L.trace = o.trace_cap > 0 ? c->d_trace : nullptr;
    c->run_began();   // the loop warps the events
    h.x_div = h.y_div = 1.0f;            // :61
    h.rot_div = h.div_div = 10000.0f;    // :62-63
    h.old_dx = h.old_dy = h.old_rot = h.old_div = 0.f;
    h.hot.it = 0; h.hot.done = 0; h.rc = 0;
    h.run_tag = (int32_t)((++c->run_counter & 0x3fffffff) | 0x40000000);   // `done` is set to this (non-zero) tag
    h.max_iter = o.max_iter;
    h.hard_cap = o.hard_iter_cap;
    h.trace_cap = o.trace_cap;
    h.hot.binned = p.bin_grid() ? 1 : 0;
    h.hot.need_rebin = p.bin_grid() ? 1 : 0;   // the first enqueued re-bin builds the bins
    h.hot.rebins = 0; h.ovf_total = 0;
    h.hot.cs = c->cs; h.hot.flip = 0;
    h.hot.pp = 0; h.hot.redo = 0; h.hot.pend = 0; h.last_j = -1;
    h.hot.spare_ = 0;   // launches of the persistent loop kernel completed in THIS run (with run_tag: the launch's id)
    if (p.bin_grid()) h.drift_limit = p.drift_limit;
    // A warm start keeps bf_set_model's warp in hot.wp: the first iteration applies it, or the first counting sort does (prewarp).  In
    // that case the bins are built for the positions THAT warp gives, so it is the reference the drift bound measures from
    // (k_bin_scan: ref_wp <- hot.wp; the first pass does not warp, and the first update overwrites hot.wp).  With the identity there,
    // the first update -- whose warp is the previous model's plus one small step -- looked like a jump of the whole flow and asked
    // for a re-bin right after the one just made: one more counting sort per warm slice, and in the persistent loop one more launch
    // with its host round trip.
    if (!p.warm_start) h.hot.wp = identity_warp();
    h.ref_wp = h.hot.wp;
    launch_run_init(c->d_state, h, c->d_ovf, h.hot.ovf_cnt[L.b0 ^ 1] ? 1u : 0u, c->d_acc, p.bin_grid() || c->acc_dirty, c->stream);
    c->acc_dirty = false;
    // Interior + margin format: iteration j adds to margin plane b0 ^ (j & 1) and clears, bin by bin, what the lists say the
    // previous executed launch left in the other one.  That works across runs as long as the plane the lists describe is not
    // the one the first iteration adds to; otherwise (or after a run that did not complete) it is cleared up front.
    if (L.split()) {
        if (c->m_unknown || c->m_dirty_plane == L.b0) {
            int rcm = margin_reset(c);
            if (rcm != BF_OK) return rcm;
        }
        c->m_unknown = true;   // (until this run has completed)
    }
    if (p.accumulate_only()) c->acc_dirty = true;   // (the sums of the last iteration are consumed, not cleared)
    if (p.loop_kernel()) {
        const size_t nrec = (size_t)c->fgrid.nbr * c->fgrid.nbc * (c->fgrid.TSR / 16);
        HIP_TRY(c, grow_zeroed(c, c->d_xrec, 2 * nrec * 32));
        HIP_TRY(c, grow_zeroed(c, c->d_xred, 2 * 16 * 32));
        HIP_TRY(c, grow_zeroed(c, c->d_verdict, 8));
        bool fresh;
        HIP_TRY(c, c->h_broken.grow(16, &fresh));
        if (fresh) *c->h_broken = 0;
        for (int i = 0; i < 4; ++i) HIP_TRY(c, c->d_xscratch[i].grow((size_t)c->cap_events));
    }
    L.ht = HostTiming();   // (BF_HOST_TIMING counts from here)
    return BF_OK;
}

// The final warp: the last project_4param_reinit of iteration_step (:340-344), kept so that pr / nx / ny describe the converged
// model; n is written for compute_uv / writeout.  check_done 2: gated on `done` (it rides along with a batch).
void enqueue_final_warp(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L, int check_done, DevState* st) {
    ProfScope ps(c, 3);
    WarpScatterArgs fa = ws_args(c, L.buf, check_done);
    fa.st = st;                         // (after `done` every launch keeps both buffers identical)
    fa.pick_set = p.bin_grid() ? 1 : 0;     // the device knows which set holds the (tile-sorted) events
    fa.sorted_out = 1;
    if (o.want_uv) fa.uv = c->d_uv;     // Event::compute_uv (event.h:135-142) in the same pass
    launch_final_warp(fa, c->stream);
    L.inf.launches++;
}

// The persistent loop kernel's rounds.  One round: the (device-gated) re-bin, the loop kernel -- which returns when the loop is
// over, when a re-bin is due or after max_passes iterations --, the final warp gated on `done`, and the state for the host.  A
// round ends with a host round trip (~20 us of idle GPU); a cold run takes about one per re-bin.  Without L.done: a launch gave up.
int run_persistent(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L) {
    DevState& h = c->hst;
    for (int batch = 0;; ++batch) {
        {
            int rc = enqueue_rebin(c, c->d_state, c->has_perm, (p.prewarp && batch == 0) ? &h.hot.wp : nullptr, true, 0);
            if (rc != BF_OK) return rc;
        }
        FusedLoopArgs la;
        la.sets = ev_sets(c);
        la.ftab = c->d_ftab;
        la.st = c->d_state; la.st_other = c->d_state + 1;
        la.snap = nullptr;
        la.rec = c->d_xrec; la.red = c->d_xred;
        for (int i = 0; i < 4; ++i) la.scratch[i] = c->d_xscratch[i];
        la.trace = L.trace;
        la.nbr = c->fgrid.nbr; la.nbc = c->fgrid.nbc;
        la.R = c->win.scale_img_x; la.C = c->win.scale_img_y;
        la.max_passes = 4096;
        la.first_warp = p.first_warp ? 1 : 0;
        la.tl = c->d_tl;
        la.verdict = c->d_verdict; la.broken = c->h_broken;
        la.debug_abort = c->dbg_persist_abort; la.debug_mute = c->dbg_persist_mute;   // (test hooks: bf_create read the environment)
        la.debug_split = -1; la.debug_split_late = c->dbg_persist_split_late;
        if (c->dbg_persist_split >= 0) {   // that pass of THIS launch, made its last one
            la.debug_split = L.launched_iters + c->dbg_persist_split;
            la.max_passes = c->dbg_persist_split + 1;
        }
        L.prewarp_done = true;
        {
            ProfScope ps(c, 0, c->n);
            HIP_TRY(c, launch_fused_loop(la, c->win.scale / 2, c->fgrid.TSR, c->n_cus, c->stream));
        }
        enqueue_final_warp(c, o, p, L, 2, c->d_state);
        L.inf.launches += 4;   // (the re-bin trio, the loop kernel)
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&c->h_state[batch & 1], c->d_state, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(c->poll_ev[batch & 1], c->stream));
        if (batch == 0) {   // ("defer_uploads": the next slice's copies and staging go out now, under this round)
            const int rcd = issue_deferred_uploads(c);
            if (rcd != BF_OK) return rcd;
        }
        if (p.warm_start) {
            HIP_TRY(c, hipEventSynchronize(c->poll_ev[batch & 1]));
        } else {
            int rcw = wait_event_sleeping(c, c->poll_ev[batch & 1]);
            if (rcw != BF_OK) return rcw;
        }
        L.inf.polls++;
        const DevState& ws = c->h_state[batch & 1];
        L.launched_iters = ws.last_j + 1;
        if (L.ht.on && batch < 40)
            fprintf(stderr, "persist round %d: it %d done %d need_rebin %d redo %d last_j %d rebins %d rc %d launches %d ovf_total %u\n", batch, ws.hot.it,
                    ws.hot.done, ws.hot.need_rebin, ws.hot.redo, ws.last_j, ws.hot.rebins, ws.rc, ws.hot.spare_, ws.ovf_total);
        if (*reinterpret_cast<volatile int*>(c->h_broken.get())) {
            *c->h_broken = 0;
            return fail(c, BF_ERR_HIP, "persistent loop kernel: a committed launch could not be read back");
        }
        if (ws.hot.spare_ < 0) {
            // The launch gave up (a work-group waited 0.2 s for others that were not resident: something else holds part of
            // the GPU) and undid itself: events and state are as it found them.  The context stays away from the kernel for
            // 1, 2, 4 ... 64 runs (plan_run).
            c->persist_giveups++;
            c->persist_backoff = c->persist_backoff ? (c->persist_backoff < 64 ? 2 * c->persist_backoff : 64) : 1;
            c->persist_skip = c->persist_backoff;
            if (L.ht.on) fprintf(stderr, "persistent loop kernel gave up in round %d (last_j %d): falling back to one launch per iteration\n", batch, ws.last_j);
            L.first = ws.last_j < 0;
            h.hot.spare_ = 0;
            for (int i = 0; i < 2; ++i)
                HIP_TRY(c, hipMemcpyAsync(&c->d_state[i].hot.spare_, &h.hot.spare_, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            return BF_OK;
        }
        if (ws.hot.done) {
            c->persist_backoff = 0;   // (a run that went through: the next give-up starts at one run again)
            return L.finish(ws, true);
        }
        if (batch > 100000) return fail(c, BF_ERR_NOCONV, "device loop did not terminate");
    }
}

// One iteration of each loop: j its number, `warp` whether its launch warps the events, `snap` the pinned snapshot whoever
// computes the new state writes it to as well (null: a quick warm start).
// The one-kernel pass: warp + scatter + stencil + moments in one launch; the update at the head of the next.
int enqueue_one_kernel(bf_ctx* c, RunLoop& L, int j, bool warp, DevState* snap) {
    FusedArgs fa;
    fa.sets = ev_sets(c); fa.ftab = c->d_ftab;
    fa.st_in = L.state_of(j); fa.st_out = L.state_of(j + 1);
    fa.snap = snap;
    fa.acc_in = L.acc_of(j - 1); fa.acc_out = L.acc_of(j); fa.acc_zero = L.acc_of(j + 1);
    fa.lost = lost_flag(c); fa.trace = L.trace;
    fa.nbr = c->fgrid.nbr; fa.nbc = c->fgrid.nbc;
    fa.R = c->win.scale_img_x; fa.C = c->win.scale_img_y;
    fa.j = j; fa.warp = warp ? 1 : 0; fa.tl = c->d_tl;
    ProfScope ps(c, 0, c->n);
    HIP_TRY(c, launch_fused_pass(fa, c->win.scale / 2, c->fgrid.TSR, c->stream));
    L.inf.launches += 1;
    return BF_OK;
}

// What the two pairs' stencil launches share: the end of the arguments, the launch and the pair's accounting.
void launch_pair_stencil(bf_ctx* c, RunLoop& L, StencilArgs& a, StencilSrc src, int j, int n_cus) {
    a.trace = L.trace; a.update_mode = 1;
    a.tl = c->d_tl; a.tl_launch = j;
    ProfScope ps(c, 1);
    launch_stencil(a, src, c->stream, n_cus);
    L.inf.launches += 2;
}

// The tile-binned pair: [k_finish_update +] warp + scatter by bin, then stencil + moments.
int enqueue_binned_pair(bf_ctx* c, const RunPlan& p, RunLoop& L, int j, bool warp, DevState* snap) {
    const int buf = L.buf;
    if (p.separate()) {   // the pending update of iteration j - 1 (none at j = 0: the state's own counter says so)
        launch_finish_update(L.state_of(j), L.acc_of(j - 1), L.ovf_of(j - 1), j, buf ^ 1, L.trace, snap, c->stream);
        L.inf.launches++;
    }
    BinScatterArgs ba;
    ba.sets = ev_sets(c); ba.bin_start = c->d_bin_start; ba.slabs = c->d_slabs;
    ba.cidx = c->d_cidx; ba.chdr = c->d_chdr;
    ba.compact = c->fmt;
    ba.ovf_plane = c->d_plane[buf]; ba.ovf_cplane = c->d_cplane[buf];
    ba.ovf_bits = c->d_ovf_bits[buf]; ba.ovf_pitch = c->ovf_pitch;
    ba.st_in = L.state_of(j); ba.st_out = L.state_of(j + 1);
    ba.acc = p.head() ? L.acc_of(j - 1) : nullptr;
    ba.ovf_cur = L.ovf_of(j); ba.ovf_prev = L.ovf_of(j - 1);
    ba.snap = snap; ba.trace = L.trace; ba.g = c->grid;
    ba.cur = buf; ba.j = j;
    ba.tl = c->d_tl ? c->d_tl + 64 * 2 * 16 : nullptr;
    ba.m_cur = c->d_mplane[buf]; ba.m_prev = c->d_mplane[buf ^ 1];
    ba.mlist = c->d_mlist; ba.mcount = c->d_mcount; ba.mcap = c->m_cap;
    { ProfScope ps(c, 0, c->n); HIP_TRY(c, launch_bin_warp_scatter(ba, warp, p.bin_threads, p.ev_per_thread, c->stream)); }
    c->launched.k1_threads = p.bin_threads; c->launched.k1_per_thread = p.ev_per_thread; c->launched.k1_head = p.head() ? 1 : 0;
    StencilArgs a = st_args(c, buf, 1);
    a.ovf_bits = c->d_ovf_bits[buf]; a.zero_bits = c->d_ovf_bits[buf ^ 1]; a.ovf_pitch = c->ovf_pitch;
    a.zero_full = j == 0 ? 1 : 0;   // (what an earlier operator left in the other buffer is not in the bitmap)
    a.ovf_cur = L.ovf_of(j); a.ovf_prev = L.ovf_of(j - 1); a.ovf_next = L.ovf_of(j + 1);
    // Which work-group takes which tile (same bits either way).  Bands of tile rows per residue class mod 8 of the launch
    // id -- neighbouring tiles' shared halo then meets in one L2 -- for the slab formats of contexts that share the GPU:
    // config 2 with four contexts in flight 206.3 -> 212.3 Mevents/s, the stencil kernel 15.7 -> 15.1 us and the lean
    // scatter kernel 14.3 -> 14.1 us per launch.  Launch order where the bands LOST (experiments/tile_order.md): a context
    // alone on the GPU (the scatter launch that FOLLOWS a banded stencil launch is 1.5 - 1.7 us slower there, 8.3 -> 9.8
    // and 9.3 -> 11.0 us, against 0.4 - 0.7 us gained in the stencil kernel) and event lists (config 5, 16 slices: 3.63 ->
    // 3.57 Mevents/s).
    a.tile_bands = (!p.head() && c->fmt != 2) ? 1 : 0;
    if (p.accumulate_only()) {   // the update runs at the head of the next warp+scatter launch (or in its own kernel)
        a.st = L.state_of(j + 1);
        a.acc = L.acc_of(j); a.acc_zero = L.acc_of(j + 1);
    } else {   // "co_schedule": the last work-group of the stencil kernel updates
        a.acc = c->d_acc; a.ticket = c->d_ticket;
        // it reads the state the (lean) scatter kernel read and writes the new one where the next scatter
        // launch looks for it -- and to the pinned snapshot the host polls; nobody copies the state in between
        a.st = L.state_of(j); a.st_rw = L.state_of(j + 1);
        a.snap = snap;
    }
    // (contexts of this process sharing the GPU -- g_live_ctx, read per launch: they come and go -- hold CU slots too.  For event
    // lists (large sparse images) count the GPU as full whatever this grid's size, i.e. take the stencil kernel's build that fits 8
    // work-groups per CU: config 5 with four contexts 3.27 against 2.90 Mevents/s.  Dense tiles on a grid that does not fill
    // the GPU by itself keep the plain build: config 2 with four contexts 208.3 against 206.5, round 5 -- since its
    // instruction diet the kernel gains less from two more work-groups per CU than it loses to the spills.)
    const bool shared_lists = c->opt_co_schedule && c->fmt == 2 && g_live_ctx[c->device & 63].load() > 1;
    const int k3_cus = shared_lists ? 1 : c->n_cus;
    launch_pair_stencil(c, L, a, StencilSrc::binned, j, k3_cus);
    // (launch_stencil_binned picks its build by the same rule from the same numbers)
    c->launched.k3_half_scale = bf_rules::stencil_half_scale(a.scale);
    c->launched.k3_mode = bf_rules::stencil_mode(a.compact);
    c->launched.k3_capped = bf_rules::stencil_capped(bf_rules::stencil_tiles(a.R, a.C), k3_cus) ? 1 : 0;
    return BF_OK;
}

// The plane pair: warp + scatter with one global atomic per event (a delta step: per event that changed pixel), then stencil +
// moments, whose last work-group reduces and runs the model / loop update.
void enqueue_plane_pair(bf_ctx* c, const RunPlan& p, RunLoop& L, int j, bool warp, DevState* snap) {
    {
        ProfScope ps(c, 0, c->n);
        if (L.delta_step()) launch_warp_scatter_delta(ws_args(c, L.buf, 1), c->stream);
        else launch_warp_scatter(ws_args(c, L.buf, 1), warp, true, false, c->stream);
    }
    StencilArgs a = st_args(c, L.buf, 1);
    if (L.delta_step()) a.zero_plane = nullptr, a.zero_cplane = nullptr;
    a.acc = c->d_acc; a.ticket = c->d_ticket; a.st_rw = c->d_state;
    if (p.kept_plane()) a.snap = snap;   // (polled like the tile-binned loop: wait_snapshot)
    // Delta scatter on a packed plane: the tile-binned loop's stencil kernel reading the plane itself (one load per pixel
    // of the halo plane where it merges 2 x 2 slabs), in banded tile order when contexts share the GPU -- k_stencil takes
    // half as long again per launch (experiments/round_8.md).  Split planes keep k_stencil.
    const bool plane_k3 = p.kept_plane() && c->packed && (unsigned long long)a.R * (unsigned long long)a.C < (1ull << 28);
    if (plane_k3) a.tile_bands = c->opt_co_schedule ? 1 : 0;
    launch_pair_stencil(c, L, a, plane_k3 ? StencilSrc::plane_binned : plane_src(c), j, c->n_cus);
}

int enqueue_iteration(bf_ctx* c, const RunPlan& p, RunLoop& L) {
    const bool warp = L.first ? p.first_warp : true;
    const int j = L.launched_iters;
    DevState* const snap = p.quick_warm ? nullptr : &c->h_state[0];
    int rc = BF_OK;
    switch (p.form) {
        case RunPlan::Form::one_kernel: case RunPlan::Form::persistent: rc = enqueue_one_kernel(c, L, j, warp, snap); break;
        case RunPlan::Form::binned: rc = enqueue_binned_pair(c, p, L, j, warp, snap); break;
        case RunPlan::Form::atomic: case RunPlan::Form::delta: enqueue_plane_pair(c, p, L, j, warp, snap); break;
    }
    if (rc != BF_OK) return rc;
    L.first = false; L.next_buf();
    ++L.launched_iters;
    return BF_OK;
}

// One batch: the re-bin when one is due, the iterations, and (quick warm start) the last one's update and the gated final warp.
int enqueue_batch(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L, int batch) {
    // The re-bin kernels are device-gated (they run only if hot.need_rebin is set), but even a
    // no-op launch costs ~4.5 us here, so they are enqueued only before the first iteration and
    // when a polled snapshot shows the update asking for one.  The request is predictive
    // (0.6 x margin of drift), which covers the one-to-two batches of polling lag; anything
    // that still escapes takes the exact overflow path.
    if (p.bin_grid() && (batch == 0 || L.want_rebin)) {
        int rc = enqueue_rebin(c, L.state_of(L.launched_iters), c->has_perm, (p.prewarp && batch == 0 && !L.prewarp_done) ? &c->hst.hot.wp : nullptr,
                               p.one_kernel(), L.launched_iters);
        if (rc != BF_OK) return rc;
        L.inf.launches += 3;
        L.want_rebin = false;
        L.skip_rebin_checks = 1;   // the next snapshot predates this re-bin
        L.last_rebin_at = L.launched_iters;
        if (p.one_kernel() && batch > 0) L.stall_allowance += 3 * o.poll_interval;
    }
    int batch_len = o.poll_interval;
    if (p.quick_warm) {
        // One more iteration than the previous warm start needed, then two at a time -- and, where the previous one needed
        // seven or more (a 640x480 stream: 5 .. 14 per slice), two more and then four at a time: a launch that finds the loop
        // over costs ~2 us, a second look at the batch ~28 us (blocking poll, follow-up launches, another gated final warp).
        // The first batch may be two polling intervals long (it was capped at one -- 8 -- which sent every slice of 9+
        // iterations through extra polls: config 3 averaged 2.2 looks per slice).
        const bool longish = c->warm_iters_hint >= 7;
        batch_len = batch == 0 ? c->warm_iters_hint + (longish ? 2 : 1) : (longish ? 4 : 2);
        if (batch_len < 2) batch_len = 2;
        if (batch_len > 2 * o.poll_interval) batch_len = 2 * o.poll_interval;
    }
    for (int k = 0; k < batch_len; ++k) {
        int rc = enqueue_iteration(c, p, L);
        if (rc != BF_OK) return rc;
    }
    if (p.quick_warm) {
        // A warm start is polled batch by batch (no pipelining: it rarely needs a second batch), and the
        // final warp rides along with every batch, gated on `done` (check_done 2) and picking the event
        // set on the device: when the batch was enough -- the usual case -- nothing is left to launch
        // after the poll (a blocking poll + launch costs ~20 us of idle GPU).
        const int n = L.launched_iters;
        if (p.accumulate_only()) {   // `done` of the batch's last iteration: apply its update now (normally the next launch would)
            L.seq_wait = ++c->seq_counter;
            launch_finish_update(L.state_of(n), L.acc_of(n - 1), L.ovf_of(n - 1), n, L.buf ^ 1, L.trace, &c->h_state[batch & 1], c->stream,
                                 p.one_kernel() ? lost_flag(c) + (n + 2) % 3 : nullptr, c->h_seq, L.seq_wait);
            L.inf.launches++;
        }
        enqueue_final_warp(c, o, p, L, 2, L.state_of(n));
    }
    if (batch == 0) {   // ("defer_uploads": the next slice's copies and staging go out now, under this batch)
        const int rcd = issue_deferred_uploads(c);
        if (rcd != BF_OK) return rcd;
    }
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// The host's guard against a device loop that does not end at the iteration cap.
int check_iteration_cap(bf_ctx* c, const bf_run_opts& o, const RunLoop& L) {
    if (L.launched_iters - L.stall_allowance > (o.hard_iter_cap > 0 ? o.hard_iter_cap : INT_MAX - 64) + 3 * o.poll_interval)
        return fail(c, BF_ERR_NOCONV, "device loop did not terminate");
    return BF_OK;
}

// Tile-binned cold run: no copy command, no event.  Whoever computes the new state -- work-group 0 of the warp+scatter launch
// (update at its head) or the stencil kernel's last work-group (update in its tail) -- writes it to pinned host memory as well;
// its first 8-byte word -- (done, it), one lane's store -- tells the host how far the device is and whether the loop is over.
// The host feeds the next batch when less than one is left in the queue and sleeps in between.  `done` is 0 while the loop runs
// and takes this run's tag when it ends (an earlier run's straggler leaves an older tag: read as `it` 0).  The watchdog is a
// wall-clock deadline since the device's iteration counter last moved: one batch can legitimately take long (large
// poll_interval, 1280x720 iterations, several contexts sharing the GPU, a first launch loading code objects).
int wait_snapshot(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L) {
    const volatile unsigned long long* w0p = reinterpret_cast<const volatile unsigned long long*>(&c->h_state[0]);
    const volatile int32_t* rebin_p = &c->h_state[0].hot.need_rebin;
    const volatile unsigned long long* lastj_p = reinterpret_cast<const volatile unsigned long long*>(&c->h_state[0].run_tag);
    const int32_t tag = c->hst.run_tag;
    bool done_seen = false;
    int gpu_it = 0;
    L.ht.lap(L.ht.launch);
    auto wd_clock = [] { return std::chrono::steady_clock::now(); };
    auto wd_mark = wd_clock();
    int wd_it = -1;
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long w0 = *w0p;
        const int32_t sdone = (int32_t)(uint32_t)(w0 & 0xffffffffull), sit = (int32_t)(uint32_t)(w0 >> 32);
        if (sdone == tag) { done_seen = true; break; }
        gpu_it = (sdone == 0) ? sit : 0;
        // (one-kernel iteration: progress is counted in LAUNCHES -- passes that wait for a re-bin, or repeat one,
        // do not advance the iteration counter)
        if (p.one_kernel()) {
            const unsigned long long wj = *lastj_p;   // (run_tag, last_j): one 8-byte store of the device
            gpu_it = ((int32_t)(uint32_t)(wj & 0xffffffffull) == tag) ? (int32_t)(uint32_t)(wj >> 32) + 1 : 0;
        }
        if (L.launched_iters - gpu_it <= o.poll_interval) break;   // less than a batch left in the queue: feed it
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
        if (gpu_it != wd_it) { wd_it = gpu_it; wd_mark = wd_clock(); }
        else if ((spins & 1023u) == 0 &&
                 std::chrono::duration<double>(wd_clock() - wd_mark).count() > c->opt_watchdog_s) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e != hipSuccess && e != hipErrorNotReady) HIP_TRY(c, e);
            return fail(c, BF_ERR_HIP, "device loop makes no progress");
        }
    }
    L.ht.lap(L.ht.wait);
    L.inf.polls++;
    if (done_seen) { L.done = true; return BF_OK; }
    // (a snapshot older than the last re-bin does not count.  With the update at the scatter head the snapshot of
    // iteration count L is written by launch L itself, behind a re-bin enqueued at L; with the update in the stencil
    // tail -- and in the one-kernel loop -- it is written by launch L - 1, ahead of that re-bin)
    if ((p.snapshot_a_launch_early() ? gpu_it > L.last_rebin_at : gpu_it >= L.last_rebin_at) && gpu_it > 0 && *rebin_p) L.want_rebin = true;
    return check_iteration_cap(c, o, L);
}

// A quick warm start looks at the batch it has just launched.  Update at the scatter head: k_finish_update has stored the state in
// the pinned snapshot itself and, behind a system-scope fence, this batch's sequence number -- the host spins on that word and has
// the model while the final warp (whose results stay on the device) is still running.  A bounded spin: past 2 ms the event decides.
int wait_quick_warm(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L, int batch) {
    if (!p.accumulate_only())   // (else k_finish_update has written the state to the pinned copy itself)
        HIP_TRY(c, hipMemcpyAsync(&c->h_state[batch & 1], L.state_of(L.launched_iters), sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->poll_ev[batch & 1], c->stream));
    bool seen = false;
    if (L.seq_wait) {
        const volatile unsigned long long* sp = c->h_seq;
        const auto t_spin = std::chrono::steady_clock::now();
        for (unsigned spins = 0; !seen; ++spins) {
            if (*sp == L.seq_wait) { seen = true; break; }
#if !defined(__HIP_DEVICE_COMPILE__)
            asm volatile("pause" ::: "memory");
#endif
            if ((spins & 4095u) == 4095u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spin).count() > 2e-3) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) HIP_TRY(c, hipEventSynchronize(c->poll_ev[batch & 1]));
    L.inf.polls++;
    const DevState& ws = c->h_state[batch & 1];
    if (ws.hot.done) return L.finish(ws, true);
    // (a warm start's follow-up batches are two iterations long: a re-bin -- three kernels, ~30 us on a large image --
    // pays only where the overflow path would cost more, i.e. when a good part of the events took it)
    // (the one-kernel loop has no overflow path: it WAITS for the re-bin it asks for)
    if (p.bin_grid() && ws.hot.need_rebin && (p.one_kernel() || (unsigned long long)ws.last_ovf * 8ull > (unsigned long long)ws.n_events)) L.want_rebin = true;
    return check_iteration_cap(c, o, L);
}

// A cold run that is not snapshot-polled is polled one batch behind the launches, so its wait can sleep (the wake-up latency hides
// behind the batch already queued) instead of burning a host core per slice context.
int wait_one_batch_behind(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L, int batch) {
    HIP_TRY(c, hipMemcpyAsync(&c->h_state[batch & 1], L.state_of(L.launched_iters), sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->poll_ev[batch & 1], c->stream));
    if (batch == 0) return BF_OK;
    L.ht.lap(L.ht.launch);
    const int rc = wait_event_sleeping(c, c->poll_ev[(batch - 1) & 1]);
    if (rc != BF_OK) return rc;
    L.ht.lap(L.ht.wait);
    L.inf.polls++;
    const DevState& snap = c->h_state[(batch - 1) & 1];
    if (snap.hot.done) return L.finish(snap, false);
    if (L.skip_rebin_checks > 0) --L.skip_rebin_checks;
    else if (p.bin_grid() && snap.hot.need_rebin) L.want_rebin = true;
    return check_iteration_cap(c, o, L);
}

// The run's end: the final warp unless it rode along, the final state, and what it means for the context and for the caller.
int run_end(bf_ctx* c, const bf_run_opts& o, const RunPlan& p, RunLoop& L, bf_model* model_out, bf_run_info* info) {
    if (L.ht.on)
        fprintf(stderr, "bf_run host time: launching %.3f ms, waiting %.3f ms, %d launches\n", 1e3 * L.ht.launch, 1e3 * L.ht.wait, (int)L.inf.launches);
    if (!L.final_done) enqueue_final_warp(c, o, p, L, 0, L.state_of(L.launched_iters));
    if (L.snap_polled) {   // the final state, consistently: behind everything that is queued
        HIP_TRY(c, hipMemcpyAsync(&c->h_state[1], L.state_of(L.launched_iters), sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(c->poll_ev[1], c->stream));
        {
            int rcw = wait_event_sleeping(c, c->poll_ev[1]);
            if (rcw != BF_OK) return rcw;
        }
        L.fin = c->h_state[1];
    }
    if (p.bin_grid()) c->sorted_by_plan(L.fin.hot.cs);   // the device chose which set holds the (tile-sorted) events
    if (p.warm_start) c->warm_iters_hint = L.fin.hot.it;
    c->run_ended(o.want_uv != 0);
    HIP_TRY(c, hipGetLastError());
    // (want_uv: the final warp writes the per-event flow into d_uv; whoever reads it -- bf_compute_uv, bf_compute_uv_ring, the
    // writers -- does so on this stream, behind it: the run does not wait for it.  It used to drain the stream here, which kept a
    // warm-started slice's ~15 MB of flow output on the chain's critical path.)

    const DevState d = L.fin;
    DevState& h = c->hst;
    h = d;   // model, dividers, warp parameters, plane-buffer dirtiness
    h.hot.pp = 0; h.hot.redo = 0; h.hot.pend = 0;   // (the final warp left the products in the set's first array)
    if (L.split()) {   // the last executed iteration added to margin plane b0 ^ ((it - 1) & 1), and the lists name those pixels
        if (d.hot.it > 0) c->m_dirty_plane = L.b0 ^ ((d.hot.it - 1) & 1);
        c->m_unknown = d.rc < 0;   // (a run stopped at the iteration cap may have one executed launch more than `it` counts)
    }
    if (p.two_kernel()) {   // the last iteration scattered its overflow events into buffer b0 ^ ((it - 1) & 1); the other one is clean
        h.hot.ovf_cnt[L.b0 ^ (d.hot.it & 1)] = 0;
        h.hot.ovf_cnt[L.b0 ^ (d.hot.it & 1) ^ 1] = d.last_ovf ? 1u : 0u;
    }

    c->cur = L.cur_after(d.hot.it);   // the next scatter goes to the clean buffer (one-kernel loops: hot.ovf_cnt came back as it went)
    c->trace_valid = d.hot.it < o.trace_cap ? d.hot.it : o.trace_cap;
    L.inf.rc = d.rc;
    L.inf.iterations = d.hot.it;
    L.inf.x_divider = d.x_div; L.inf.y_divider = d.y_div;
    L.inf.rot_divider = d.rot_div; L.inf.div_divider = d.div_div;
    L.inf.rebins = d.hot.rebins;
    L.inf.overflow_events = (int32_t)(d.ovf_total > 0x7fffffffu ? 0x7fffffffu : d.ovf_total);
    if (model_out) *model_out = d.model;
    if (info) *info = L.inf;
    if (d.rc < 0) return fail(c, d.rc, "iteration cap (%d) reached without convergence", o.hard_iter_cap);
    return d.rc;
}

}  // namespace

extern "C" {

int bf_set_model(bf_ctx* c, const bf_model* model) {
    if (!c || !model) return BF_ERR_ARG;
    if (!c->have_window) return fail(c, BF_ERR_STATE, "bf_set_model before bf_set_cloud");
    if (c->degenerate) {   // nothing to warp; get_model() still returns what was set
        c->hst.model = *model;
        return BF_OK;
    }
    // optimizer_rolling.h:289-299: model <- m; warp(-total_dx, -total_dy, cx, cy, total_div, -total_rot)
    c->hst.model = *model;
    set_model_warp(c->hst.hot.wp, *model);
    c->warp_pending();
    return BF_OK;
}

int bf_run(bf_ctx* c, const bf_run_opts* opts_in, bf_model* model_out, bf_run_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->have_window) return fail(c, BF_ERR_STATE, "bf_run before bf_set_cloud");
    bf_run_opts o;
    if (opts_in) o = *opts_in; else bf_run_opts_default(&o);
    if (o.poll_interval < 1) o.poll_interval = 1;
    HIP_TRY(c, hipSetDevice(c->device));
    const bf_window& w = c->win;

    // optimizer_rolling.h:49-55 (integer arithmetic) and :57-58
    const bool noise = (w.scale_img_x < w.scale * o.res_x / 15) && (w.scale_img_y < w.scale * o.res_y / 15);
    if (noise) c->all_noise_marked();   // "for (auto &e : *events) e.noise = true;"
    if (noise || c->n < (long long)o.min_events) {
        if (model_out) *model_out = c->hst.model;
        if (info) *info = bf_run_info{BF_SKIPPED, 0, 1.0f, 1.0f, 10000.0f, 10000.0f};
        c->last_loop = -1;
        return BF_SKIPPED;
    }

    if (o.trace_cap > 0) HIP_TRY(c, c->d_trace.grow((size_t)o.trace_cap));
    const RunPlan p = plan_run(c, o);
    c->launched = bf_ctx::Launched{};
    RunLoop L{c, p};
    int rc = run_begin(c, o, p, L);
    if (rc == BF_OK && p.loop_kernel()) rc = run_persistent(c, o, p, L);
    if (rc != BF_OK) return rc;
    c->last_loop = (int)((p.loop_kernel() && !L.done) ? RunPlan::Form::one_kernel : p.form);   // (a persistent launch gave up: the loop that finishes the run)
    // Pipelined polling: batch b+1 is enqueued BEFORE the host waits for the state snapshot
    // taken after batch b, so the GPU never idles on the host (a blocking poll costs ~25 us of
    // idle GPU).  Kernels launched after `done` was set return at once (~1 us each).
    L.snap_polled = p.snap_polled && !L.done;   // (not after persistent rounds that ended the loop)
    if (L.snap_polled) {
        *reinterpret_cast<volatile unsigned long long*>(&c->h_state[0]) = 0ull;
        *reinterpret_cast<volatile unsigned long long*>(&c->h_state[0].run_tag) = 0ull;
    }
    for (int batch = 0; !L.done; ++batch) {
        rc = enqueue_batch(c, o, p, L, batch);
        if (rc == BF_OK) rc = L.snap_polled ? wait_snapshot(c, o, p, L)
                            : p.quick_warm ? wait_quick_warm(c, o, p, L, batch) : wait_one_batch_behind(c, o, p, L, batch);
        if (rc != BF_OK) return rc;
    }
    return run_end(c, o, p, L, model_out, info);
}

int bf_run_many(bf_ctx* const* ctxs, int32_t n, const bf_run_opts* opts, bf_model* models_out, bf_run_info* infos_out) {
    if (!ctxs || n < 0) return BF_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return BF_ERR_ARG;
        for (int k = 0; k < i; ++k)
            if (ctxs[k] == ctxs[i]) return fail(ctxs[i], BF_ERR_ARG, "bf_run_many: context %d is also context %d (a context holds one slice)", i, k);
    }
    std::vector<int> rc((size_t)n, BF_OK);
    auto one = [&](int i) {
        bf_model m;
        bf_run_info inf;
        memset(&m, 0, sizeof(m));   // (a run refused before it starts writes neither)
        memset(&inf, 0, sizeof(inf));
        rc[(size_t)i] = bf_run(ctxs[i], opts, &m, &inf);
        if (models_out) models_out[i] = m;
        if (infos_out) { infos_out[i] = inf; infos_out[i].rc = rc[(size_t)i]; }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n; ++i) th.emplace_back(one, i);
    if (n > 0) one(0);
    for (auto& t : th) t.join();
    for (int i = 0; i < n; ++i)
        if (rc[(size_t)i] < 0) return rc[(size_t)i];
    return BF_OK;
}

int bf_get_trace(bf_ctx* c, bf_trace_rec* out, int32_t cap, int32_t* written) {
    if (!c || !out || cap < 0) return BF_ERR_ARG;
    int n = c->trace_valid < cap ? c->trace_valid : cap;
    HIP_TRY(c, hipSetDevice(c->device));
    if (n > 0) {
        HIP_TRY(c, hipMemcpyAsync(out, c->d_trace, (size_t)n * sizeof(bf_trace_rec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (written) *written = n;
    return BF_OK;
}

}  // extern "C"
