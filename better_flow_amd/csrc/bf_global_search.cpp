// bf_global_search.cpp -- C-ABI of the exhaustive search, OptimizerGlobal (optimizer_global.h / optimizer_global.cpp): the window
// (update_fields), one project_all, compute_flow_bruteforce over a candidate grid (per slice, and per cell of a grid over the
// sensor), and the per-event state.  The kernels are in bf_global.hip; the definitions this build adds (the per-event best
// candidate, the objective S, the objective per cell, the candidate set of a pyramid level, the piecewise projection, the
// interpolated field, the held flow) are stated in include/bf_accel.h and DESIGN.md.
#include "bf_hold_groups.h"
#include "bf_vote_planes.h"

constexpr int kGlobalHoldBest = 3;   // GlobalSearch::Held::mode after bf_global_hold_best (1, 2: BF_GLOBAL_HOLD_CELLS / _FIELD)
constexpr int kGlobalHoldGroups = 4; // ... after bf_hold_groups
// a hold that keeps its own copy of the slot order (d_xy / d_idx): it outlives the cells and every later re-sort of the context
constexpr bool global_hold_own_order(int mode) { return mode == kGlobalHoldBest || mode == kGlobalHoldGroups; }

struct GlobalSearch {
    // the window of bf_global_set_window, the per-event state and the buffers of one batch of candidates
    bf_global_window w;
    bool have = false;
    long long n = 0;                        // events of the slice the window was set on
    GlobalGeom g;
    DevArray<double> d_state;               // 6 arrays of d_state.size() / 6 doubles (GlobalEventState)
    DevArray<uint32_t> d_pts, d_win;        // the point / window planes of one batch of candidates
    DevArray<GlobalCand> d_cands;
    DevArray<unsigned long long> d_S;
    DevArray<uint8_t> d_img;
    DevArray<float> d_scores;
    std::vector<GlobalCand> h_cands;

    // the cell grid of bf_global_set_cells: valid while `have` (bf_global_set_window clears it)
    struct Cells {
        bool have = false;
        GlobalCellGrid cg;
        int run_len = 0;
        long long n_runs = 0;
        std::vector<uint32_t> h_count;                         // events per cell
        DevArray<uint32_t> d_count, d_start, d_cxy, d_cidx;    // (d_count: the sort's counts, then its cursors)
        DevArray<int32_t> d_ct;
        DevArray<uint32_t> d_run_cell, d_run_start;
        DevArray<unsigned long long> d_block, d_best;
        DevArray<uint32_t> d_best_k;
        DevArray<long long> d_surface;
        // bf_global_project_cells: one candidate per cell and the per-cell sums S_pw(cell)
        std::vector<GlobalCand> h_pw_cands;
        DevArray<GlobalCand> d_pw_cands;
        DevArray<unsigned long long> d_pw_sums;
        // bf_global_project_field: the grid as two tables of n_cells doubles (nx, then ny) and, when asked for, the
        // per-event (nx_e, ny_e) as two arrays of n doubles; its per-cell sums go through d_pw_sums
        DevArray<double> d_field_grid, d_field_ev;
    } cells;

    // scratch of one bf_global_search_cells_pyramid call: the lattice bitmaps (one bit per k), the compaction's scratch,
    // the level's list of k, the axis tables and the seeds; d_state_save holds the per-event state while the call may
    // still fail for a short buffer
    struct Pyramid {
        DevArray<uint32_t> d_bm_eval, d_bm_level, d_bm_cnt, d_bm_offs, d_level_k;
        DevArray<uint8_t> d_scan_tmp;
        DevArray<GlobalAxis> d_tab_x, d_tab_y;
        DevArray<int32_t> d_seed;
        DevArray<double> d_state_save;
    } pyr;

    // The held flow (bf_global_hold_field / bf_global_hold_best / bf_hold_groups), of the slice the window was set on: valid while `have` and
    // mode != 0.  bf_global_set_window drops it, bf_global_set_cells drops one of the grid modes (whose address words and
    // upload indices are the cells' own d_cxy / d_cidx); an upload invalidates it with the window (bf_ctx::glob_valid).
    // The nz it was formed with (one for a grid mode, best_nz per event for the snapshot) is spent at the hold: d_p and
    // d_uv carry it.
    struct Held {
        int mode = 0;                      // 0: none, BF_GLOBAL_HOLD_CELLS, BF_GLOBAL_HOLD_FIELD, kGlobalHoldBest or kGlobalHoldGroups
        DevArray<double2> d_nxny, d_uv;    // upload order
        DevArray<float2> d_p;              // the hold's source order: the cells', or (global_hold_own_order) that of d_xy / d_idx
        DevArray<uint32_t> d_xy, d_idx;    // global_hold_own_order: the context's slot order at the hold
        DevArray<uint8_t> d_med;           // bf_group_flow_medians: the select's state (bf_hold_groups.h: MedianState)
        HostArray<uint8_t> h_med;          // ... and the pinned copy of all of it but the digit counts
        DevArray<double2> d_pr;            // bf_global_get_flow: the positions, upload order
        HostArray<double2> h_stage;        // ... and its pinned staging, 3 n pairs
        Event landed[3];                   // ... one per array: its copy has landed in h_stage
    } held;

    GlobalEventState state() const {
        GlobalEventState s;
        const long long k = (long long)(d_state.size() / 6);
        s.max_score = d_state; s.best_nx = d_state + k; s.best_ny = d_state + 2 * k; s.best_nz = d_state + 3 * k;
        s.best_pr_x = d_state + 4 * k; s.best_pr_y = d_state + 5 * k;
        return s;
    }
};

void GlobalSearchFree::operator()(GlobalSearch* g) const { delete g; }

namespace {

constexpr long long kGlobalBatchBytes = 512ll << 20;   // point + window planes of one batch
constexpr int kGlobalMaxBatch = 32;
constexpr long long kGlobalMaxCandidates = 1ll << 26;
constexpr long long kGlobalMaxCells = 1ll << 16;
constexpr long long kGlobalMaxCellSurface = 1ll << 27;   // entries: 1 GiB of int64

GlobalCand make_cand(double nx, double ny, double nz) {
    GlobalCand k;
    k.nx = nx; k.ny = ny; k.nz = nz;
    k.kx = (float)((double)(float)nx / nz);   // event.h:164-165: float(nx) / nz, a double division rounded to float
    k.ky = (float)((double)(float)ny / nz);
    return k;
}

// buffers for batches of up to `nb` candidates of the current window
int ensure_batch(bf_ctx* c, GlobalSearch* gs, int nb) {
    const size_t need = (size_t)nb * (size_t)gs->g.plane;
    HIP_TRY(c, gs->d_pts.grow(need));
    HIP_TRY(c, gs->d_win.grow(need));
    return BF_OK;
}

int ensure_cands(bf_ctx* c, GlobalSearch* gs, long long k) {
    HIP_TRY(c, gs->d_cands.grow((size_t)k));
    HIP_TRY(c, gs->d_S.grow((size_t)k));
    return BF_OK;
}

int global_ready(bf_ctx* c) {
    if (!c->glob || !c->glob->have) return fail(c, BF_ERR_ARG, "no window: call bf_global_set_window first");
    if (!c->uploaded || !c->glob_valid || c->n != c->glob->n)
        return fail(c, BF_ERR_STATE, "events were uploaded since bf_global_set_window: set the window again");
    return BF_OK;
}

// what a launcher of bf_global.hip returned, and the launches' own errors, as the call's result
int launch_rc(bf_ctx* c, const GlobalSearch* gs, int lr) {
    if (lr == -1) return fail(c, BF_ERR_ARG, "the 8-bit Gaussian is defined for scale <= 7");
    if (lr == -3) return fail(c, BF_ERR_ARG, "metric_wsize %d: the tile does not fit the LDS", gs->w.metric_wsize);
    if (lr != 0) return fail(c, BF_ERR_HIP, "bf_global: kernel attributes");
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// the k candidates at d_cands: S into d_S, folded into the per-event state.
// cells (may be null): the per-cell form of the fold, batch after batch; its k0 and ks advance with the batches
int run_candidates(bf_ctx* c, GlobalSearch* gs, long long k, uint8_t* d_img, float* d_scores, GlobalCells* cells = nullptr) {
    if (gs->n <= 0) return BF_OK;   // no event: every S stays 0
    static_assert(kGlobalMaxBatch <= kGlobalCellStride, "a batch must fit the cell block");
    const int B = (int)std::max(1ll, std::min((long long)kGlobalMaxBatch, kGlobalBatchBytes / (gs->g.plane * 8)));
    int rc = ensure_batch(c, gs, (int)std::min((long long)B, k));
    if (rc != BF_OK) return rc;
    const bf_ctx::EvSet& e = c->set[c->cs];
    const uint32_t* perm = c->has_perm ? e.perm : nullptr;
    for (long long b0 = 0; b0 < k; b0 += B) {
        const int nb = (int)std::min((long long)B, k - b0);
        HIP_TRY(c, hipMemsetAsync(gs->d_pts, 0, (size_t)nb * (size_t)gs->g.plane * sizeof(uint32_t), c->stream));
        rc = launch_rc(c, gs, launch_global_batch(e.xy, e.t, perm, gs->n, gs->g, gs->d_cands + b0, nb, gs->d_pts, gs->d_win, d_img,
                                                  gs->state(), gs->d_S + b0, d_scores, cells, c->stream));
        if (rc != BF_OK) return rc;
        if (cells) {
            cells->k0 += nb;
            if (cells->ks) cells->ks += nb;
        }
    }
    return BF_OK;
}

// The device's view of the cell grid for a sweep of n_cand candidates, at its first batch.
// surface: null, or [n_cells][n_cand] on the device; ks: null, or the lattice k of each candidate
GlobalCells cells_view(const GlobalSearch* gs, long long* surface, long long n_cand, const uint32_t* ks = nullptr) {
    const GlobalSearch::Cells& cs = gs->cells;
    GlobalCells cl;
    cl.xy = cs.d_cxy; cl.t = cs.d_ct; cl.idx = cs.d_cidx;
    cl.cell_start = cs.d_start; cl.run_cell = cs.d_run_cell; cl.run_start = cs.d_run_start;
    cl.n_runs = (int32_t)cs.n_runs; cl.run_len = cs.run_len; cl.n_cells = cs.cg.n_cells;
    cl.block = cs.d_block; cl.best_sum = cs.d_best; cl.best_k = cs.d_best_k;
    cl.surface = surface; cl.n_cand = n_cand; cl.k0 = 0; cl.ks = ks;
    return cl;
}

// before a search: the batch block zero, no cell has a best
int reset_cell_bests(bf_ctx* c, GlobalSearch* gs) {
    const size_t nc = (size_t)gs->cells.cg.n_cells;
    HIP_TRY(c, hipMemsetAsync(gs->cells.d_block, 0, nc * kGlobalCellStride * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->cells.d_best, 0, nc * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->cells.d_best_k, 0xff, nc * sizeof(uint32_t), c->stream));   // kGlobalNoCand
    return BF_OK;
}

// The caller's buffers (each may be null: not checked) against nc cells and a surface of nc x k entries.
// at_least: more candidates may follow (the levels of the pyramid)
int check_cell_buffers(bf_ctx* c, long long nc, long long k, const void* cells_out, int64_t cells_cap, const void* surface_out,
                       int64_t surface_cap, const char* at_least = "") {
    if (cells_out && cells_cap < nc) return fail(c, BF_ERR_ARG, "cell buffer holds %lld of %lld", (long long)cells_cap, nc);
    if (surface_out) {
        if (nc * k > kGlobalMaxCellSurface)
            return fail(c, BF_ERR_CAPACITY, "a surface of %lld cells x %lld candidates has more than 2^27 entries", nc, k);
        if (surface_cap < nc * k)
            return fail(c, BF_ERR_ARG, "cell surface buffer holds %lld of %s%lld", (long long)surface_cap, at_least, nc * k);
    }
    return BF_OK;
}

// the largest S; among equals the lowest key (null: the index itself, so the first of the largest)
long long best_of_S(const std::vector<unsigned long long>& S, const uint32_t* key = nullptr) {
    long long best = 0;
    for (long long m = 1; m < (long long)S.size(); ++m)
        if (S[(size_t)m] > S[(size_t)best] || (key && S[(size_t)m] == S[(size_t)best] && key[m] < key[best])) best = m;
    return best;
}

// The checks of a sweep and its candidate values: opts (NULL: the defaults) validated, the window ready, then the
// reference's loops (:134-135): repeated double addition, ny restarting from y_low on every row
int sweep_grid(bf_ctx* c, const bf_global_search_opts* opts, std::vector<double>& xs, std::vector<double>& ys, double& nz) {
    bf_global_search_opts o;
    bf_global_search_opts_default(&o);
    if (opts) o = *opts;
    if (!(o.x_step > 0) || !(o.y_step > 0) || !(o.x_low < o.x_hi) || !(o.y_low < o.y_hi))   // optimizer_global.cpp:110
        return fail(c, BF_ERR_ARG, "bad search range: need lo < hi and step > 0");
    if (!(o.nz > 0) || !std::isfinite(o.x_hi) || !std::isfinite(o.y_hi)) return fail(c, BF_ERR_ARG, "bad nz / range");
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    for (double v = o.x_low; v < o.x_hi; v += o.x_step) {
        xs.push_back(v);
        if ((long long)xs.size() > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "more than 2^26 candidates");
    }
    for (double v = o.y_low; v < o.y_hi; v += o.y_step) {
        ys.push_back(v);
        if ((long long)ys.size() > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "more than 2^26 candidates");
    }
    const long long k = (long long)xs.size() * (long long)ys.size();
    if (k > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "%lld candidates (more than 2^26)", k);
    nz = o.nz;
    return BF_OK;
}

// the sweep's candidates (nx outer, ny inner) onto the device, their S zeroed
int upload_cands(bf_ctx* c, GlobalSearch* gs, const std::vector<double>& xs, const std::vector<double>& ys, double nz) {
    const long long nxc = (long long)xs.size(), nyc = (long long)ys.size(), k = nxc * nyc;
    gs->h_cands.resize((size_t)k);
    for (long long i = 0; i < nxc; ++i)
        for (long long j = 0; j < nyc; ++j) gs->h_cands[(size_t)(i * nyc + j)] = make_cand(xs[(size_t)i], ys[(size_t)j], nz);
    int rc = ensure_cands(c, gs, k);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(gs->d_cands, gs->h_cands.data(), (size_t)k * sizeof(GlobalCand), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->d_S, 0, (size_t)k * sizeof(unsigned long long), c->stream));
    return BF_OK;
}

// Event::compute_uv, event.h:135-142
void cand_uv(double nx, double ny, double nz, double* u, double* v) {
    const double xy_len = std::hypot(nx, ny);
    const double speed = xy_len / (nz / (1000000000 / (1 * 10000)));
    *u = xy_len == 0 ? 0 : speed * nx / xy_len;
    *v = xy_len == 0 ? 0 : speed * ny / xy_len;
}

// lattice point k (nx outer, ny inner) and its S as the slice's answer
void write_result(bf_global_result* out, const std::vector<double>& xs, const std::vector<double>& ys, long long k,
                  unsigned long long sum) {
    if (!out) return;
    const long long nyc = (long long)ys.size();
    out->best_nx = xs[(size_t)(k / nyc)];
    out->best_ny = ys[(size_t)(k % nyc)];
    out->best_sum = (int64_t)sum;
    out->n_x = (int64_t)xs.size();
    out->n_y = nyc;
}

void write_cells(bf_global_cell_result* out, const GlobalSearch* gs, const std::vector<double>& xs, const std::vector<double>& ys,
                 double nz, const std::vector<uint32_t>& cell_k, const std::vector<unsigned long long>& cell_best) {
    const long long nyc = (long long)ys.size();
    for (size_t i = 0; out && i < cell_k.size(); ++i) {
        bf_global_cell_result& r = out[i];
        const long long b = (long long)cell_k[i];
        r.best_nx = xs[(size_t)(b / nyc)];
        r.best_ny = ys[(size_t)(b % nyc)];
        cand_uv(r.best_nx, r.best_ny, nz, &r.best_u, &r.best_v);
        r.best_sum = (int64_t)cell_best[i];
        r.best_index = b;
        r.events = (int64_t)gs->cells.h_count[i];
    }
}

// The blurred image and current_scores of one projection, for the outputs the caller asked for (a null one is neither
// rendered nor copied): begin() leaves their device buffers zeroed for the launches (d_img / d_scores: null when not asked
// for), copy_back() queues the copies to the caller.
struct ProjectionOut {
    uint8_t* img_out; float* scores_out;
    size_t img_px = 0, sc_px = 0;
    uint8_t* d_img = nullptr; float* d_scores = nullptr;
    ProjectionOut(uint8_t* img, float* scores) : img_out(img), scores_out(scores) {}
    int begin(bf_ctx* c, GlobalSearch* gs) {
        const bf_global_window& w = gs->w;
        img_px = (size_t)w.scale_bordered_img_x * (size_t)w.scale_bordered_img_y;
        sc_px = (size_t)w.scale_img_x * (size_t)w.scale_img_y;
        if (img_out) HIP_TRY(c, gs->d_img.grow(img_px));
        if (scores_out) HIP_TRY(c, gs->d_scores.grow(sc_px));
        if (img_out && img_px) HIP_TRY(c, hipMemsetAsync(gs->d_img, 0, img_px, c->stream));
        if (scores_out && sc_px) HIP_TRY(c, hipMemsetAsync(gs->d_scores, 0, sc_px * sizeof(float), c->stream));
        d_img = img_out ? gs->d_img.get() : nullptr;
        d_scores = scores_out ? gs->d_scores.get() : nullptr;
        return BF_OK;
    }
    int copy_back(bf_ctx* c, GlobalSearch* gs) const {
        if (img_out && img_px) HIP_TRY(c, hipMemcpyAsync(img_out, gs->d_img, img_px, hipMemcpyDeviceToHost, c->stream));
        if (scores_out && sc_px)
            HIP_TRY(c, hipMemcpyAsync(scores_out, gs->d_scores, sc_px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        return BF_OK;
    }
};

// The checks bf_global_project_cells and bf_global_project_field share, in their order; `who`: the entry point's name
int check_project_runs(bf_ctx* c, const char* who, const double* cell_nx, const double* cell_ny, int64_t cells_cap, double nz,
                       const int64_t* cell_sums_out, int64_t cell_sums_cap) {
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    if (!c->glob->cells.have) return fail(c, BF_ERR_ARG, "no cells: call bf_global_set_cells first");
    const long long nc = c->glob->cells.cg.n_cells;
    if (!cell_nx || !cell_ny) return fail(c, BF_ERR_ARG, "%s: no candidate grid", who);
    if (cells_cap < nc) return fail(c, BF_ERR_ARG, "candidate grid holds %lld of %lld cells", (long long)cells_cap, nc);
    if (cell_sums_out && cell_sums_cap < nc)
        return fail(c, BF_ERR_ARG, "cell sum buffer holds %lld of %lld", (long long)cell_sums_cap, nc);
    if (!(nz > 0)) return fail(c, BF_ERR_ARG, "bad nz");
    return BF_OK;
}

// The grid of the piecewise projection as one candidate per cell (kx, ky once per cell, here): a cell that has events must
// be finite in the float form the projection uses, kx and ky (1e39 is as infinite there as inf and NaN are); the entry of
// any other cell is not read.
int table_cands(bf_ctx* c, const GlobalSearch::Cells& cs, const double* cell_nx, const double* cell_ny, double nz,
                std::vector<GlobalCand>& cands) {
    const long long nc = cs.cg.n_cells;
    cands.assign((size_t)nc, make_cand(0.0, 0.0, nz));
    for (long long i = 0; i < nc; ++i) {
        if (cs.h_count[(size_t)i] == 0u) continue;
        cands[(size_t)i] = make_cand(cell_nx[i], cell_ny[i], nz);
        if (!std::isfinite(cands[(size_t)i].kx) || !std::isfinite(cands[(size_t)i].ky))
            return fail(c, BF_ERR_ARG, "the candidate of cell %lld, which has events, is not finite as a float", i);
    }
    return BF_OK;
}

// The grid of the interpolated field: every cell is a corner for its neighbours, with events or without, so all of the
// grid is read, and all of it must be finite in that float form.
int check_field_grid(bf_ctx* c, long long nc, const double* cell_nx, const double* cell_ny, double nz) {
    for (long long i = 0; i < nc; ++i) {
        const GlobalCand k = make_cand(cell_nx[i], cell_ny[i], nz);
        if (!std::isfinite(k.kx) || !std::isfinite(k.ky))
            return fail(c, BF_ERR_ARG, "the candidate of cell %lld is not finite as a float", i);
    }
    return BF_OK;
}

// The checked grid onto the device (n > 0: the slice has events), for the launches of the piecewise / the interpolated form.
// h_pw_cands / the caller's grids are read until the stream has been waited for.
int upload_table(bf_ctx* c, GlobalSearch::Cells& cs) {
    const size_t nc = (size_t)cs.cg.n_cells;
    HIP_TRY(c, cs.d_pw_cands.grow(nc));
    HIP_TRY(c, hipMemcpyAsync(cs.d_pw_cands, cs.h_pw_cands.data(), nc * sizeof(GlobalCand), hipMemcpyHostToDevice, c->stream));
    return BF_OK;
}
int upload_field_grid(bf_ctx* c, GlobalSearch::Cells& cs, const double* cell_nx, const double* cell_ny, GlobalCandField& src) {
    const size_t nc = (size_t)cs.cg.n_cells;
    HIP_TRY(c, cs.d_field_grid.grow(nc * 2));
    src.cell_nx = cs.d_field_grid;
    src.cell_ny = src.cell_nx + nc;
    HIP_TRY(c, hipMemcpyAsync(cs.d_field_grid, cell_nx, nc * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cs.d_field_grid + nc, cell_ny, nc * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return BF_OK;
}

// room for a held flow of the window's slice; best: with the hold's own copy of the slot order
int ensure_held(bf_ctx* c, GlobalSearch* gs, bool best, GlobalHeld& h) {
    GlobalSearch::Held& hd = gs->held;
    const size_t n = (size_t)gs->n;
    HIP_TRY(c, hd.d_nxny.grow(n));
    HIP_TRY(c, hd.d_uv.grow(n));
    HIP_TRY(c, hd.d_p.grow(n));
    if (best) {
        HIP_TRY(c, hd.d_xy.grow(n));
        HIP_TRY(c, hd.d_idx.grow(n));
    }
    h.nxny = hd.d_nxny; h.uv = hd.d_uv; h.p = hd.d_p;
    h.xy = best ? hd.d_xy.get() : nullptr; h.idx = best ? hd.d_idx.get() : nullptr;
    return BF_OK;
}

// The per-cell sums at d_pw_sums (have false: nothing was launched, all zero) to the host, the stream waited for, and
// their total: at most 65 536 values, added on the host after the one copy that brought them back
int fetch_cell_sums(bf_ctx* c, GlobalSearch* gs, bool have, int64_t* sum_out, int64_t* cell_sums_out) {
    const size_t nc = (size_t)gs->cells.cg.n_cells;
    std::vector<unsigned long long> sums(nc, 0ull);
    if (have)
        HIP_TRY(c, hipMemcpyAsync(sums.data(), gs->cells.d_pw_sums, nc * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long S = 0;
    for (size_t i = 0; i < nc; ++i) {
        S += sums[i];
        if (cell_sums_out) cell_sums_out[i] = (int64_t)sums[i];
    }
    if (sum_out) *sum_out = (int64_t)S;
    return BF_OK;
}

// What bf_global_project_cells and bf_global_project_field do once their own checks have passed: the slice rendered and
// scored with every event's candidate taken from `src` (a GlobalCandTable or a GlobalCandField whose device arrays the
// caller has queued the uploads of; not used when the slice has no event: then nothing is launched, every sum is 0 and the
// images are zero).  `also` (bytes 0: nothing): one more array the launches wrote, brought back with the rest.  Ends with
// the call's one synchronise: whatever host memory the caller's uploads read is free after it.
struct AlsoBack {
    void* dst = nullptr; const void* d_src = nullptr; size_t bytes = 0;
};
template <class Src>
int project_runs(bf_ctx* c, GlobalSearch* gs, const Src& src, uint8_t* img_out, float* scores_out, int64_t* sum_out,
                 int64_t* cell_sums_out, const AlsoBack& also = AlsoBack()) {
    GlobalSearch::Cells& cs = gs->cells;
    const size_t nc = (size_t)cs.cg.n_cells;
    ProjectionOut po(img_out, scores_out);
    int rc = po.begin(c, gs);
    if (rc != BF_OK) return rc;
    if (gs->n > 0) {
        HIP_TRY(c, cs.d_pw_sums.grow(nc));
        if ((rc = ensure_batch(c, gs, 1)) != BF_OK) return rc;
        HIP_TRY(c, hipMemsetAsync(cs.d_pw_sums, 0, nc * sizeof(unsigned long long), c->stream));
        HIP_TRY(c, hipMemsetAsync(gs->d_pts, 0, (size_t)gs->g.plane * sizeof(uint32_t), c->stream));
        rc = launch_rc(c, gs, launch_global_runs(cells_view(gs, nullptr, 0), gs->g, src, gs->d_pts, gs->d_win, po.d_img, po.d_scores,
                                                 cs.d_pw_sums, c->stream));
        if (rc != BF_OK) return rc;
        if (also.bytes) HIP_TRY(c, hipMemcpyAsync(also.dst, also.d_src, also.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = po.copy_back(c, gs)) != BF_OK) return rc;
    return fetch_cell_sums(c, gs, gs->n > 0, sum_out, cell_sums_out);
}

}  // namespace

extern "C" {

void bf_global_search_opts_default(bf_global_search_opts* o) {
    if (!o) return;
    o->x_low = -0.09; o->x_hi = 0.09;   // optimizer_global.cpp:106-108
    o->y_low = -0.04; o->y_hi = 0.04;
    o->x_step = 0.001; o->y_step = 0.001;
    o->nz = 127;                        // NZ, common.h:60
}

int bf_global_set_window(bf_ctx* c, int32_t scale, int32_t metric_wsize, bf_global_window* out) {
    if (!c) return BF_ERR_ARG;
    if (scale != 1 && scale != 3 && scale != 5 && scale != 7)   // odd (:188); the Gaussian is stated to 7
        return fail(c, BF_ERR_ARG, "scale must be 1, 3, 5 or 7 (got %d)", scale);
    if (metric_wsize <= 0) metric_wsize = 5 * scale;             // optimizer_global.h:27-35
    if (metric_wsize % 2 == 0 || metric_wsize > 63)              // odd (:189); 63: the packed window word
        return fail(c, BF_ERR_ARG, "metric_wsize must be odd and <= 63 (got %d)", metric_wsize);
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_global_set_window before bf_upload_events");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc != BF_OK) return rc;
    bf_global_window w;
    memset(&w, 0, sizeof(w));
    w.scale = scale;
    w.metric_wsize = metric_wsize;
    w.x_min = 0; w.y_min = 0; w.x_max = -1; w.y_max = -1;
    if (c->n > 0) {   // datastructures.h:144-147
        if ((rc = fold_stats(c)) != BF_OK) return rc;
        w.x_min = c->stats.xmin; w.x_max = c->stats.xmax;
        w.y_min = c->stats.ymin; w.y_max = c->stats.ymax;
    }
    w.scale_img_x = (w.x_max - w.x_min + 1) * scale;   // :191-194
    w.scale_img_y = (w.y_max - w.y_min + 1) * scale;
    w.scale_bordered_img_x = w.scale_img_x + metric_wsize;
    w.scale_bordered_img_y = w.scale_img_y + metric_wsize;
    const long long plane = (long long)w.scale_bordered_img_x * w.scale_bordered_img_y;
    if (plane * 8 > kGlobalBatchBytes)
        return fail(c, BF_ERR_CAPACITY, "bordered image %d x %d is too large", w.scale_bordered_img_x, w.scale_bordered_img_y);
    if (!c->glob) c->glob.reset(new GlobalSearch());
    GlobalSearch* gs = c->glob.get();
    gs->have = false;
    gs->cells.have = false;
    gs->held.mode = 0;
    c->global_window_dropped();
    HIP_TRY(c, gs->d_state.grow((size_t)c->cap_events * 6));   // (n <= cap_events: one allocation for every slice)
    GlobalGeom& g = gs->g;
    g.scale = scale; g.mw = metric_wsize;
    g.xs = w.x_min * scale; g.ys = w.y_min * scale;
    g.sx = w.scale_img_x; g.sy = w.scale_img_y;
    g.Rb = w.scale_bordered_img_x; g.Cb = w.scale_bordered_img_y;
    g.plane = plane;
    const bf_ctx::EvSet& e = c->set[c->cs];
    launch_global_reset(e.xy, c->has_perm ? e.perm : nullptr, c->n, gs->state(), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    gs->w = w;
    gs->n = c->n;
    gs->have = true;
    c->global_window_held();
    if (out) *out = w;
    return BF_OK;
}

int bf_global_project_all(bf_ctx* c, double nx, double ny, double nz, uint8_t* img_out, float* scores_out, int64_t* sum_out) {
    if (!c) return BF_ERR_ARG;
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    if ((rc = ensure_cands(c, gs, 1)) != BF_OK) return rc;
    ProjectionOut po(img_out, scores_out);
    gs->h_cands.assign(1, make_cand(nx, ny, nz));
    HIP_TRY(c, hipMemcpyAsync(gs->d_cands, gs->h_cands.data(), sizeof(GlobalCand), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->d_S, 0, sizeof(unsigned long long), c->stream));
    if ((rc = po.begin(c, gs)) != BF_OK) return rc;
    if ((rc = run_candidates(c, gs, 1, po.d_img, po.d_scores)) != BF_OK) return rc;
    unsigned long long S = 0;
    HIP_TRY(c, hipMemcpyAsync(&S, gs->d_S, sizeof(S), hipMemcpyDeviceToHost, c->stream));
    if ((rc = po.copy_back(c, gs)) != BF_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (sum_out) *sum_out = (int64_t)S;
    return BF_OK;
}

int bf_global_search(bf_ctx* c, const bf_global_search_opts* opts, bf_global_result* out, int64_t* surface_out,
                     int64_t surface_cap) {
    if (!c) return BF_ERR_ARG;
    std::vector<double> xs, ys;
    double nz = 0;
    int rc = sweep_grid(c, opts, xs, ys, nz);
    if (rc != BF_OK) return rc;
    const long long k = (long long)xs.size() * (long long)ys.size();
    if (surface_out && surface_cap < k) return fail(c, BF_ERR_ARG, "surface buffer holds %lld of %lld", (long long)surface_cap, k);
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    if ((rc = upload_cands(c, gs, xs, ys, nz)) != BF_OK) return rc;
    if ((rc = run_candidates(c, gs, k, nullptr, nullptr)) != BF_OK) return rc;
    std::vector<unsigned long long> S((size_t)k);
    HIP_TRY(c, hipMemcpyAsync(S.data(), gs->d_S, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (surface_out)
        for (long long i = 0; i < k; ++i) surface_out[i] = (int64_t)S[(size_t)i];
    const long long best = best_of_S(S);
    write_result(out, xs, ys, best, S[(size_t)best]);
    return BF_OK;
}

int bf_global_set_cells(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t cell_rows, int32_t cell_cols, bf_global_cells* out) {
    if (!c) return BF_ERR_ARG;
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    GlobalSearch::Cells& cs = gs->cells;
    cs.have = false;
    if (!global_hold_own_order(gs->held.mode)) gs->held.mode = 0;   // (a grid hold lives in the cells' order)
    if (res_x <= 0 || res_y <= 0 || cell_rows <= 0 || cell_cols <= 0)
        return fail(c, BF_ERR_ARG, "sensor %d x %d, cells %d x %d: every size must be positive", res_x, res_y, cell_rows, cell_cols);
    if (gs->n > 0 && (gs->w.x_max >= res_x || gs->w.y_max >= res_y))   // (addresses are unsigned: x_min, y_min >= 0)
        return fail(c, BF_ERR_ARG, "an event at (%d, %d) lies outside the %d x %d sensor", gs->w.x_max, gs->w.y_max, res_x, res_y);
    bf_global_cells gc;
    gc.n_cell_x = (int32_t)(((long long)res_x + cell_rows - 1) / cell_rows);
    gc.n_cell_y = (int32_t)(((long long)res_y + cell_cols - 1) / cell_cols);
    const long long nc = (long long)gc.n_cell_x * gc.n_cell_y;
    if (nc > kGlobalMaxCells) return fail(c, BF_ERR_ARG, "%lld cells (more than 65536)", nc);
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalCellGrid& cg = cs.cg;
    cg.cell_rows = cell_rows; cg.cell_cols = cell_cols; cg.n_cell_y = gc.n_cell_y; cg.n_cells = (int32_t)nc;
    cs.h_count.assign((size_t)nc, 0u);
    cs.n_runs = 0;
    cs.run_len = 64;
    HIP_TRY(c, cs.d_block.grow((size_t)nc * kGlobalCellStride));
    HIP_TRY(c, cs.d_best.grow((size_t)nc));
    HIP_TRY(c, cs.d_best_k.grow((size_t)nc));
    if (gs->n > 0) {
        const size_t n = (size_t)gs->n;
        const bf_ctx::EvSet& e = c->set[c->cs];
        HIP_TRY(c, cs.d_count.grow((size_t)nc));
        HIP_TRY(c, cs.d_start.grow((size_t)nc + 1));
        HIP_TRY(c, cs.d_cxy.grow(n));
        HIP_TRY(c, cs.d_ct.grow(n));
        HIP_TRY(c, cs.d_cidx.grow(n));
        HIP_TRY(c, hipMemsetAsync(cs.d_count, 0, (size_t)nc * sizeof(uint32_t), c->stream));
        launch_global_cell_count(e.xy, gs->n, cg, cs.d_count, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(cs.h_count.data(), cs.d_count, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // the scan, and the runs: a cell of m events is cut into ceil(m / run_len) work-groups.  Work-groups of one wave
        // unless the occupied cells hold 256 events or more on average (a 256-wide group on a 75-event cell idles 3 waves)
        std::vector<uint32_t> start((size_t)nc + 1, 0u);
        long long occupied = 0;
        for (long long i = 0; i < nc; ++i) {
            start[(size_t)i + 1] = start[(size_t)i] + cs.h_count[(size_t)i];
            occupied += cs.h_count[(size_t)i] != 0u;
        }
        if ((long long)start[(size_t)nc] != gs->n) return fail(c, BF_ERR_HIP, "bf_global_set_cells: the cell counts do not add up");
        cs.run_len = gs->n >= 256 * occupied ? 256 : 64;
        std::vector<uint32_t> run_cell, run_start;
        for (long long i = 0; i < nc; ++i)
            for (uint32_t s = start[(size_t)i]; s < start[(size_t)i + 1]; s += (uint32_t)cs.run_len) {
                run_cell.push_back((uint32_t)i);
                run_start.push_back(s);
            }
        cs.n_runs = (long long)run_cell.size();
        HIP_TRY(c, cs.d_run_cell.grow(run_cell.size()));
        HIP_TRY(c, cs.d_run_start.grow(run_start.size()));
        HIP_TRY(c, hipMemcpyAsync(cs.d_start, start.data(), start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cs.d_run_cell, run_cell.data(), run_cell.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cs.d_run_start, run_start.data(), run_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemsetAsync(cs.d_count, 0, (size_t)nc * sizeof(uint32_t), c->stream));
        launch_global_cell_order(e.xy, e.t, c->has_perm ? e.perm : nullptr, gs->n, cg, cs.d_start, cs.d_count, cs.d_cxy,
                                 cs.d_ct, cs.d_cidx, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the host vectors above are read until here)
    }
    cs.have = true;
    if (out) *out = gc;
    return BF_OK;
}

int bf_global_search_cells(bf_ctx* c, const bf_global_search_opts* opts, bf_global_result* slice_out,
                           bf_global_cell_result* cells_out, int64_t cells_cap, int64_t* cell_surface_out,
                           int64_t cell_surface_cap) {
    if (!c) return BF_ERR_ARG;
    std::vector<double> xs, ys;
    double nz = 0;
    int rc = sweep_grid(c, opts, xs, ys, nz);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    if (!gs->cells.have) return fail(c, BF_ERR_ARG, "no cells: call bf_global_set_cells first");
    const long long k = (long long)xs.size() * (long long)ys.size();
    const long long nc = gs->cells.cg.n_cells;
    if ((rc = check_cell_buffers(c, nc, k, cells_out, cells_cap, cell_surface_out, cell_surface_cap)) != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = upload_cands(c, gs, xs, ys, nz)) != BF_OK) return rc;
    std::vector<unsigned long long> S((size_t)k, 0ull), cell_best((size_t)nc, 0ull);
    std::vector<uint32_t> cell_k((size_t)nc, 0u);
    if (gs->n > 0) {   // (no event: nothing is launched, every S(k, cell) is 0)
        DevArray<long long>& d_surface = gs->cells.d_surface;
        if (cell_surface_out) HIP_TRY(c, d_surface.grow((size_t)(nc * k)));
        if ((rc = reset_cell_bests(c, gs)) != BF_OK) return rc;
        GlobalCells cl = cells_view(gs, cell_surface_out ? d_surface.get() : nullptr, k);
        if ((rc = run_candidates(c, gs, k, nullptr, nullptr, &cl)) != BF_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(S.data(), gs->d_S, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cell_best.data(), gs->cells.d_best, (size_t)nc * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(cell_k.data(), gs->cells.d_best_k, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (cell_surface_out)
            HIP_TRY(c, hipMemcpyAsync(cell_surface_out, d_surface, (size_t)(nc * k) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (cell_surface_out) {
        std::fill(cell_surface_out, cell_surface_out + nc * k, (int64_t)0);
    }
    const long long best = best_of_S(S);
    write_result(slice_out, xs, ys, best, S[(size_t)best]);
    write_cells(cells_out, gs, xs, ys, nz, cell_k, cell_best);
    return BF_OK;
}

int bf_global_search_cells_pyramid(bf_ctx* c, const bf_global_search_opts* opts, const bf_global_pyramid_opts* pyramid,
                                   const int64_t* seed_index, bf_global_result* slice_out, bf_global_cell_result* cells_out,
                                   int64_t cells_cap, int64_t* evaluated_out, int64_t evaluated_cap, int64_t* cell_surface_out,
                                   int64_t cell_surface_cap, bf_global_pyramid_info* info) {
    if (!c) return BF_ERR_ARG;
    bf_global_pyramid_opts po;
    po.levels = 1; po.factor = 2; po.radius = 1;
    if (pyramid) po = *pyramid;
    if (po.levels < 1 || po.levels > 8) return fail(c, BF_ERR_ARG, "levels must be 1..8 (got %d)", po.levels);
    if (po.factor < 2) return fail(c, BF_ERR_ARG, "factor must be >= 2 (got %d)", po.factor);
    if (po.radius < 1 || po.radius > 64) return fail(c, BF_ERR_ARG, "radius must be 1..64 (got %d)", po.radius);
    std::vector<double> xs, ys;
    double nz = 0;
    int rc = sweep_grid(c, opts, xs, ys, nz);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    if (!gs->cells.have) return fail(c, BF_ERR_ARG, "no cells: call bf_global_set_cells first");
    const long long nxc = (long long)xs.size(), nyc = (long long)ys.size(), K = nxc * nyc;
    const long long nc = gs->cells.cg.n_cells;
    const int L = po.levels;
    long long stride[8];
    stride[L - 1] = 1;
    for (int l = L - 2; l >= 0; --l) {
        stride[l] = stride[l + 1] * po.factor;
        if (stride[l] > std::max(nxc, nyc))
            return fail(c, BF_ERR_ARG, "the stride of level %d (%d^%d) exceeds the %lld x %lld lattice", l, po.factor, L - 1 - l, nxc, nyc);
    }
    if ((rc = check_cell_buffers(c, nc, 0, cells_out, cells_cap, nullptr, 0)) != BF_OK) return rc;
    const bool seeded = seed_index != nullptr;
    std::vector<int32_t> h_seed;
    if (seeded) {
        h_seed.resize((size_t)nc);
        bool any = false;
        for (long long i = 0; i < nc; ++i) {
            if (seed_index[i] < -1 || seed_index[i] >= K)
                return fail(c, BF_ERR_ARG, "seed %lld of cell %lld is outside the lattice of %lld", (long long)seed_index[i], i, K);
            h_seed[(size_t)i] = (int32_t)seed_index[i];
            any = any || (seed_index[i] >= 0 && gs->cells.h_count[(size_t)i] != 0u);
        }
        if (!any) return fail(c, BF_ERR_ARG, "the seeds leave nothing to evaluate (no cell has both events and a seed)");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    std::vector<uint32_t> evaluated;            // lattice k, evaluation order
    std::vector<unsigned long long> S;          // S(k) of them
    std::vector<std::vector<int64_t>> surf;     // per level [cell][level_count]
    std::vector<unsigned long long> cell_best((size_t)nc, 0ull);
    std::vector<uint32_t> cell_k((size_t)nc, 0u);
    long long level_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // what a level of `cnt` more candidates needs of the caller's buffers
    auto fits = [&](long long cnt) -> int {
        const long long tot = (long long)evaluated.size() + cnt;
        if (evaluated_out && evaluated_cap < tot)
            return fail(c, BF_ERR_ARG, "evaluated buffer holds %lld of at least %lld", (long long)evaluated_cap, tot);
        return check_cell_buffers(c, nc, tot, nullptr, 0, cell_surface_out, cell_surface_cap, "at least ");
    };
    if (gs->n <= 0) {
        // no event: nothing is launched.  No cell has a centre, so only the strided pass evaluates, and every S is 0
        const long long s0 = stride[0];
        const long long cnt = ((nxc + s0 - 1) / s0) * ((nyc + s0 - 1) / s0);
        if ((rc = fits(cnt)) != BF_OK) return rc;
        for (long long i = 0; i < nxc; i += s0)
            for (long long j = 0; j < nyc; j += s0) evaluated.push_back((uint32_t)(i * nyc + j));
        S.assign(evaluated.size(), 0ull);
        level_count[0] = cnt;
        if (cell_surface_out) surf.emplace_back((size_t)(nc * cnt), (int64_t)0);
    } else {
        const long long n_words = (K + 31) / 32;
        const GlobalLattice lt{nxc, nyc};
        GlobalSearch::Pyramid& py = gs->pyr;
        DevArray<long long>& d_surface = gs->cells.d_surface;
        HIP_TRY(c, py.d_bm_eval.grow((size_t)n_words));
        HIP_TRY(c, py.d_bm_level.grow((size_t)n_words));
        HIP_TRY(c, py.d_bm_cnt.grow((size_t)n_words + 1));
        HIP_TRY(c, py.d_bm_offs.grow((size_t)n_words + 1));
        const size_t tmp_bytes = global_scan_temp_bytes(n_words);
        HIP_TRY(c, py.d_scan_tmp.grow(tmp_bytes ? tmp_bytes : 1));
        HIP_TRY(c, py.d_tab_x.grow((size_t)nxc));
        HIP_TRY(c, py.d_tab_y.grow((size_t)nyc));
        std::vector<GlobalAxis> tx((size_t)nxc), ty((size_t)nyc);
        for (long long i = 0; i < nxc; ++i) {
            const GlobalCand k = make_cand(xs[(size_t)i], 0.0, nz);
            tx[(size_t)i].n = k.nx; tx[(size_t)i].k = k.kx; tx[(size_t)i].pad = 0.f;
        }
        for (long long j = 0; j < nyc; ++j) {
            const GlobalCand k = make_cand(0.0, ys[(size_t)j], nz);
            ty[(size_t)j].n = k.ny; ty[(size_t)j].k = k.ky; ty[(size_t)j].pad = 0.f;
        }
        HIP_TRY(c, hipMemcpyAsync(py.d_tab_x, tx.data(), tx.size() * sizeof(GlobalAxis), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(py.d_tab_y, ty.data(), ty.size() * sizeof(GlobalAxis), hipMemcpyHostToDevice, c->stream));
        if (seeded) {
            HIP_TRY(c, py.d_seed.grow((size_t)nc));
            HIP_TRY(c, hipMemcpyAsync(py.d_seed, h_seed.data(), (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        }
        const bool may_fail = evaluated_out || cell_surface_out;   // only a short buffer can stop the levels half way
        if (may_fail) {
            HIP_TRY(c, py.d_state_save.grow(gs->d_state.size()));
            HIP_TRY(c, hipMemcpyAsync(py.d_state_save, gs->d_state, gs->d_state.size() * sizeof(double), hipMemcpyDeviceToDevice,
                                      c->stream));
        }
        HIP_TRY(c, hipMemsetAsync(py.d_bm_eval, 0, (size_t)n_words * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(py.d_bm_level, 0, (size_t)n_words * sizeof(uint32_t), c->stream));
        if ((rc = reset_cell_bests(c, gs)) != BF_OK) return rc;
        for (int l = 0; l < L; ++l) {
            if (l == 0 && !seeded)
                launch_global_stride_mark(lt, stride[0], py.d_bm_level, c->stream);
            else
                launch_global_seed_mark(lt, stride[l], po.radius, (int)nc, gs->cells.d_start, gs->cells.d_best, gs->cells.d_best_k,
                                        seeded ? py.d_seed.get() : nullptr, py.d_bm_eval, py.d_bm_level, c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, launch_global_bitmap_scan(py.d_bm_level, n_words, py.d_bm_cnt, py.d_bm_offs, py.d_scan_tmp, tmp_bytes,
                                                 c->stream));
            uint32_t cnt32 = 0;   // the one value a level brings back: the launches below need it
            HIP_TRY(c, hipMemcpyAsync(&cnt32, py.d_bm_offs + n_words, sizeof(cnt32), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));   // (also: the previous level's copies into the vectors below are done)
            const long long cnt = (long long)cnt32;
            level_count[l] = cnt;
            if (cnt == 0) continue;
            if ((rc = fits(cnt)) != BF_OK) {
                if (!evaluated.empty()) {   // levels ran: the state goes back to what the call found
                    HIP_TRY(c, hipMemcpyAsync(gs->d_state, py.d_state_save, gs->d_state.size() * sizeof(double),
                                              hipMemcpyDeviceToDevice, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                }
                return rc;
            }
            HIP_TRY(c, py.d_level_k.grow((size_t)cnt));
            if ((rc = ensure_cands(c, gs, cnt)) != BF_OK) return rc;
            launch_global_bitmap_list(py.d_bm_level, py.d_bm_eval, n_words, py.d_bm_offs, py.d_level_k, c->stream);
            launch_global_cands_from_lattice(lt, py.d_level_k, cnt, py.d_tab_x, py.d_tab_y, nz, gs->d_cands, c->stream);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemsetAsync(gs->d_S, 0, (size_t)cnt * sizeof(unsigned long long), c->stream));
            if (cell_surface_out) HIP_TRY(c, d_surface.grow((size_t)(nc * cnt)));
            GlobalCells cl = cells_view(gs, cell_surface_out ? d_surface.get() : nullptr, cnt, py.d_level_k);
            if ((rc = run_candidates(c, gs, cnt, nullptr, nullptr, &cl)) != BF_OK) return rc;
            const size_t at = evaluated.size();
            evaluated.resize(at + (size_t)cnt);
            S.resize(at + (size_t)cnt);
            HIP_TRY(c, hipMemcpyAsync(evaluated.data() + at, py.d_level_k, (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                      c->stream));
            HIP_TRY(c, hipMemcpyAsync(S.data() + at, gs->d_S, (size_t)cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                      c->stream));
            if (cell_surface_out) {
                surf.emplace_back((size_t)(nc * cnt));
                HIP_TRY(c, hipMemcpyAsync(surf.back().data(), d_surface, (size_t)(nc * cnt) * sizeof(int64_t),
                                          hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the next level grows d_surface)
            }
        }
        HIP_TRY(c, hipMemcpyAsync(cell_best.data(), gs->cells.d_best, (size_t)nc * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(cell_k.data(), gs->cells.d_best_k, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const long long ne = (long long)evaluated.size();
    if (ne == 0) return fail(c, BF_ERR_HIP, "bf_global_search_cells_pyramid: nothing was evaluated");   // (never: checked above)
    const long long best = best_of_S(S, evaluated.data());   // the largest S, the lowest k among equals
    if (gs->n <= 0) std::fill(cell_k.begin(), cell_k.end(), evaluated[(size_t)best]);
    write_result(slice_out, xs, ys, (long long)evaluated[(size_t)best], S[(size_t)best]);
    write_cells(cells_out, gs, xs, ys, nz, cell_k, cell_best);
    for (long long m = 0; evaluated_out && m < ne; ++m) evaluated_out[m] = (int64_t)evaluated[(size_t)m];
    if (cell_surface_out) {   // the levels side by side: [cell][ne]
        long long at = 0;
        for (size_t l = 0; l < surf.size(); ++l) {
            const long long cnt = (long long)surf[l].size() / nc;
            for (long long i = 0; i < nc; ++i)
                std::copy(surf[l].begin() + i * cnt, surf[l].begin() + (i + 1) * cnt, cell_surface_out + i * ne + at);
            at += cnt;
        }
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_x = nxc; info->n_y = nyc;
        info->evaluated = ne;
        for (int l = 0; l < L; ++l) info->level_count[l] = level_count[l];
        info->levels_run = L;
    }
    return BF_OK;
}

int bf_global_project_cells(bf_ctx* c, const double* cell_nx, const double* cell_ny, int64_t cells_cap, double nz,
                            uint8_t* img_out, float* scores_out, int64_t* sum_out, int64_t* cell_sums_out,
                            int64_t cell_sums_cap) {
    if (!c) return BF_ERR_ARG;
    int rc = check_project_runs(c, "bf_global_project_cells", cell_nx, cell_ny, cells_cap, nz, cell_sums_out, cell_sums_cap);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    GlobalSearch::Cells& cs = gs->cells;
    std::vector<GlobalCand> cands;
    if ((rc = table_cands(c, cs, cell_nx, cell_ny, nz, cands)) != BF_OK) return rc;
    cs.h_pw_cands.swap(cands);   // (nothing of this object is written before every check has passed)
    HIP_TRY(c, hipSetDevice(c->device));
    if (gs->n > 0 && (rc = upload_table(c, cs)) != BF_OK) return rc;   // (h_pw_cands is read until project_runs has synchronised)
    return project_runs(c, gs, GlobalCandTable{cs.d_pw_cands}, img_out, scores_out, sum_out, cell_sums_out);
}

int bf_global_project_field(bf_ctx* c, const double* cell_nx, const double* cell_ny, int64_t cells_cap, double nz,
                            uint8_t* img_out, float* scores_out, int64_t* sum_out, int64_t* cell_sums_out,
                            int64_t cell_sums_cap, double* event_nx_out, double* event_ny_out, double* event_u_out,
                            double* event_v_out) {
    if (!c) return BF_ERR_ARG;
    int rc = check_project_runs(c, "bf_global_project_field", cell_nx, cell_ny, cells_cap, nz, cell_sums_out, cell_sums_cap);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    GlobalSearch::Cells& cs = gs->cells;
    const long long nc = cs.cg.n_cells;
    if ((rc = check_field_grid(c, nc, cell_nx, cell_ny, nz)) != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)gs->n;
    const bool want_ev = event_nx_out || event_ny_out || event_u_out || event_v_out;
    std::vector<double> ev;   // (nx_e, then ny_e) of every event
    GlobalCandField src{cs.cg, (uint32_t)(nc / cs.cg.n_cell_y), nullptr, nullptr, nz, nullptr, nullptr};
    AlsoBack ev_back;
    if (n > 0) {   // (no event: no per-event value is written)
        if ((rc = upload_field_grid(c, cs, cell_nx, cell_ny, src)) != BF_OK) return rc;
        if (want_ev) {   // (the caller's grids are read until project_runs has synchronised)
            HIP_TRY(c, cs.d_field_ev.grow(n * 2));
            ev.resize(n * 2);
            src.ev_nx = cs.d_field_ev;
            src.ev_ny = src.ev_nx + n;
            ev_back = AlsoBack{ev.data(), src.ev_nx, n * 2 * sizeof(double)};
        }
    }
    if ((rc = project_runs(c, gs, src, img_out, scores_out, sum_out, cell_sums_out, ev_back)) != BF_OK) return rc;
    for (size_t i = 0; i < ev.size() / 2; ++i) {   // u / v: compute_uv of the event's own (nx_e, ny_e), as bf_global_get_events
        if (event_nx_out) event_nx_out[i] = ev[i];
        if (event_ny_out) event_ny_out[i] = ev[n + i];
        double u, v;
        cand_uv(ev[i], ev[n + i], nz, &u, &v);
        if (event_u_out) event_u_out[i] = u;
        if (event_v_out) event_v_out[i] = v;
    }
    return BF_OK;
}

int bf_global_get_events(bf_ctx* c, double* max_score, double* best_nx, double* best_ny, double* best_pr_x, double* best_pr_y,
                         double* best_u, double* best_v) {
    if (!c) return BF_ERR_ARG;
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    const size_t n = (size_t)gs->n;
    if (n == 0) return BF_OK;
    const GlobalEventState st = gs->state();
    std::vector<double> nx(n), ny(n), nz(n);
    HIP_TRY(c, hipMemcpyAsync(nx.data(), st.best_nx, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ny.data(), st.best_ny, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(nz.data(), st.best_nz, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (max_score) HIP_TRY(c, hipMemcpyAsync(max_score, st.max_score, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (best_pr_x) HIP_TRY(c, hipMemcpyAsync(best_pr_x, st.best_pr_x, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (best_pr_y) HIP_TRY(c, hipMemcpyAsync(best_pr_y, st.best_pr_y, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        if (best_nx) best_nx[i] = nx[i];
        if (best_ny) best_ny[i] = ny[i];
        double u, v;
        cand_uv(nx[i], ny[i], nz[i], &u, &v);
        if (best_u) best_u[i] = u;
        if (best_v) best_v[i] = v;
    }
    return BF_OK;
}

int bf_global_hold_field(bf_ctx* c, const double* cell_nx, const double* cell_ny, int64_t cells_cap, double nz, int32_t mode) {
    if (!c) return BF_ERR_ARG;
    if (mode != BF_GLOBAL_HOLD_CELLS && mode != BF_GLOBAL_HOLD_FIELD)
        return fail(c, BF_ERR_ARG, "bf_global_hold_field: unknown mode %d", mode);
    int rc = check_project_runs(c, "bf_global_hold_field", cell_nx, cell_ny, cells_cap, nz, nullptr, 0);
    if (rc != BF_OK) return rc;
    GlobalSearch* gs = c->glob.get();
    GlobalSearch::Cells& cs = gs->cells;
    const long long nc = cs.cg.n_cells;
    const bool table = mode == BF_GLOBAL_HOLD_CELLS;
    std::vector<GlobalCand> cands;
    rc = table ? table_cands(c, cs, cell_nx, cell_ny, nz, cands) : check_field_grid(c, nc, cell_nx, cell_ny, nz);
    if (rc != BF_OK) return rc;
    if (table) cs.h_pw_cands.swap(cands);
    HIP_TRY(c, hipSetDevice(c->device));
    gs->held.mode = 0;   // (a failure below leaves no held flow)
    if (gs->n > 0) {
        GlobalHeld h;
        if ((rc = ensure_held(c, gs, false, h)) != BF_OK) return rc;
        const GlobalCells cl = cells_view(gs, nullptr, 0);
        if (table) {
            if ((rc = upload_table(c, cs)) != BF_OK) return rc;
            launch_global_hold(cl, GlobalCandTable{cs.d_pw_cands}, h, c->stream);
        } else {
            GlobalCandField src{cs.cg, (uint32_t)(nc / cs.cg.n_cell_y), nullptr, nullptr, nz, nullptr, nullptr};
            if ((rc = upload_field_grid(c, cs, cell_nx, cell_ny, src)) != BF_OK) return rc;
            launch_global_hold(cl, src, h, c->stream);
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the grids are the caller's, or h_pw_cands: read until here)
    }
    gs->held.mode = mode;
    return BF_OK;
}

int bf_global_hold_best(bf_ctx* c) {
    if (!c) return BF_ERR_ARG;
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    gs->held.mode = 0;
    if (gs->n > 0) {
        GlobalHeld h;
        if ((rc = ensure_held(c, gs, true, h)) != BF_OK) return rc;
        const bf_ctx::EvSet& e = c->set[c->cs];
        launch_global_hold_best(e.xy, e.t, c->has_perm ? e.perm.get() : nullptr, gs->n, gs->state(), h, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    gs->held.mode = kGlobalHoldBest;
    return BF_OK;
}

int bf_hold_groups(bf_ctx* c, const bf_model* models, int32_t n_models) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_hold_groups before bf_upload_events");
    GlobalSearch* gs = c->glob.get();
    if (!gs || !gs->have || !c->glob_valid || c->n != gs->n)
        return fail(c, BF_ERR_STATE, "bf_hold_groups: no window of the uploaded slice: call bf_global_set_window first");
    if (!models) return fail(c, BF_ERR_ARG, "bf_hold_groups: models %p", (const void*)models);
    int rc = held_grouping_check(c, "bf_hold_groups", n_models, "");
    if (rc != BF_OK) return rc;
    const int K = n_models;
    HIP_TRY(c, hipSetDevice(c->device));
    gs->held.mode = 0;   // (a failure below leaves no held flow)
    if (gs->n > 0) {
        GlobalHeld h;
        if ((rc = ensure_held(c, gs, true, h)) != BF_OK) return rc;
        AssignArgs a{};   // (the events as stored, the staged warps and the held grouping: only the pointers are read)
        if ((rc = vote_warps_stage(c, models, K, true, a)) != BF_OK) return rc;
        {
            ProfScope ps(c, 3);
            launch_hold_groups(a.xy, a.t, a.perm, a.prior, a.wp, K, gs->n, h, c->stream);
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the staged warps are the assignment's too: free again from here)
    }
    gs->held.mode = kGlobalHoldGroups;
    return BF_OK;
}

int bf_group_flow_medians(bf_ctx* c, double* u_med, double* v_med, int32_t* counts) {
    if (!c) return BF_ERR_ARG;
    GlobalHeldFlow f;
    int rc = global_held_flow(c, "bf_group_flow_medians", &f);
    if (rc != BF_OK) return rc;
    if (!c->groups_valid) return fail(c, BF_ERR_STATE, "bf_group_flow_medians: no grouping of the uploaded slice is held");
    const int K = c->groups_K;
    if (K > kAssignMaxModels) return fail(c, BF_ERR_CAPACITY, "bf_group_flow_medians: %d groups (at most %d)", K, kAssignMaxModels);
    for (int k = 0; k < K; ++k) {
        if (u_med) u_med[k] = 0.0;
        if (v_med) v_med[k] = 0.0;
        if (counts) counts[k] = 0;
    }
    if (counts) counts[K] = (int32_t)f.n;
    if (f.n == 0 || K == 0) return BF_OK;   // every group empty
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch::Held& hd = c->glob->held;
    // the state: prefix, median, rank, count -- the part read back -- then the digit counts
    const size_t head = median_state_head(K), bytes = median_state_bytes(K);
    HIP_TRY(c, hd.d_med.grow(median_state_bytes(kAssignMaxModels)));
    HIP_TRY(c, hd.h_med.grow(median_state_head(kAssignMaxModels)));
    uint8_t* b = hd.d_med;
    MedianState st;
    st.prefix = reinterpret_cast<unsigned long long*>(b);
    st.median = reinterpret_cast<double*>(st.prefix + 4 * K);
    st.rank = reinterpret_cast<uint32_t*>(st.median + 2 * K);
    st.count = st.rank + 4 * K;
    st.hist = reinterpret_cast<uint32_t*>(b + head);   // (16-byte aligned: the pick reads four counts at a time)
    HIP_TRY(c, hipMemsetAsync(b, 0, bytes, c->stream));
    {
        ProfScope ps(c, 3);
        for (int pass = 0; pass < 8; ++pass) {   // (the picks narrow the ranks on the device: no wait in between)
            if (pass > 0) HIP_TRY(c, hipMemsetAsync(st.hist, 0, (size_t)K * 4 * 256 * sizeof(uint32_t), c->stream));
            launch_median_pass(f.uv, c->d_group_id, f.n, K, pass, st, c->stream);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(hd.h_med, b, head, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint8_t* hb = hd.h_med;
    const double* med = reinterpret_cast<const double*>(hb + (size_t)K * 4 * 8);
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(hb + (size_t)K * (4 * 8 + 2 * 8 + 4 * 4));
    long long assigned = 0;
    for (int k = 0; k < K; ++k) {
        if (u_med) u_med[k] = med[2 * k];
        if (v_med) v_med[k] = med[2 * k + 1];
        if (counts) counts[k] = (int32_t)cnt[2 * k];
        assigned += (long long)cnt[2 * k];
    }
    if (counts) counts[K] = (int32_t)(f.n - assigned);
    return BF_OK;
}

int bf_global_get_flow(bf_ctx* c, double* nx, double* ny, double* u, double* v, double* pr_x, double* pr_y) {
    if (!c) return BF_ERR_ARG;
    GlobalHeldFlow f;
    int rc = global_held_flow(c, "bf_global_get_flow", &f);
    if (rc != BF_OK) return rc;
    const size_t n = (size_t)f.n;
    if (n == 0) return BF_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch::Held& hd = c->glob->held;
    // up to three arrays of n pairs through pinned memory, every copy followed by an event of its own: the host takes an
    // array apart as soon as ITS copy has landed, while the copies behind it are still on their way
    struct Part { double *a, *b; const double2* d_src; } part[3] = {{nx, ny, f.nxny}, {u, v, f.uv}, {pr_x, pr_y, nullptr}};
    if (pr_x || pr_y) {
        HIP_TRY(c, hd.d_pr.grow(n));
        launch_expand_pr(f.xy, f.p, f.idx, hd.d_pr, f.n, c->stream);
        HIP_TRY(c, hipGetLastError());
        part[2].d_src = hd.d_pr;
    }
    HIP_TRY(c, hd.h_stage.grow(3 * n));
    for (int i = 0; i < 3; ++i) {
        if (!part[i].a && !part[i].b) continue;
        HIP_TRY(c, hd.landed[i].create(hipEventDisableTiming));
        HIP_TRY(c, hipMemcpyAsync(hd.h_stage + (size_t)i * n, part[i].d_src, n * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(hd.landed[i], c->stream));
    }
    for (int i = 0; i < 3; ++i) {
        if (!part[i].a && !part[i].b) continue;
        HIP_TRY(c, hipEventSynchronize(hd.landed[i]));
        const double2* src = hd.h_stage + (size_t)i * n;
        double *a = part[i].a, *b = part[i].b;
        for (size_t j = 0; j < n; ++j) {
            if (a) a[j] = src[j].x;
            if (b) b[j] = src[j].y;
        }
    }
    return BF_OK;
}

}  // extern "C"

int global_best_state(bf_ctx* c, const bf_global_search_opts* lattice, std::vector<double>& xs, std::vector<double>& ys,
                      GlobalBestState* out) {
    std::memset(out, 0, sizeof(*out));
    int rc = sweep_grid(c, lattice, xs, ys, out->nz);
    if (rc != BF_OK) return rc;
    const GlobalSearch* gs = c->glob.get();
    out->n = gs->n;
    if (gs->n <= 0) return BF_OK;
    const GlobalEventState st = gs->state();
    out->max_score = st.max_score; out->best_nx = st.best_nx; out->best_ny = st.best_ny;
    return BF_OK;
}

void global_cand_uv(double nx, double ny, double nz, double* u, double* v) { cand_uv(nx, ny, nz, u, v); }

int global_held_flow(bf_ctx* c, const char* who, GlobalHeldFlow* out) {
    GlobalSearch* gs = c->glob.get();
    if (!gs || !gs->have || !gs->held.mode)
        return fail(c, BF_ERR_STATE, "%s: no held flow: call bf_global_hold_field, bf_global_hold_best or bf_hold_groups first", who);
    if (!c->uploaded || !c->glob_valid || c->n != gs->n)
        return fail(c, BF_ERR_STATE, "%s: events were uploaded since the flow was held", who);
    const GlobalSearch::Held& hd = gs->held;
    std::memset(out, 0, sizeof(*out));
    out->n = gs->n;
    if (gs->n <= 0) return BF_OK;
    const bool best = global_hold_own_order(hd.mode);
    out->xy = best ? hd.d_xy.get() : gs->cells.d_cxy.get();
    out->idx = best ? hd.d_idx.get() : gs->cells.d_cidx.get();
    out->p = hd.d_p;
    out->nxny = hd.d_nxny;
    out->uv = hd.d_uv;
    return BF_OK;
}
