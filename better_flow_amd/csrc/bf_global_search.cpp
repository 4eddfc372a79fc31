// bf_global_search.cpp -- C-ABI of the exhaustive search, OptimizerGlobal (optimizer_global.h / optimizer_global.cpp): the window
// (update_fields), one project_all, compute_flow_bruteforce over a candidate grid, and the per-event state.  The kernels
// are in bf_global.hip; the two definitions this build adds (the per-event best candidate, the objective S) are stated in
// include/bf_accel.h and DESIGN.md.
#include "bf_ctx.h"

struct GlobalSearch {
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

    GlobalEventState state() const {
        GlobalEventState s;
        const long long k = (long long)(d_state.size() / 6);
        s.max_score = d_state; s.best_nx = d_state + k; s.best_ny = d_state + 2 * k; s.best_nz = d_state + 3 * k;
        s.best_pr_x = d_state + 4 * k; s.best_pr_y = d_state + 5 * k;
        return s;
    }
};

void GlobalSearchFree::operator()(GlobalSearch* g) const { delete g; }

extern "C" {

namespace {

constexpr long long kGlobalBatchBytes = 512ll << 20;   // point + window planes of one batch
constexpr int kGlobalMaxBatch = 32;
constexpr long long kGlobalMaxCandidates = 1ll << 26;

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

// candidates [k0, k0 + k) of gs->h_cands, already on the device at d_cands + k0: S into d_S + k0, folded into the state
int run_candidates(bf_ctx* c, GlobalSearch* gs, long long k0, long long k, uint8_t* d_img, float* d_scores) {
    if (gs->n <= 0) return BF_OK;   // no event: every S stays 0
    const int B = (int)std::max(1ll, std::min((long long)kGlobalMaxBatch, kGlobalBatchBytes / (gs->g.plane * 8)));
    int rc = ensure_batch(c, gs, (int)std::min((long long)B, k));
    if (rc != BF_OK) return rc;
    const bf_ctx::EvSet& e = c->set[c->cs];
    const uint32_t* perm = c->has_perm ? e.perm : nullptr;
    for (long long b0 = 0; b0 < k; b0 += B) {
        const int nb = (int)std::min((long long)B, k - b0);
        HIP_TRY(c, hipMemsetAsync(gs->d_pts, 0, (size_t)nb * (size_t)gs->g.plane * sizeof(uint32_t), c->stream));
        const int lr = launch_global_batch(e.xy, e.t, perm, gs->n, gs->g, gs->d_cands + k0 + b0, nb, gs->d_pts, gs->d_win,
                                           d_img, gs->state(), gs->d_S + k0 + b0, d_scores, c->stream);
        if (lr == -1) return fail(c, BF_ERR_ARG, "the 8-bit Gaussian is defined for scale <= 7");
        if (lr == -3) return fail(c, BF_ERR_ARG, "metric_wsize %d: the tile does not fit the LDS", gs->w.metric_wsize);
        if (lr != 0) return fail(c, BF_ERR_HIP, "bf_global: kernel attributes");
        HIP_TRY(c, hipGetLastError());
    }
    return BF_OK;
}

}  // namespace

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
    c->glob_valid = false;
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
    c->glob_valid = true;
    if (out) *out = w;
    return BF_OK;
}

int bf_global_project_all(bf_ctx* c, double nx, double ny, double nz, uint8_t* img_out, float* scores_out, int64_t* sum_out) {
    if (!c) return BF_ERR_ARG;
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    const bf_global_window& w = gs->w;
    const size_t img_px = (size_t)w.scale_bordered_img_x * (size_t)w.scale_bordered_img_y;
    const size_t sc_px = (size_t)w.scale_img_x * (size_t)w.scale_img_y;
    if ((rc = ensure_cands(c, gs, 1)) != BF_OK) return rc;
    if (img_out) HIP_TRY(c, gs->d_img.grow(img_px));
    if (scores_out) HIP_TRY(c, gs->d_scores.grow(sc_px));
    gs->h_cands.assign(1, make_cand(nx, ny, nz));
    HIP_TRY(c, hipMemcpyAsync(gs->d_cands, gs->h_cands.data(), sizeof(GlobalCand), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->d_S, 0, sizeof(unsigned long long), c->stream));
    if (img_out && img_px) HIP_TRY(c, hipMemsetAsync(gs->d_img, 0, img_px, c->stream));
    if (scores_out && sc_px) HIP_TRY(c, hipMemsetAsync(gs->d_scores, 0, sc_px * sizeof(float), c->stream));
    if ((rc = run_candidates(c, gs, 0, 1, img_out ? gs->d_img.get() : nullptr, scores_out ? gs->d_scores.get() : nullptr)) != BF_OK)
        return rc;
    unsigned long long S = 0;
    HIP_TRY(c, hipMemcpyAsync(&S, gs->d_S, sizeof(S), hipMemcpyDeviceToHost, c->stream));
    if (img_out && img_px) HIP_TRY(c, hipMemcpyAsync(img_out, gs->d_img, img_px, hipMemcpyDeviceToHost, c->stream));
    if (scores_out && sc_px)
        HIP_TRY(c, hipMemcpyAsync(scores_out, gs->d_scores, sc_px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (sum_out) *sum_out = (int64_t)S;
    return BF_OK;
}

int bf_global_search(bf_ctx* c, const bf_global_search_opts* opts, bf_global_result* out, int64_t* surface_out,
                     int64_t surface_cap) {
    if (!c) return BF_ERR_ARG;
    bf_global_search_opts o;
    bf_global_search_opts_default(&o);
    if (opts) o = *opts;
    if (!(o.x_step > 0) || !(o.y_step > 0) || !(o.x_low < o.x_hi) || !(o.y_low < o.y_hi))   // optimizer_global.cpp:110
        return fail(c, BF_ERR_ARG, "bad search range: need lo < hi and step > 0");
    if (!(o.nz > 0) || !std::isfinite(o.x_hi) || !std::isfinite(o.y_hi)) return fail(c, BF_ERR_ARG, "bad nz / range");
    int rc = global_ready(c);
    if (rc != BF_OK) return rc;
    // the reference's loops (:134-135): repeated double addition, ny restarting from y_low on every row
    std::vector<double> xs, ys;
    for (double v = o.x_low; v < o.x_hi; v += o.x_step) {
        xs.push_back(v);
        if ((long long)xs.size() > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "more than 2^26 candidates");
    }
    for (double v = o.y_low; v < o.y_hi; v += o.y_step) {
        ys.push_back(v);
        if ((long long)ys.size() > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "more than 2^26 candidates");
    }
    const long long nxc = (long long)xs.size(), nyc = (long long)ys.size(), k = nxc * nyc;
    if (k > kGlobalMaxCandidates) return fail(c, BF_ERR_ARG, "%lld candidates (more than 2^26)", k);
    if (surface_out && surface_cap < k) return fail(c, BF_ERR_ARG, "surface buffer holds %lld of %lld", (long long)surface_cap, k);
    HIP_TRY(c, hipSetDevice(c->device));
    GlobalSearch* gs = c->glob.get();
    gs->h_cands.resize((size_t)k);
    for (long long i = 0; i < nxc; ++i)
        for (long long j = 0; j < nyc; ++j) gs->h_cands[(size_t)(i * nyc + j)] = make_cand(xs[i], ys[j], o.nz);
    if ((rc = ensure_cands(c, gs, k)) != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(gs->d_cands, gs->h_cands.data(), (size_t)k * sizeof(GlobalCand), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(gs->d_S, 0, (size_t)k * sizeof(unsigned long long), c->stream));
    if ((rc = run_candidates(c, gs, 0, k, nullptr, nullptr)) != BF_OK) return rc;
    std::vector<unsigned long long> S((size_t)k);
    HIP_TRY(c, hipMemcpyAsync(S.data(), gs->d_S, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    long long best = 0;
    for (long long i = 1; i < k; ++i)
        if (S[(size_t)i] > S[(size_t)best]) best = i;   // the first of the largest
    if (surface_out)
        for (long long i = 0; i < k; ++i) surface_out[i] = (int64_t)S[(size_t)i];
    if (out) {
        out->best_nx = xs[(size_t)(best / nyc)];
        out->best_ny = ys[(size_t)(best % nyc)];
        out->best_sum = (int64_t)S[(size_t)best];
        out->n_x = nxc;
        out->n_y = nyc;
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
        // Event::compute_uv, event.h:135-142
        const double xy_len = std::hypot(nx[i], ny[i]);
        const double speed = xy_len / (nz[i] / (1000000000 / (1 * 10000)));
        if (best_u) best_u[i] = xy_len == 0 ? 0 : speed * nx[i] / xy_len;
        if (best_v) best_v[i] = xy_len == 0 ? 0 : speed * ny[i] / xy_len;
    }
    return BF_OK;
}

}  // extern "C"
