// bf_propose_abi.cpp -- C-ABI of the proposal step (include/bf_accel.h, "event groups: candidate models"; kernels in
// bf_propose.hip): bf_propose_models turns the modes of the per-event best flow the exhaustive search left behind into candidate
// models for bf_assign_groups.
#include "bf_ctx.h"

extern "C" {

int bf_propose_models(bf_ctx* c, const bf_global_search_opts* lattice, const bf_propose_opts* opts, bf_model* models_out,
                      bf_proposal* proposals_out, int32_t cap, uint32_t* hist_out, uint32_t* box_out, int64_t planes_cap,
                      bf_propose_info* info) {
    if (!c) return BF_ERR_ARG;
    bf_propose_opts o;
    memset(&o, 0, sizeof(o));
    o.radius = 1; o.suppress = 2; o.max_models = 8; o.min_votes = 1;
    if (opts) o = *opts;
    if (o.radius < 0 || o.radius > kProposeMaxRadius)
        return fail(c, BF_ERR_ARG, "bf_propose_models: radius %d (0 .. %d)", o.radius, kProposeMaxRadius);
    if (o.suppress < 0 || o.suppress > kProposeMaxSuppress)
        return fail(c, BF_ERR_ARG, "bf_propose_models: suppress %d (0 .. %d)", o.suppress, kProposeMaxSuppress);
    if (o.max_models < 1 || o.max_models > kProposeMaxModels)
        return fail(c, BF_ERR_ARG, "bf_propose_models: max_models %d (1 .. %d)", o.max_models, kProposeMaxModels);
    if (o.min_votes < 1) return fail(c, BF_ERR_ARG, "bf_propose_models: min_votes %d (>= 1)", o.min_votes);
    std::vector<double> xs, ys;
    GlobalBestState st;
    int rc = global_best_state(c, lattice, xs, ys, &st);
    if (rc != BF_OK) return rc;
    const long long nxc = (long long)xs.size(), nyc = (long long)ys.size(), bins = nxc * nyc;
    if (bins > kProposeMaxBins) return fail(c, BF_ERR_CAPACITY, "bf_propose_models: a lattice of %lld x %lld exceeds 2^22 points", nxc, nyc);
    if ((models_out || proposals_out) && cap < o.max_models)
        return fail(c, BF_ERR_ARG, "bf_propose_models: the outputs hold %d of max_models %d", cap, o.max_models);
    if ((hist_out || box_out) && planes_cap < bins)
        return fail(c, BF_ERR_ARG, "bf_propose_models: a plane holds %lld of %lld words", (long long)planes_cap, bins);
    if (models_out && st.nz != 127.0)
        return fail(c, BF_ERR_ARG, "bf_propose_models: models are defined for nz 127 (got %g)", st.nz);

    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_x = nxc; info->n_y = nyc;
    }
    c->propose_form = 0;
    if (st.n == 0) {   // nothing is launched: H and B are zero, no proposal
        if (hist_out) memset(hist_out, 0, (size_t)bins * sizeof(uint32_t));
        if (box_out) memset(box_out, 0, (size_t)bins * sizeof(uint32_t));
        return BF_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int K = o.max_models, nout = propose_out_words(K);
    HIP_TRY(c, c->d_propose_tab.grow((size_t)(nxc + nyc)));
    HIP_TRY(c, c->d_propose_hist.grow((size_t)bins));
    HIP_TRY(c, c->d_propose_box.grow((size_t)bins));
    HIP_TRY(c, c->d_propose_out.grow((size_t)propose_out_words(kProposeMaxModels)));
    HIP_TRY(c, c->h_propose_out.grow((size_t)propose_out_words(kProposeMaxModels)));
    // (xs and ys are read until the stream has been waited for, below)
    HIP_TRY(c, hipMemcpyAsync(c->d_propose_tab, xs.data(), (size_t)nxc * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_propose_tab + nxc, ys.data(), (size_t)nyc * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->d_propose_hist, 0, (size_t)bins * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemsetAsync(c->d_propose_out, 0, (size_t)nout * sizeof(uint32_t), s));
    ProposeArgs a;
    a.max_score = st.max_score; a.best_nx = st.best_nx; a.best_ny = st.best_ny;
    a.tab = c->d_propose_tab;
    a.n = st.n;
    a.n_x = (int)nxc; a.n_y = (int)nyc;
    {
        ProfScope ps(c, 3);
        c->propose_form = launch_propose_vote(a, c->d_propose_hist, c->d_propose_out, s);
        launch_propose_box(c->d_propose_hist, c->d_propose_box, a.n_x, a.n_y, o.radius, s);
        launch_propose_pick(c->d_propose_hist, c->d_propose_box, a.n_x, a.n_y, o.suppress, K, o.min_votes, c->d_propose_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_propose_out, c->d_propose_out, (size_t)nout * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (hist_out) HIP_TRY(c, hipMemcpyAsync(hist_out, c->d_propose_hist, (size_t)bins * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (box_out) HIP_TRY(c, hipMemcpyAsync(box_out, c->d_propose_box, (size_t)bins * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* r = c->h_propose_out;
    const int P = (int)r[3];
    if (P < 0 || P > K) return fail(c, BF_ERR_HIP, "bf_propose_models: the device reported %d proposals of at most %d", P, K);
    for (int p = 0; p < P; ++p) {
        const long long idx = (long long)r[kProposeOutHead + 3 * p];
        const double nx = xs[(size_t)(idx / nyc)], ny = ys[(size_t)(idx % nyc)];
        if (proposals_out) {
            bf_proposal& q = proposals_out[p];
            memset(&q, 0, sizeof(q));
            q.nx = nx; q.ny = ny;
            global_cand_uv(nx, ny, st.nz, &q.u, &q.v);
            q.index = idx;
            q.votes = (int32_t)r[kProposeOutHead + 3 * p + 1];
            q.peak = (int32_t)r[kProposeOutHead + 3 * p + 2];
        }
        if (models_out) {   // the model whose set_model warp compensates the flow (optimizer_rolling.h:289-299)
            bf_model& m = models_out[p];
            memset(&m, 0, sizeof(m));
            m.total_dx = -nx;
            m.total_dy = -ny;
        }
    }
    if (info) {
        info->voted = (int32_t)r[0];
        info->unscored = (int32_t)r[1];
        info->off_lattice = (int32_t)r[2];
        info->proposals = P;
    }
    return BF_OK;
}

}  // extern "C"
