// bf_assign_abi.cpp -- C-ABI of the entries that work on the K models' vote planes (include/bf_accel.h, "event groups:
// assignment", "event groups: projection" and "event groups: merge gains"; kernels in bf_assign.hip, bf_project.hip and
// bf_merge.hip):
//   bf_assign_groups   gives every event of the uploaded slice to one of K candidate models, and may install the result as the
//                      context's grouping for bf_run_groups;
//   bf_project_groups  renders the slice with every event warped by its own group's model -- per pixel the event count, the
//                      owning group and its colour -- and scores it: per group and overall the integer moments of that image.
//   bf_merge_scores    says, for every ordered pair (b, a) of groups, how much of the contrast sum N^2 the events of group b
//                      add under model a: the projection's planes once, then the trial planes of A target models per pass.
// What they share is here once: the option checks, the window of the widened sensor and its capacity check (vote_planes_check),
// and the planes, the staged warps and the kernels' AssignArgs (vote_planes_stage).  Between the two each entry zeroes its own
// outputs and applies its own rule for a slice without events.
// (bf_track_keep, bf_track_abi.cpp, drives the projection's kernels through the same three helpers: declared in bf_ctx.h.)
#include "bf_ctx.h"

// The checks both entries make after those of their own pointers, in their order; `who`: the entry point's name; `knob`: the
// entry's own option, which must be >= 1, and its name; `prior`: null when the held grouping is not read, else what the message
// says before "no grouping ... is held".  Then the window and the capacity check.  Fills everything of vp but a's pointers.
// vote_planes_window: the window alone, of options that have passed these checks (bf_track_overlap: the kept plane's).
int vote_planes_check(bf_ctx* c, const char* who, int scale, int res_x, int res_y, int margin, const char* knob_name, int knob,
                      int n_models, const char* prior, VotePlanes& vp) {
    if (scale < 1 || scale % 2 == 0 || scale / 2 > kMaxHalfScale)
        return fail(c, BF_ERR_ARG, "scale must be odd and <= %d (got %d)", 2 * kMaxHalfScale + 1, scale);
    if (res_x < 1 || res_y < 1 || res_x > 65536 || res_y > 65536) return fail(c, BF_ERR_ARG, "bad sensor size");
    if (margin < 0 || margin > 65536 || knob < 1)
        return fail(c, BF_ERR_ARG, "%s: margin %d (0 .. 65536), %s %d (>= 1)", who, margin, knob_name, knob);
    if (n_models < 1 || n_models > kAssignMaxModels) return fail(c, BF_ERR_ARG, "%s: %d models (1 .. %d)", who, n_models, kAssignMaxModels);
    if (c->has_noise) return fail(c, BF_ERR_ARG, "%s does not take a noise mask", who);
    const int K = n_models;
    if (prior) {
        if (!c->groups_valid) return fail(c, BF_ERR_STATE, "%s: %sno grouping of the uploaded slice is held", who, prior);
        if (c->groups_K != K) return fail(c, BF_ERR_ARG, "%s: the held grouping has %d groups, %d models given", who, c->groups_K, K);
    }
    vote_planes_window(c, scale, res_x, res_y, margin, K, vp);
    if ((long long)K * (long long)vp.plane > kAssignMaxWords)
        return fail(c, BF_ERR_CAPACITY, "%s: %d planes of %d x %d exceed 2^27 words", who, K, vp.R, vp.C);
    return BF_OK;
}

void vote_planes_window(const bf_ctx* c, int scale, int res_x, int res_y, int margin, int K, VotePlanes& vp) {
    // the window of the whole sensor widened by the margin (optimizer_rolling.h:248-283): the same for every call on a sensor
    const bf_window w = window_of_box(scale, -margin, res_x - 1 + margin, -margin, res_y - 1 + margin);
    vp.R = w.scale_img_x;
    vp.C = w.scale_img_y;
    vp.plane = (size_t)vp.R * (size_t)vp.C;
    AssignArgs& a = vp.a;
    a.xy = nullptr; a.t = nullptr; a.perm = nullptr; a.wp = nullptr;
    a.prior = nullptr;
    a.n = c->n;
    a.K = K; a.scale = scale;
    a.x_sh = (int)w.x_shift;   // double -> int parameter conversion of accel_lib.h:147
    a.y_sh = (int)w.y_shift;
    a.wsx = w.metric_wsizex; a.wsy = w.metric_wsizey;
    a.R = vp.R; a.C = vp.C;
}

// (n > 0, the device set) The vote planes grown and V cleared, the box planes grown when they are used, the K warps staged, and
// a's pointers; `prior`: the held grouping is the kernels' prior.
int vote_planes_stage(bf_ctx* c, const bf_model* models, bool prior, VotePlanes& vp) {
    AssignArgs& a = vp.a;
    const size_t words = (size_t)a.K * vp.plane;
    HIP_TRY(c, c->d_assign_votes.grow(words));
    if (a.scale > 1) HIP_TRY(c, c->d_assign_box.grow(words));
    HIP_TRY(c, c->d_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->h_assign_wp.grow((size_t)kAssignMaxModels));
    for (int k = 0; k < a.K; ++k) set_model_warp(c->h_assign_wp[k], models[k]);   // (sine and cosine from the host's libm)
    HIP_TRY(c, hipMemcpyAsync(c->d_assign_wp, c->h_assign_wp, (size_t)a.K * sizeof(WarpParams), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_assign_votes, 0, words * sizeof(uint32_t), c->stream));
    const bf_ctx::EvSet& e = c->set[c->cs];
    a.xy = e.xy; a.t = e.t;
    a.perm = c->has_perm ? e.perm.get() : nullptr;
    a.wp = c->d_assign_wp;
    a.prior = prior ? c->d_group_id.get() : nullptr;
    return BF_OK;
}

// The planes the second kernel of either entry reads: the box sums, or V itself at scale 1.
const uint32_t* vote_planes_summed(bf_ctx* c, const VotePlanes& vp) {
    return vp.a.scale > 1 ? c->d_assign_box.get() : c->d_assign_votes.get();
}

extern "C" {

int bf_assign_groups(bf_ctx* c, const bf_assign_opts* o, const bf_model* models, int32_t n_models, int32_t* group_id_out,
                     int32_t* score_out, int32_t* counts_out, bf_assign_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_assign_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_assign_groups: opts %p, models %p", (const void*)o, (const void*)models);
    VotePlanes vp;
    int rc = vote_planes_check(c, "bf_assign_groups", o->scale, o->sensor_res_x, o->sensor_res_y, o->margin, "min_score",
                               o->min_score, n_models, o->use_prior ? "use_prior, but " : nullptr, vp);
    if (rc != BF_OK) return rc;
    const AssignArgs& a = vp.a;
    const int K = a.K;

    if (counts_out) memset(counts_out, 0, ((size_t)K + 1) * sizeof(int32_t));
    if (info) memset(info, 0, sizeof(*info));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->n == 0) {   // every output zero; an installed result is the empty grouping
        return o->install ? install_grouping(c, nullptr, hipMemcpyDeviceToDevice, K) : BF_OK;
    }

    const int nout = assign_out_words(K);
    rc = vote_planes_stage(c, models, o->use_prior != 0, vp);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, c->d_assign_gid.grow((size_t)c->n));
    HIP_TRY(c, c->d_assign_score.grow((size_t)c->n));
    HIP_TRY(c, c->d_assign_out.grow((size_t)assign_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_assign_out.grow((size_t)assign_out_words(kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(c->d_assign_out, 0, (size_t)nout * sizeof(uint32_t), s));
    {
        ProfScope ps(c, 3);
        launch_assign_vote(a, c->d_assign_votes, s);
        if (a.scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, vp.R, vp.C, a.scale, s);
        launch_assign_pick(a, vote_planes_summed(c, vp), o->min_score, c->d_assign_gid, c->d_assign_score, c->d_assign_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_assign_out, c->d_assign_out, (size_t)nout * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (group_id_out)
        HIP_TRY(c, hipMemcpyAsync(group_id_out, c->d_assign_gid, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (score_out)
        HIP_TRY(c, hipMemcpyAsync(score_out, c->d_assign_score, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (o->install && (rc = install_grouping(c, c->d_assign_gid, hipMemcpyDeviceToDevice, K)) != BF_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* r = c->h_assign_out;
    if (counts_out)
        for (int k = 0; k <= K; ++k) counts_out[k] = (int32_t)r[k];
    if (info) {
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = (int32_t)r[K];
        info->assigned = (int32_t)(c->n - (long long)r[K]);
        info->changed = (int32_t)r[K + 1];
        info->max_score = (int32_t)r[K + 2];
    }
    return BF_OK;
}

int bf_project_groups(bf_ctx* c, const bf_project_opts* o, const bf_model* models, int32_t n_models, uint32_t* count_out,
                      int32_t* label_out, uint8_t* bgr_out, bf_group_score* scores_out, bf_project_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_project_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_project_groups: opts %p, models %p", (const void*)o, (const void*)models);
    VotePlanes vp;
    int rc = vote_planes_check(c, "bf_project_groups", o->scale, o->sensor_res_x, o->sensor_res_y, o->margin, "gain", o->gain,
                               n_models, "", vp);   // (the held grouping is required: here an event's ONE model)
    if (rc != BF_OK) return rc;
    const AssignArgs& a = vp.a;
    const int K = a.K;
    const size_t plane = vp.plane;

    if (scores_out) memset(scores_out, 0, (size_t)K * sizeof(bf_group_score));
    if (info) memset(info, 0, sizeof(*info));
    if (c->n == 0) {   // N == 0 everywhere
        if (count_out) memset(count_out, 0, plane * sizeof(uint32_t));
        if (label_out) memset(label_out, 0xff, plane * sizeof(int32_t));
        if (bgr_out) memset(bgr_out, 0, 3 * plane);
        return BF_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;

    const int nout = project_out_words(K);
    rc = vote_planes_stage(c, models, true, vp);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, c->d_project_count.grow(plane));
    HIP_TRY(c, c->d_project_label.grow(plane));
    HIP_TRY(c, c->d_project_bgr.grow(3 * plane));
    HIP_TRY(c, c->d_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(c->d_project_out, 0, (size_t)nout * sizeof(unsigned long long), s));
    {
        ProfScope ps(c, 3);
        launch_project_vote(a, c->d_assign_votes, c->d_project_out, s);
        if (a.scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, vp.R, vp.C, a.scale, s);
        launch_project_compose(vote_planes_summed(c, vp), K, vp.R, vp.C, o->gain, c->d_project_count, c->d_project_label,
                               c->d_project_bgr, c->d_project_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_project_out, c->d_project_out, (size_t)nout * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (count_out) HIP_TRY(c, hipMemcpyAsync(count_out, c->d_project_count, plane * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (label_out) HIP_TRY(c, hipMemcpyAsync(label_out, c->d_project_label, plane * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (bgr_out) HIP_TRY(c, hipMemcpyAsync(bgr_out, c->d_project_bgr, 3 * plane, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const unsigned long long* h = c->h_project_out;
    auto r = [h](int word) { return h[(size_t)word * kProjectStride]; };
    long long outside = 0;
    for (int k = 0; k < K; ++k) {
        outside += (long long)r(k) - (long long)r(K + k);
        if (!scores_out) continue;
        bf_group_score& g = scores_out[k];
        g.events = (int32_t)r(k);
        g.inside = (int32_t)r(K + k);
        g.pixels_hit = (int32_t)r(2 * K + k);
        g.pixels_owned = (int32_t)r(3 * K + k);
        g.max = (int32_t)r(4 * K + k);
        g.sum_sq = r(5 * K + k);
    }
    if (info) {
        const int t = kProjectTables * K;
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = (int32_t)r(t);
        info->outside = (int32_t)outside;
        info->pixels = (int32_t)r(t + 1);
        info->sum = r(t + 2);
        info->sum_sq = r(t + 3);
    }
    return BF_OK;
}

int bf_merge_scores(bf_ctx* c, const bf_merge_opts* o, const bf_model* models, int32_t n_models, uint64_t* gain_out,
                    int32_t* inside_out, int32_t* events_out, bf_merge_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_merge_scores before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_merge_scores: opts %p, models %p", (const void*)o, (const void*)models);
    if (o->targets_per_pass < 0) return fail(c, BF_ERR_ARG, "bf_merge_scores: targets_per_pass %d (>= 0)", o->targets_per_pass);
    VotePlanes vp;
    int rc = vote_planes_check(c, "bf_merge_scores", o->scale, o->sensor_res_x, o->sensor_res_y, o->margin, "targets_per_pass + 1",
                               o->targets_per_pass + 1, n_models, "", vp);   // (the held grouping is required, as for the projection)
    if (rc != BF_OK) return rc;
    const AssignArgs& a = vp.a;
    const int K = a.K;
    const size_t plane = vp.plane;
    const size_t pairs = (size_t)K * (size_t)K;

    if (gain_out) memset(gain_out, 0, pairs * sizeof(uint64_t));
    if (inside_out) memset(inside_out, 0, pairs * sizeof(int32_t));
    if (events_out) memset(events_out, 0, (size_t)K * sizeof(int32_t));
    if (info) memset(info, 0, sizeof(*info));
    if (c->n == 0) return BF_OK;   // everything zero
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;

    const int A = merge_targets_per_pass(K, (long long)plane, o->targets_per_pass);
    const int passes = (K + A - 1) / A;
    const size_t trial = (size_t)A * (size_t)K * plane;
    const int nbase = project_out_words(K), nout = merge_out_words(K);
    rc = vote_planes_stage(c, models, true, vp);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, c->d_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->d_merge_n.grow(plane));
    HIP_TRY(c, c->d_merge_votes.grow(trial));
    if (a.scale > 1) HIP_TRY(c, c->d_merge_box.grow(trial));
    HIP_TRY(c, c->d_merge_out.grow((size_t)merge_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_merge_out.grow((size_t)merge_out_words(kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(c->d_project_out, 0, (size_t)nbase * sizeof(unsigned long long), s));
    HIP_TRY(c, hipMemsetAsync(c->d_merge_out, 0, (size_t)nout * sizeof(unsigned long long), s));
    {
        ProfScope ps(c, 3);
        // the base planes: every group under its own model, exactly the projection's
        launch_project_vote(a, c->d_assign_votes, c->d_project_out, s);
        if (a.scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, vp.R, vp.C, a.scale, s);
        const uint32_t* B = vote_planes_summed(c, vp);
        launch_merge_total(B, K, vp.R, vp.C, c->d_merge_n, c->d_merge_out, s);
        for (int a0 = 0; a0 < K; a0 += A) {   // (the passes follow each other on the stream: they share the trial planes)
            const int targets = K - a0 < A ? K - a0 : A;
            const size_t words = (size_t)targets * (size_t)K * plane;
            HIP_TRY(c, hipMemsetAsync(c->d_merge_votes, 0, words * sizeof(uint32_t), s));
            launch_merge_vote(a, a0, targets, c->d_merge_votes, c->d_merge_out, s);
            if (a.scale > 1) launch_assign_box(c->d_merge_votes, c->d_merge_box, targets * K, vp.R, vp.C, a.scale, s);
            launch_merge_gain(a.scale > 1 ? c->d_merge_box.get() : c->d_merge_votes.get(), B, c->d_merge_n, K, a0, targets, vp.R,
                              vp.C, c->d_merge_out, s);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_project_out, c->d_project_out, (size_t)nbase * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(c->h_merge_out, c->d_merge_out, (size_t)nout * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const unsigned long long* hb = c->h_project_out;
    const unsigned long long* hm = c->h_merge_out;
    auto r = [hm](size_t word) { return hm[word * kProjectStride]; };
    for (size_t w = 0; w < pairs; ++w) {
        if (gain_out) gain_out[w] = r(w);
        if (inside_out) inside_out[w] = (int32_t)r(pairs + w);
    }
    if (inside_out)   // the diagonal is the base pass's: events of k inside under their own model
        for (int k = 0; k < K; ++k) inside_out[(size_t)k * K + k] = (int32_t)hb[(size_t)(K + k) * kProjectStride];
    if (events_out)
        for (int k = 0; k < K; ++k) events_out[k] = (int32_t)hb[(size_t)k * kProjectStride];
    if (info) {
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = (int32_t)hb[(size_t)(kProjectTables * K) * kProjectStride];
        info->passes = passes;
        info->sum = r(2 * pairs);
        info->sum_sq = r(2 * pairs + 1);
    }
    return BF_OK;
}

}  // extern "C"
