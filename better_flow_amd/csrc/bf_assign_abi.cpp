// bf_assign_abi.cpp -- C-ABI of the entries that work on the K models' vote planes (include/bf_accel.h, "event groups:
// assignment", "event groups: projection" and "event groups: merge gains"; kernels in bf_assign.hip, bf_project.hip and
// bf_merge.hip):
//   bf_assign_groups   gives every event of the uploaded slice to one of K candidate models, and may install the result as the
//                      context's grouping for bf_run_groups;
//   bf_project_groups  renders the slice with every event warped by its own group's model -- per pixel the event count, the
//                      owning group and its colour -- and scores it: per group and overall the integer moments of that image.
//   bf_merge_scores    says, for every ordered pair (b, a) of groups, how much of the contrast sum N^2 the events of group b
//                      add under model a: the projection's planes once, then the trial planes of A target models per pass.
// What they share -- with bf_track_abi.cpp and bf_hold_groups, through bf_vote_planes.h -- is here once: the check that K models
// are given for the held grouping, the window's checks, the window of the widened sensor and its capacity check; the staging of
// the K warps and of the planes; and the projection's base pass with the decode of its shared words, which bf_project_groups,
// bf_merge_scores and bf_track_keep all run.  Around these each entry checks its own option, zeroes its own outputs and applies
// its own rule for a slice without events.  The scratch is bf_ctx::vote; the result blocks' words are bf_group_blocks.h's.
#include "bf_vote_planes.h"

int held_grouping_check(bf_ctx* c, const char* who, int n_models, const char* prior) {
    if (n_models < 1 || n_models > kAssignMaxModels) return fail(c, BF_ERR_ARG, "%s: %d models (1 .. %d)", who, n_models, kAssignMaxModels);
    if (c->has_noise) return fail(c, BF_ERR_ARG, "%s does not take a noise mask", who);
    if (!prior) return BF_OK;
    if (!c->groups_valid) return fail(c, BF_ERR_STATE, "%s: %sno grouping of the uploaded slice is held", who, prior);
    if (c->groups_K != n_models)
        return fail(c, BF_ERR_ARG, "%s: the held grouping has %d groups, %d models given", who, c->groups_K, n_models);
    return BF_OK;
}

int vote_window_check(bf_ctx* c, const VoteWindow& w) {
    if (w.scale < 1 || w.scale % 2 == 0 || w.scale / 2 > kMaxHalfScale)
        return fail(c, BF_ERR_ARG, "scale must be odd and <= %d (got %d)", 2 * kMaxHalfScale + 1, w.scale);
    if (w.res_x < 1 || w.res_y < 1 || w.res_x > 65536 || w.res_y > 65536) return fail(c, BF_ERR_ARG, "bad sensor size");
    return BF_OK;
}

int vote_planes_check(bf_ctx* c, const char* who, const VoteWindow& w, int n_models, const char* prior, VotePlanes& vp) {
    const int rc = held_grouping_check(c, who, n_models, prior);
    if (rc != BF_OK) return rc;
    const int K = n_models;
    vote_planes_window(c, w, K, vp);
    if ((long long)K * (long long)vp.plane > kAssignMaxWords)
        return fail(c, BF_ERR_CAPACITY, "%s: %d planes of %d x %d exceed 2^27 words", who, K, vp.R, vp.C);
    return BF_OK;
}

void vote_planes_window(const bf_ctx* c, const VoteWindow& o, int K, VotePlanes& vp) {
    // the window of the whole sensor widened by the margin (optimizer_rolling.h:248-283): the same for every call on a sensor
    const bf_window w = window_of_box(o.scale, -o.margin, o.res_x - 1 + o.margin, -o.margin, o.res_y - 1 + o.margin);
    vp.R = w.scale_img_x;
    vp.C = w.scale_img_y;
    vp.plane = (size_t)vp.R * (size_t)vp.C;
    AssignArgs& a = vp.a;
    a = AssignArgs{};   // (the pointers: null until the staging)
    a.n = c->n;
    a.K = K; a.scale = o.scale;
    a.x_sh = (int)w.x_shift;   // double -> int parameter conversion of accel_lib.h:147
    a.y_sh = (int)w.y_shift;
    a.wsx = w.metric_wsizex; a.wsy = w.metric_wsizey;
    a.R = vp.R; a.C = vp.C;
}

int vote_warps_stage(bf_ctx* c, const bf_model* models, int K, bool prior, AssignArgs& a) {
    bf_ctx::VoteScratch::Shared& sh = c->vote.shared;
    HIP_TRY(c, sh.d_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, sh.h_wp.grow((size_t)kAssignMaxModels));
    for (int k = 0; k < K; ++k) set_model_warp(sh.h_wp[k], models[k]);   // (sine and cosine from the host's libm)
    HIP_TRY(c, hipMemcpyAsync(sh.d_wp, sh.h_wp, (size_t)K * sizeof(WarpParams), hipMemcpyHostToDevice, c->stream));
    const bf_ctx::EvSet& e = c->set[c->cs];
    a.xy = e.xy; a.t = e.t;
    a.perm = c->has_perm ? e.perm.get() : nullptr;
    a.wp = sh.d_wp;
    a.prior = prior ? c->d_group_id.get() : nullptr;
    return BF_OK;
}

int vote_planes_stage(bf_ctx* c, const bf_model* models, bool prior, VotePlanes& vp) {
    bf_ctx::VoteScratch::Shared& sh = c->vote.shared;
    const size_t words = (size_t)vp.a.K * vp.plane;
    HIP_TRY(c, sh.votes.grow(words));
    if (vp.a.scale > 1) HIP_TRY(c, sh.box.grow(words));
    const int rc = vote_warps_stage(c, models, vp.a.K, prior, vp.a);   // (the small copy ahead of the long clear, as it always was)
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(sh.votes, 0, words * sizeof(uint32_t), c->stream));
    return BF_OK;
}

const uint32_t* vote_planes_summed(bf_ctx* c, const VotePlanes& vp) {
    return vp.a.scale > 1 ? c->vote.shared.box.get() : c->vote.shared.votes.get();
}

int project_base_pass(bf_ctx* c, const bf_model* models, VotePlanes& vp, int gain, int32_t* label) {
    bf_ctx::VoteScratch::Project& pr = c->vote.project;
    const AssignArgs& a = vp.a;
    hipStream_t s = c->stream;
    const int rc = vote_planes_stage(c, models, true, vp);
    if (rc != BF_OK) return rc;
    if (label) {
        HIP_TRY(c, pr.count.grow(vp.plane));
        HIP_TRY(c, pr.bgr.grow(3 * vp.plane));
    }
    HIP_TRY(c, pr.d_out.grow(ProjectBlock::size(kAssignMaxModels)));
    HIP_TRY(c, pr.h_out.grow(ProjectBlock::size(kAssignMaxModels)));
    const size_t bytes = ProjectBlock::size(a.K) * sizeof(unsigned long long);
    HIP_TRY(c, hipMemsetAsync(pr.d_out, 0, bytes, s));
    {
        ProfScope ps(c, 3);
        launch_project_vote(a, c->vote.shared.votes, pr.d_out, s);
        if (a.scale > 1) launch_assign_box(c->vote.shared.votes, c->vote.shared.box, a.K, vp.R, vp.C, a.scale, s);
        if (label) launch_project_compose(vote_planes_summed(c, vp), a.K, vp.R, vp.C, gain, pr.count, label, pr.bgr, pr.d_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pr.h_out, pr.d_out, bytes, hipMemcpyDeviceToHost, s));
    return BF_OK;
}

ProjectBase project_base_decode(const bf_ctx* c, int K) {
    const unsigned long long* h = c->vote.project.h_out;
    ProjectBase b;
    long long outside = 0;
    for (int k = 0; k < K; ++k) {
        b.events[k] = (int32_t)h[ProjectBlock::events(K, k)];
        b.inside[k] = (int32_t)h[ProjectBlock::inside(K, k)];
        outside += (long long)h[ProjectBlock::events(K, k)] - (long long)h[ProjectBlock::inside(K, k)];
    }
    b.unassigned = (int32_t)h[ProjectBlock::unassigned(K)];
    b.outside = (int32_t)outside;
    return b;
}

extern "C" {

int bf_assign_groups(bf_ctx* c, const bf_assign_opts* o, const bf_model* models, int32_t n_models, int32_t* group_id_out,
                     int32_t* score_out, int32_t* counts_out, bf_assign_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_assign_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_assign_groups: opts %p, models %p", (const void*)o, (const void*)models);
    const VoteWindow w{o->scale, o->sensor_res_x, o->sensor_res_y, o->margin};
    VotePlanes vp;
    int rc = vote_window_check(c, w);
    if (rc == BF_OK && (!vote_margin_ok(o->margin) || o->min_score < 1))
        rc = fail(c, BF_ERR_ARG, "bf_assign_groups: margin %d (0 .. 65536), min_score %d (>= 1)", o->margin, o->min_score);
    if (rc == BF_OK) rc = vote_planes_check(c, "bf_assign_groups", w, n_models, o->use_prior ? "use_prior, but " : nullptr, vp);
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

    bf_ctx::VoteScratch::Shared& sh = c->vote.shared;
    bf_ctx::VoteScratch::Assign& as = c->vote.assign;
    const size_t bytes = (size_t)AssignBlock::size(K) * sizeof(uint32_t);
    rc = vote_planes_stage(c, models, o->use_prior != 0, vp);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, as.gid.grow((size_t)c->n));
    HIP_TRY(c, as.score.grow((size_t)c->n));
    HIP_TRY(c, as.d_out.grow((size_t)AssignBlock::size(kAssignMaxModels)));
    HIP_TRY(c, as.h_out.grow((size_t)AssignBlock::size(kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(as.d_out, 0, bytes, s));
    {
        ProfScope ps(c, 3);
        launch_assign_vote(a, sh.votes, s);
        if (a.scale > 1) launch_assign_box(sh.votes, sh.box, K, vp.R, vp.C, a.scale, s);
        launch_assign_pick(a, vote_planes_summed(c, vp), o->min_score, as.gid, as.score, as.d_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(as.h_out, as.d_out, bytes, hipMemcpyDeviceToHost, s));
    if (group_id_out) HIP_TRY(c, hipMemcpyAsync(group_id_out, as.gid, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (score_out) HIP_TRY(c, hipMemcpyAsync(score_out, as.score, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (o->install && (rc = install_grouping(c, as.gid, hipMemcpyDeviceToDevice, K)) != BF_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* r = as.h_out;
    if (counts_out)
        for (int k = 0; k <= K; ++k) counts_out[k] = (int32_t)r[AssignBlock::count(K, k)];
    if (info) {
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = (int32_t)r[AssignBlock::count(K, K)];
        info->assigned = (int32_t)(c->n - (long long)r[AssignBlock::count(K, K)]);
        info->changed = (int32_t)r[AssignBlock::changed(K)];
        info->max_score = (int32_t)r[AssignBlock::max_score(K)];
    }
    return BF_OK;
}

int bf_project_groups(bf_ctx* c, const bf_project_opts* o, const bf_model* models, int32_t n_models, uint32_t* count_out,
                      int32_t* label_out, uint8_t* bgr_out, bf_group_score* scores_out, bf_project_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_project_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_project_groups: opts %p, models %p", (const void*)o, (const void*)models);
    const VoteWindow w{o->scale, o->sensor_res_x, o->sensor_res_y, o->margin};
    VotePlanes vp;
    int rc = vote_window_check(c, w);
    if (rc == BF_OK && (!vote_margin_ok(o->margin) || o->gain < 1))
        rc = fail(c, BF_ERR_ARG, "bf_project_groups: margin %d (0 .. 65536), gain %d (>= 1)", o->margin, o->gain);
    if (rc == BF_OK) rc = vote_planes_check(c, "bf_project_groups", w, n_models, "", vp);   // (the held grouping is required: here an event's ONE model)
    if (rc != BF_OK) return rc;
    const int K = vp.a.K;
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

    bf_ctx::VoteScratch::Project& pr = c->vote.project;
    HIP_TRY(c, pr.label.grow(plane));
    rc = project_base_pass(c, models, vp, o->gain, pr.label);
    if (rc != BF_OK) return rc;
    if (count_out) HIP_TRY(c, hipMemcpyAsync(count_out, pr.count, plane * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (label_out) HIP_TRY(c, hipMemcpyAsync(label_out, pr.label, plane * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (bgr_out) HIP_TRY(c, hipMemcpyAsync(bgr_out, pr.bgr, 3 * plane, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const unsigned long long* h = pr.h_out;
    const ProjectBase base = project_base_decode(c, K);
    for (int k = 0; scores_out && k < K; ++k) {
        bf_group_score& g = scores_out[k];
        g.events = base.events[k];
        g.inside = base.inside[k];
        g.pixels_hit = (int32_t)h[ProjectBlock::pixels_hit(K, k)];
        g.pixels_owned = (int32_t)h[ProjectBlock::pixels_owned(K, k)];
        g.max = (int32_t)h[ProjectBlock::max(K, k)];
        g.sum_sq = h[ProjectBlock::sum_sq(K, k)];
    }
    if (info) {
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = base.unassigned;
        info->outside = base.outside;
        info->pixels = (int32_t)h[ProjectBlock::pixels(K)];
        info->sum = h[ProjectBlock::sum(K)];
        info->sum_sq = h[ProjectBlock::sum_sq_total(K)];
    }
    return BF_OK;
}

int bf_merge_scores(bf_ctx* c, const bf_merge_opts* o, const bf_model* models, int32_t n_models, uint64_t* gain_out,
                    int32_t* inside_out, int32_t* events_out, bf_merge_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_merge_scores before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_merge_scores: opts %p, models %p", (const void*)o, (const void*)models);
    if (o->targets_per_pass < 0) return fail(c, BF_ERR_ARG, "bf_merge_scores: targets_per_pass %d (>= 0)", o->targets_per_pass);
    const VoteWindow w{o->scale, o->sensor_res_x, o->sensor_res_y, o->margin};
    VotePlanes vp;
    int rc = vote_window_check(c, w);
    if (rc == BF_OK && !vote_margin_ok(o->margin))   // (targets_per_pass + 1 >= 1 was checked above: the text is kept)
        rc = fail(c, BF_ERR_ARG, "bf_merge_scores: margin %d (0 .. 65536), targets_per_pass + 1 %d (>= 1)", o->margin, o->targets_per_pass + 1);
    if (rc == BF_OK) rc = vote_planes_check(c, "bf_merge_scores", w, n_models, "", vp);   // (the held grouping is required, as for the projection)
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
    bf_ctx::VoteScratch::Merge& mg = c->vote.merge;
    const size_t bytes = MergeBlock::size(K) * sizeof(unsigned long long);
    HIP_TRY(c, mg.n.grow(plane));   // (everything is grown before the first launch)
    HIP_TRY(c, mg.votes.grow(trial));
    if (a.scale > 1) HIP_TRY(c, mg.box.grow(trial));
    HIP_TRY(c, mg.d_out.grow(MergeBlock::size(kAssignMaxModels)));
    HIP_TRY(c, mg.h_out.grow(MergeBlock::size(kAssignMaxModels)));
    // the base planes: every group under its own model, exactly the projection's, without its compose
    rc = project_base_pass(c, models, vp, 0, nullptr);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(mg.d_out, 0, bytes, s));
    {
        ProfScope ps(c, 3);
        const uint32_t* B = vote_planes_summed(c, vp);
        launch_merge_total(B, K, vp.R, vp.C, mg.n, mg.d_out, s);
        for (int a0 = 0; a0 < K; a0 += A) {   // (the passes follow each other on the stream: they share the trial planes)
            const int targets = K - a0 < A ? K - a0 : A;
            const size_t words = (size_t)targets * (size_t)K * plane;
            HIP_TRY(c, hipMemsetAsync(mg.votes, 0, words * sizeof(uint32_t), s));
            launch_merge_vote(a, a0, targets, mg.votes, mg.d_out, s);
            if (a.scale > 1) launch_assign_box(mg.votes, mg.box, targets * K, vp.R, vp.C, a.scale, s);
            launch_merge_gain(a.scale > 1 ? mg.box.get() : mg.votes.get(), B, mg.n, K, a0, targets, vp.R, vp.C, mg.d_out, s);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(mg.h_out, mg.d_out, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const unsigned long long* h = mg.h_out;
    const ProjectBase base = project_base_decode(c, K);
    for (int b = 0; b < K; ++b)
        for (int t = 0; t < K; ++t) {
            const size_t w = (size_t)b * K + t;
            if (gain_out) gain_out[w] = h[MergeBlock::gain(K, b, t)];
            // (the diagonal is the base pass's: events of b inside under their own model)
            if (inside_out) inside_out[w] = b == t ? base.inside[b] : (int32_t)h[MergeBlock::inside(K, b, t)];
        }
    if (events_out) memcpy(events_out, base.events, (size_t)K * sizeof(int32_t));
    if (info) {
        info->models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = base.unassigned;
        info->passes = passes;
        info->sum = h[MergeBlock::sum(K)];
        info->sum_sq = h[MergeBlock::sum_sq(K)];
    }
    return BF_OK;
}

}  // extern "C"
