// bf_assign_abi.cpp -- C-ABI of the assignment step (include/bf_accel.h, "event groups: assignment"; kernels in bf_assign.hip):
// bf_assign_groups gives every event of the uploaded slice to one of K candidate models, and may install the result as the
// context's grouping for bf_run_groups.
#include "bf_ctx.h"

extern "C" {

int bf_assign_groups(bf_ctx* c, const bf_assign_opts* o, const bf_model* models, int32_t n_models, int32_t* group_id_out,
                     int32_t* score_out, int32_t* counts_out, bf_assign_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_assign_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_assign_groups: opts %p, models %p", (const void*)o, (const void*)models);
    if (o->scale < 1 || o->scale % 2 == 0 || o->scale / 2 > kMaxHalfScale)
        return fail(c, BF_ERR_ARG, "scale must be odd and <= %d (got %d)", 2 * kMaxHalfScale + 1, o->scale);
    if (o->sensor_res_x < 1 || o->sensor_res_y < 1 || o->sensor_res_x > 65536 || o->sensor_res_y > 65536)
        return fail(c, BF_ERR_ARG, "bad sensor size");
    if (o->margin < 0 || o->margin > 65536 || o->min_score < 1)
        return fail(c, BF_ERR_ARG, "bf_assign_groups: margin %d (0 .. 65536), min_score %d (>= 1)", o->margin, o->min_score);
    if (n_models < 1 || n_models > kAssignMaxModels)
        return fail(c, BF_ERR_ARG, "bf_assign_groups: %d models (1 .. %d)", n_models, kAssignMaxModels);
    if (c->has_noise) return fail(c, BF_ERR_ARG, "bf_assign_groups does not take a noise mask");
    const int K = n_models;
    if (o->use_prior) {
        if (!c->groups_valid) return fail(c, BF_ERR_STATE, "bf_assign_groups: use_prior, but no grouping of the uploaded slice is held");
        if (c->groups_K != K) return fail(c, BF_ERR_ARG, "bf_assign_groups: the held grouping has %d groups, %d models given", c->groups_K, K);
    }
    // the window of the whole sensor widened by the margin (optimizer_rolling.h:248-283): the same for every call on a sensor
    const bf_window w = window_of_box(o->scale, -o->margin, o->sensor_res_x - 1 + o->margin, -o->margin, o->sensor_res_y - 1 + o->margin);
    const int R = w.scale_img_x, C = w.scale_img_y;
    const long long plane = (long long)R * C;
    if ((long long)K * plane > kAssignMaxWords)
        return fail(c, BF_ERR_CAPACITY, "bf_assign_groups: %d planes of %d x %d exceed 2^27 words", K, R, C);

    if (counts_out) memset(counts_out, 0, ((size_t)K + 1) * sizeof(int32_t));
    if (info) memset(info, 0, sizeof(*info));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->n == 0) {   // every output zero; an installed result is the empty grouping
        if (o->install) {
            HIP_TRY(c, c->d_group_id.grow(1));
            c->groups_K = K;
            c->groups_valid = true;
        }
        return BF_OK;
    }

    const size_t words = (size_t)K * (size_t)plane;
    const int nout = assign_out_words(K);
    HIP_TRY(c, c->d_assign_votes.grow(words));
    if (o->scale > 1) HIP_TRY(c, c->d_assign_box.grow(words));
    HIP_TRY(c, c->d_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->h_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->d_assign_gid.grow((size_t)c->n));
    HIP_TRY(c, c->d_assign_score.grow((size_t)c->n));
    HIP_TRY(c, c->d_assign_out.grow((size_t)assign_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_assign_out.grow((size_t)assign_out_words(kAssignMaxModels)));
    for (int k = 0; k < K; ++k) {   // set_model's warp (optimizer_rolling.h:289-299), sine and cosine from the host's libm
        const bf_model& m = models[k];
        set_warp(c->h_assign_wp[k], -m.total_dx, -m.total_dy, m.cx, m.cy, m.total_div, -m.total_rot);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_assign_wp, c->h_assign_wp, (size_t)K * sizeof(WarpParams), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->d_assign_votes, 0, words * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemsetAsync(c->d_assign_out, 0, (size_t)nout * sizeof(uint32_t), s));

    const bf_ctx::EvSet& e = c->set[c->cs];
    AssignArgs a;
    a.xy = e.xy; a.t = e.t;
    a.perm = c->has_perm ? e.perm.get() : nullptr;
    a.wp = c->d_assign_wp;
    a.prior = o->use_prior ? c->d_group_id.get() : nullptr;
    a.n = c->n;
    a.K = K; a.scale = o->scale;
    a.x_sh = (int)w.x_shift;   // double -> int parameter conversion of accel_lib.h:147
    a.y_sh = (int)w.y_shift;
    a.wsx = w.metric_wsizex; a.wsy = w.metric_wsizey;
    a.R = R; a.C = C;
    {
        ProfScope ps(c, 3);
        launch_assign_vote(a, c->d_assign_votes, s);
        if (o->scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, R, C, o->scale, s);
        launch_assign_pick(a, o->scale > 1 ? c->d_assign_box.get() : c->d_assign_votes.get(), o->min_score, c->d_assign_gid,
                           c->d_assign_score, c->d_assign_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_assign_out, c->d_assign_out, (size_t)nout * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (group_id_out)
        HIP_TRY(c, hipMemcpyAsync(group_id_out, c->d_assign_gid, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (score_out)
        HIP_TRY(c, hipMemcpyAsync(score_out, c->d_assign_score, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (o->install) {   // the rule of bf_set_groups: the context's own plane, held until the next upload
        c->groups_valid = false;
        HIP_TRY(c, c->d_group_id.grow((size_t)c->n));
        HIP_TRY(c, hipMemcpyAsync(c->d_group_id, c->d_assign_gid, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        c->groups_K = K;
        c->groups_valid = true;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* r = c->h_assign_out;
    if (counts_out)
        for (int k = 0; k <= K; ++k) counts_out[k] = (int32_t)r[k];
    if (info) {
        info->models = K;
        info->rows = R; info->cols = C;
        info->unassigned = (int32_t)r[K];
        info->assigned = (int32_t)(c->n - (long long)r[K]);
        info->changed = (int32_t)r[K + 1];
        info->max_score = (int32_t)r[K + 2];
    }
    return BF_OK;
}

}  // extern "C"
