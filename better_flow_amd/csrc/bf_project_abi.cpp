// bf_project_abi.cpp -- C-ABI of the projection of a grouping (include/bf_accel.h, "event groups: projection"; kernels in
// bf_project.hip and the box sum of bf_assign.hip): bf_project_groups renders the uploaded slice with every event warped by its
// own group's model -- per pixel the event count, the owning group and its colour -- and scores it: per group and overall the
// integer moments of that image.
#include "bf_ctx.h"

extern "C" {

int bf_project_groups(bf_ctx* c, const bf_project_opts* o, const bf_model* models, int32_t n_models, uint32_t* count_out,
                      int32_t* label_out, uint8_t* bgr_out, bf_group_score* scores_out, bf_project_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_project_groups before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_project_groups: opts %p, models %p", (const void*)o, (const void*)models);
    if (o->scale < 1 || o->scale % 2 == 0 || o->scale / 2 > kMaxHalfScale)
        return fail(c, BF_ERR_ARG, "scale must be odd and <= %d (got %d)", 2 * kMaxHalfScale + 1, o->scale);
    if (o->sensor_res_x < 1 || o->sensor_res_y < 1 || o->sensor_res_x > 65536 || o->sensor_res_y > 65536)
        return fail(c, BF_ERR_ARG, "bad sensor size");
    if (o->margin < 0 || o->margin > 65536 || o->gain < 1)
        return fail(c, BF_ERR_ARG, "bf_project_groups: margin %d (0 .. 65536), gain %d (>= 1)", o->margin, o->gain);
    if (n_models < 1 || n_models > kAssignMaxModels)
        return fail(c, BF_ERR_ARG, "bf_project_groups: %d models (1 .. %d)", n_models, kAssignMaxModels);
    if (c->has_noise) return fail(c, BF_ERR_ARG, "bf_project_groups does not take a noise mask");
    if (!c->groups_valid) return fail(c, BF_ERR_STATE, "bf_project_groups: no grouping of the uploaded slice is held");
    const int K = n_models;
    if (c->groups_K != K) return fail(c, BF_ERR_ARG, "bf_project_groups: the held grouping has %d groups, %d models given", c->groups_K, K);
    // bf_assign_groups' window: the whole sensor widened by the margin (optimizer_rolling.h:248-283)
    const bf_window w = window_of_box(o->scale, -o->margin, o->sensor_res_x - 1 + o->margin, -o->margin, o->sensor_res_y - 1 + o->margin);
    const int R = w.scale_img_x, C = w.scale_img_y;
    const size_t plane = (size_t)R * (size_t)C;
    if ((long long)K * (long long)plane > kAssignMaxWords)
        return fail(c, BF_ERR_CAPACITY, "bf_project_groups: %d planes of %d x %d exceed 2^27 words", K, R, C);

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

    const size_t words = (size_t)K * plane;
    const int nout = project_out_words(K);
    HIP_TRY(c, c->d_assign_votes.grow(words));
    if (o->scale > 1) HIP_TRY(c, c->d_assign_box.grow(words));
    HIP_TRY(c, c->d_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->h_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->d_project_count.grow(plane));
    HIP_TRY(c, c->d_project_label.grow(plane));
    HIP_TRY(c, c->d_project_bgr.grow(3 * plane));
    HIP_TRY(c, c->d_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    for (int k = 0; k < K; ++k) {   // set_model's warp (optimizer_rolling.h:289-299), sine and cosine from the host's libm
        const bf_model& m = models[k];
        set_warp(c->h_assign_wp[k], -m.total_dx, -m.total_dy, m.cx, m.cy, m.total_div, -m.total_rot);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_assign_wp, c->h_assign_wp, (size_t)K * sizeof(WarpParams), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->d_assign_votes, 0, words * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemsetAsync(c->d_project_out, 0, (size_t)nout * sizeof(unsigned long long), s));

    const bf_ctx::EvSet& e = c->set[c->cs];
    AssignArgs a;
    a.xy = e.xy; a.t = e.t;
    a.perm = c->has_perm ? e.perm.get() : nullptr;
    a.wp = c->d_assign_wp;
    a.prior = c->d_group_id.get();   // here: the event's one model
    a.n = c->n;
    a.K = K; a.scale = o->scale;
    a.x_sh = (int)w.x_shift;   // double -> int parameter conversion of accel_lib.h:147
    a.y_sh = (int)w.y_shift;
    a.wsx = w.metric_wsizex; a.wsy = w.metric_wsizey;
    a.R = R; a.C = C;
    {
        ProfScope ps(c, 3);
        launch_project_vote(a, c->d_assign_votes, c->d_project_out, s);
        if (o->scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, R, C, o->scale, s);
        launch_project_compose(o->scale > 1 ? c->d_assign_box.get() : c->d_assign_votes.get(), K, R, C, o->gain, c->d_project_count,
                               c->d_project_label, c->d_project_bgr, c->d_project_out, s);
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
        info->rows = R; info->cols = C;
        info->unassigned = (int32_t)r(t);
        info->outside = (int32_t)outside;
        info->pixels = (int32_t)r(t + 1);
        info->sum = r(t + 2);
        info->sum_sq = r(t + 3);
    }
    return BF_OK;
}

}  // extern "C"
