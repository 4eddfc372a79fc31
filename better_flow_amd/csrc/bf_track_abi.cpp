// bf_track_abi.cpp -- C-ABI of tracking objects across slices (include/bf_accel.h, "event groups: tracks"):
//   bf_track_keep     keeps the owner plane of the held grouping under its models -- bf_project_groups' label_out, by the
//                     projection's own kernels with the label directed into a buffer that no other entry writes -- together with
//                     its window and its number of groups.  The kept plane is not slice state: it survives the next upload.
//   bf_track_overlap  counts, per group of the slice uploaded NOW, on whose pixels of the kept plane its events land once they
//                     are carried back by the time between the two slices (kernel in bf_track.hip).
//   bf_track_drop     releases the kept plane.
// The option checks, the window and the staging of the K warps are bf_assign_abi.cpp's (vote_planes_*).
#include "bf_ctx.h"
#include "bf_track.h"

extern "C" {

int bf_track_keep(bf_ctx* c, const bf_track_opts* o, const bf_model* models, int32_t n_models, int32_t* plane_out,
                  bf_track_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_track_keep before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_track_keep: opts %p, models %p", (const void*)o, (const void*)models);
    VotePlanes vp;
    int rc = vote_planes_check(c, "bf_track_keep", o->scale, o->sensor_res_x, o->sensor_res_y, o->margin, "gain", 1, n_models, "",
                               vp);   // (the held grouping is required, as for the projection)
    if (rc != BF_OK) return rc;
    const AssignArgs& a = vp.a;
    const int K = a.K;
    const size_t plane = vp.plane;

    // from here on the call is accepted: the previous plane goes, and a failure below leaves none
    if (info) memset(info, 0, sizeof(*info));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->track.valid = false;
    HIP_TRY(c, c->d_track_plane.grow(plane));
    bf_ctx::TrackKept kept;
    kept.Kp = K;
    kept.scale = o->scale; kept.res_x = o->sensor_res_x; kept.res_y = o->sensor_res_y; kept.margin = o->margin;
    kept.R = vp.R; kept.C = vp.C;
    if (c->n == 0) {   // N == 0 everywhere: every label -1
        HIP_TRY(c, hipMemsetAsync(c->d_track_plane, 0xff, plane * sizeof(int32_t), s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (plane_out) memset(plane_out, 0xff, plane * sizeof(int32_t));
        kept.valid = true;
        c->track = kept;
        return BF_OK;
    }

    // bf_project_groups' launches, the label into the kept buffer; count, colour and the result block are the projection's scratch
    const int nout = project_out_words(K);
    rc = vote_planes_stage(c, models, true, vp);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, c->d_project_count.grow(plane));
    HIP_TRY(c, c->d_project_bgr.grow(3 * plane));
    HIP_TRY(c, c->d_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, c->h_project_out.grow((size_t)project_out_words(kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(c->d_project_out, 0, (size_t)nout * sizeof(unsigned long long), s));
    {
        ProfScope ps(c, 3);
        launch_project_vote(a, c->d_assign_votes, c->d_project_out, s);
        if (a.scale > 1) launch_assign_box(c->d_assign_votes, c->d_assign_box, K, vp.R, vp.C, a.scale, s);
        launch_project_compose(vote_planes_summed(c, vp), K, vp.R, vp.C, 1, c->d_project_count, c->d_track_plane, c->d_project_bgr,
                               c->d_project_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_project_out, c->d_project_out, (size_t)nout * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (plane_out) HIP_TRY(c, hipMemcpyAsync(plane_out, c->d_track_plane, plane * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    kept.valid = true;
    c->track = kept;
    if (info) {
        const unsigned long long* h = c->h_project_out;
        auto r = [h](int word) { return h[(size_t)word * kProjectStride]; };
        long long outside = 0;
        for (int k = 0; k < K; ++k) outside += (long long)r(k) - (long long)r(K + k);
        info->models = K;
        info->kept_models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = (int32_t)r(kProjectTables * K);
        info->outside = (int32_t)outside;
    }
    return BF_OK;
}

int bf_track_overlap(bf_ctx* c, const bf_track_opts* o, const bf_model* models, int32_t n_models, int64_t dt_ns,
                     int32_t* overlap_out, int32_t* inside_out, bf_track_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_track_overlap before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_track_overlap: opts %p, models %p", (const void*)o, (const void*)models);
    if (n_models < 1 || n_models > kAssignMaxModels)
        return fail(c, BF_ERR_ARG, "bf_track_overlap: %d models (1 .. %d)", n_models, kAssignMaxModels);
    if (c->has_noise) return fail(c, BF_ERR_ARG, "bf_track_overlap does not take a noise mask");
    const int K = n_models;
    if (!c->groups_valid) return fail(c, BF_ERR_STATE, "bf_track_overlap: no grouping of the uploaded slice is held");
    if (c->groups_K != K)
        return fail(c, BF_ERR_ARG, "bf_track_overlap: the held grouping has %d groups, %d models given", c->groups_K, K);
    const bf_ctx::TrackKept& kept = c->track;
    if (!kept.valid) return fail(c, BF_ERR_STATE, "bf_track_overlap: no plane is kept (bf_track_keep)");
    if (o->scale != kept.scale || o->sensor_res_x != kept.res_x || o->sensor_res_y != kept.res_y || o->margin != kept.margin)
        return fail(c, BF_ERR_ARG, "bf_track_overlap: window (scale %d, sensor %d x %d, margin %d) differs from the kept plane's (%d, %d x %d, %d)",
                    o->scale, o->sensor_res_x, o->sensor_res_y, o->margin, kept.scale, kept.res_x, kept.res_y, kept.margin);
    constexpr int64_t kMaxDt = (int64_t)1 << 40;
    if (dt_ns > kMaxDt || dt_ns < -kMaxDt) return fail(c, BF_ERR_ARG, "bf_track_overlap: |dt_ns| %lld exceeds 2^40", (long long)dt_ns);
    const int Kp = kept.Kp, W = Kp + 1;

    if (overlap_out) memset(overlap_out, 0, (size_t)K * (size_t)W * sizeof(int32_t));
    if (inside_out) memset(inside_out, 0, (size_t)K * sizeof(int32_t));
    if (info) memset(info, 0, sizeof(*info));
    if (c->n == 0) return BF_OK;   // every output zero
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;

    VotePlanes vp;
    vote_planes_window(c, kept.scale, kept.res_x, kept.res_y, kept.margin, K, vp);   // (the kept options passed bf_track_keep's checks)
    AssignArgs& a = vp.a;
    const size_t out_size = track_out_size(K, Kp);
    HIP_TRY(c, c->d_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->h_assign_wp.grow((size_t)kAssignMaxModels));
    HIP_TRY(c, c->d_track_out.grow(track_out_size(kAssignMaxModels, kAssignMaxModels)));
    HIP_TRY(c, c->h_track_out.grow(track_out_size(kAssignMaxModels, kAssignMaxModels)));
    for (int k = 0; k < K; ++k) set_model_warp(c->h_assign_wp[k], models[k]);   // (sine and cosine from the host's libm)
    HIP_TRY(c, hipMemcpyAsync(c->d_assign_wp, c->h_assign_wp, (size_t)K * sizeof(WarpParams), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(c->d_track_out, 0, out_size * sizeof(uint32_t), s));
    const bf_ctx::EvSet& e = c->set[c->cs];
    a.xy = e.xy; a.t = e.t;
    a.perm = c->has_perm ? e.perm.get() : nullptr;
    a.wp = c->d_assign_wp;
    a.prior = c->d_group_id.get();
    {
        ProfScope ps(c, 3);
        launch_track_overlap(a, c->d_track_plane, Kp, (long long)dt_ns, c->d_track_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_track_out, c->d_track_out, out_size * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* h = c->h_track_out;
    auto r = [h](size_t word) { return h[word * kTrackStride]; };
    for (int k = 0; k < K; ++k) {
        uint32_t row = 0;
        for (int j = 0; j < W; ++j) {
            const uint32_t v = r((size_t)k * W + j);
            row += v;
            if (overlap_out) overlap_out[(size_t)k * W + j] = (int32_t)v;
        }
        if (inside_out) inside_out[k] = (int32_t)row;
    }
    if (info) {
        info->models = K;
        info->kept_models = Kp;
        info->rows = vp.R; info->cols = vp.C;
        info->outside = (int32_t)r((size_t)K * W);
        info->unassigned = (int32_t)r((size_t)K * W + 1);
    }
    return BF_OK;
}

int bf_track_drop(bf_ctx* c) {
    if (!c) return BF_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    c->track = bf_ctx::TrackKept();
    c->d_track_plane = DevArray<int32_t>();   // (the handle waits for the device before it frees)
    return BF_OK;
}

}  // extern "C"
