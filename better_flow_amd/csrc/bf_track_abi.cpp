// bf_track_abi.cpp -- C-ABI of tracking objects across slices (include/bf_accel.h, "event groups: tracks"):
//   bf_track_keep     keeps the owner plane of the held grouping under its models -- bf_project_groups' label_out, by the
//                     projection's own base pass (project_base_pass) with the label directed into a buffer that no other entry
//                     writes -- together with its window and its number of groups.  The kept plane is not slice state: it
//                     survives the next upload.
//   bf_track_overlap  counts, per group of the slice uploaded NOW, on whose pixels of the kept plane its events land once they
//                     are carried back by the time between the two slices (kernel in bf_track.hip).
//   bf_track_drop     releases the kept plane.
// The checks, the window, the staging of the K warps and the base pass are bf_assign_abi.cpp's (bf_vote_planes.h); the scratch is
// bf_ctx::vote.track, the overlap's result block TrackBlock (bf_group_blocks.h).
#include "bf_track.h"
#include "bf_vote_planes.h"

extern "C" {

int bf_track_keep(bf_ctx* c, const bf_track_opts* o, const bf_model* models, int32_t n_models, int32_t* plane_out,
                  bf_track_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_track_keep before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_track_keep: opts %p, models %p", (const void*)o, (const void*)models);
    const VoteWindow w{o->scale, o->sensor_res_x, o->sensor_res_y, o->margin};
    VotePlanes vp;
    int rc = vote_window_check(c, w);
    if (rc == BF_OK && !vote_margin_ok(o->margin)) rc = fail(c, BF_ERR_ARG, "bf_track_keep: margin %d (0 .. 65536)", o->margin);
    if (rc == BF_OK) rc = vote_planes_check(c, "bf_track_keep", w, n_models, "", vp);   // (the held grouping is required, as for the projection)
    if (rc != BF_OK) return rc;
    const int K = vp.a.K;
    const size_t plane = vp.plane;

    // from here on the call is accepted: the previous plane goes, and a failure below leaves none
    if (info) memset(info, 0, sizeof(*info));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    bf_ctx::VoteScratch::Track& tr = c->vote.track;
    tr.kept.valid = false;
    HIP_TRY(c, tr.plane.grow(plane));
    const bf_ctx::VoteScratch::TrackKept kept{true, K, w, vp.R, vp.C};
    if (c->n == 0) {   // N == 0 everywhere: every label -1
        HIP_TRY(c, hipMemsetAsync(tr.plane, 0xff, plane * sizeof(int32_t), s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (plane_out) memset(plane_out, 0xff, plane * sizeof(int32_t));
        tr.kept = kept;
        return BF_OK;
    }

    // bf_project_groups' base pass under gain 1, the owner plane into the kept buffer
    rc = project_base_pass(c, models, vp, 1, tr.plane);
    if (rc != BF_OK) return rc;
    if (plane_out) HIP_TRY(c, hipMemcpyAsync(plane_out, tr.plane, plane * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    tr.kept = kept;
    if (info) {
        const ProjectBase base = project_base_decode(c, K);
        info->models = K;
        info->kept_models = K;
        info->rows = vp.R; info->cols = vp.C;
        info->unassigned = base.unassigned;
        info->outside = base.outside;
    }
    return BF_OK;
}

int bf_track_overlap(bf_ctx* c, const bf_track_opts* o, const bf_model* models, int32_t n_models, int64_t dt_ns,
                     int32_t* overlap_out, int32_t* inside_out, bf_track_info* info) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_track_overlap before bf_upload_events");
    if (!o || !models) return fail(c, BF_ERR_ARG, "bf_track_overlap: opts %p, models %p", (const void*)o, (const void*)models);
    int rc = held_grouping_check(c, "bf_track_overlap", n_models, "");
    if (rc != BF_OK) return rc;
    const int K = n_models;
    bf_ctx::VoteScratch::Track& tr = c->vote.track;
    const bf_ctx::VoteScratch::TrackKept& kept = tr.kept;
    if (!kept.valid) return fail(c, BF_ERR_STATE, "bf_track_overlap: no plane is kept (bf_track_keep)");
    const VoteWindow w{o->scale, o->sensor_res_x, o->sensor_res_y, o->margin};
    if (!(w == kept.win))
        return fail(c, BF_ERR_ARG, "bf_track_overlap: window (scale %d, sensor %d x %d, margin %d) differs from the kept plane's (%d, %d x %d, %d)",
                    w.scale, w.res_x, w.res_y, w.margin, kept.win.scale, kept.win.res_x, kept.win.res_y, kept.win.margin);
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
    vote_planes_window(c, kept.win, K, vp);   // (the kept options passed bf_track_keep's checks)
    rc = vote_warps_stage(c, models, K, true, vp.a);
    if (rc != BF_OK) return rc;
    const size_t bytes = TrackBlock::size(K, Kp) * sizeof(uint32_t);
    HIP_TRY(c, tr.d_out.grow(TrackBlock::size(kAssignMaxModels, kAssignMaxModels)));
    HIP_TRY(c, tr.h_out.grow(TrackBlock::size(kAssignMaxModels, kAssignMaxModels)));
    HIP_TRY(c, hipMemsetAsync(tr.d_out, 0, bytes, s));
    {
        ProfScope ps(c, 3);
        launch_track_overlap(vp.a, tr.plane, Kp, (long long)dt_ns, tr.d_out, s);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(tr.h_out, tr.d_out, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint32_t* h = tr.h_out;
    for (int k = 0; k < K; ++k) {
        uint32_t row = 0;
        for (int j = 0; j < W; ++j) {
            const uint32_t v = h[TrackBlock::overlap(K, Kp, k, j)];
            row += v;
            if (overlap_out) overlap_out[(size_t)k * W + j] = (int32_t)v;
        }
        if (inside_out) inside_out[k] = (int32_t)row;
    }
    if (info) {
        info->models = K;
        info->kept_models = Kp;
        info->rows = vp.R; info->cols = vp.C;
        info->outside = (int32_t)h[TrackBlock::outside(K, Kp)];
        info->unassigned = (int32_t)h[TrackBlock::unassigned(K, Kp)];
    }
    return BF_OK;
}

int bf_track_drop(bf_ctx* c) {
    if (!c) return BF_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    c->vote.track.kept = bf_ctx::VoteScratch::TrackKept();
    c->vote.track.plane = DevArray<int32_t>();   // (the handle waits for the device before it frees)
    return BF_OK;
}

}  // extern "C"
