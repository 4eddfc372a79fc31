// bf_local_abi.cpp -- C-ABI: the contrast-score optimiser OptimizerLocal (optimizer_sampler.h / .cpp) on one window of the
// slice, and the projection image (event_file.h:460-515), which shares its point planes.
#include "bf_ctx.h"

extern "C" {

namespace {

// Event::project -> apply_project (event.h:65-70,164-168) of one event on the host (the centre
// event of the window); this file is compiled with -ffp-contract=off like the kernels.
void project_one(int32_t fr_x, int32_t fr_y, int64_t t, float kx, float ky, double* pr_x, double* pr_y) {
    const float ft = (float)t;
    const float px = kx * ft, py = ky * ft;
    *pr_x = (double)(float)fr_x - (double)px / 10000.0;
    *pr_y = (double)(float)fr_y - (double)py / 10000.0;
}

// point planes, score and image of the contrast-score path (bf_projection_img shares them)
int ensure_lplanes(bf_ctx* c) {
    for (int i = 0; i < 2; ++i) HIP_TRY(c, c->d_lplane[i].grow(c->cap_px));
    HIP_TRY(c, c->d_lscore.grow(2));
    HIP_TRY(c, c->d_limg.grow(c->cap_px));
    HIP_TRY(c, c->h_lscore.grow(2));
    return BF_OK;
}

int local_step(bf_ctx* c, double nx, double ny, double* score, bool want_img) {
    const bf_local_window& w = c->lwin;
    LocalGeom g;
    memset(&g, 0, sizeof(g));
    g.scale = w.scale; g.wsx = w.metric_wsizex; g.wsy = w.metric_wsizey;
    g.R = w.scale_img_x; g.C = w.scale_img_y;
    g.kx = (float)((double)(float)nx / 127.0);   // event.h:164-165, nz is the double 127
    g.ky = (float)((double)(float)ny / 127.0);
    double cpx, cpy;
    project_one(w.c_fr_x, w.c_fr_y, w.c_t, g.kx, g.ky, &cpx, &cpy);           // optimizer_sampler.cpp:122
    g.x_shift = -cpx * (double)w.scale + (double)w.metric_wsizex / 2.0;        // :126
    g.y_shift = -cpy * (double)w.scale + (double)w.metric_wsizey / 2.0;        // :127
    const bf_ctx::EvSet& e = c->set[c->cs];
    HIP_TRY(c, hipMemsetAsync(c->d_lscore, 0, 2 * sizeof(unsigned long long), c->stream));
    launch_local_project_count(e.xy, e.t, c->n, g, c->d_lplane[c->lcur], c->stream);
    if (launch_local_blur_score(c->d_lplane[c->lcur], c->d_lplane[c->lcur ^ 1], g, c->d_lscore,
                                want_img ? c->d_limg.get() : nullptr, c->stream) != 0)
        return fail(c, BF_ERR_ARG, "the 8-bit Gaussian is defined for scale <= 7 (got %d)", w.scale);
    c->lcur ^= 1;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_lscore, c->d_lscore, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // get_event_score, optimizer_sampler.cpp:192-205 (integer sums are exact in a double far beyond any image)
    *score = c->h_lscore[1] == 0 ? 0.0 : (double)c->h_lscore[0] / (double)c->h_lscore[1];
    return BF_OK;
}

}  // namespace

// EventFile::projection_img (event_file.h:460-515) of n events (address words, f32 products, noise flags or null) into d_img (at
// least (scale res_x) x (scale res_y) bytes): enqueued on the context stream, nothing copied, nothing waited for.  Arguments
// checked by the callers.
int render_projection_img_of(bf_ctx* c, const uint32_t* xy, const float2* p, const uint8_t* noise, long long n, int32_t scale,
                             int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_img) {
    const size_t px = (size_t)res_x * scale * (size_t)res_y * scale;
    int rc = ensure_lplanes(c);
    if (rc != BF_OK) return rc;
    // the point planes are shared with the contrast-score path: lay them out afresh for this geometry
    for (int i = 0; i < 2; ++i) HIP_TRY(c, hipMemsetAsync(c->d_lplane[i], 0, c->cap_px * sizeof(uint32_t), c->stream));
    c->local_window_dropped();
    c->lcur = 0;
    HIP_TRY(c, hipMemsetAsync(c->d_lscore, 0, 2 * sizeof(unsigned long long), c->stream));
    launch_proj_count(xy, p, noise, n, scale, res_x, res_y, show_final ? 1 : 0, c->d_lplane[0], c->stream);
    LocalGeom g;
    memset(&g, 0, sizeof(g));
    g.scale = scale; g.R = res_x * scale; g.C = res_y * scale;
    if (launch_local_blur_score(c->d_lplane[0], c->d_lplane[1], g, c->d_lscore, d_img, c->stream) != 0)
        return fail(c, BF_ERR_ARG, "unsupported scale %d", scale);
    launch_proj_scale(d_img, (long long)px, c->d_lscore, c->stream);
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// The same of the live slice.
int render_projection_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_img) {
    const int rc = flush_pending(c);   // a pending bf_set_model warp moves the events first
    if (rc != BF_OK) return rc;
    const bf_ctx::EvSet& e = c->set[c->cs];
    return render_projection_img_of(c, e.xy, e.p, c->has_noise ? c->d_noise.get() : nullptr, c->n, scale, res_x, res_y, show_final, d_img);
}

int bf_local_set_window(bf_ctx* c, int32_t scale, int32_t wsz, int32_t c_fr_x, int32_t c_fr_y, int64_t c_t,
                        bf_local_window* window_out) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_local_set_window before bf_upload_events");
    if (scale < 1 || scale % 2 == 0 || scale > 7)   // optimizer_sampler.cpp:206 (odd); the Gaussian is stated to 7
        return fail(c, BF_ERR_ARG, "scale must be odd and <= 7 (got %d)", scale);
    HIP_TRY(c, hipSetDevice(c->device));
    bf_local_window w;
    memset(&w, 0, sizeof(w));
    w.scale = scale;
    if (wsz <= 0) {   // OptimizerLocal(events, scale), optimizer_sampler.h:35-48
        if (c->n <= 0) return fail(c, BF_ERR_STATE, "the bounding box of an empty cloud is undefined");
        int rc = fold_stats(c);
        if (rc != BF_OK) return rc;
        const SliceStats& s = c->stats;
        w.metric_wsizex = scale * (s.xmax - s.xmin);
        w.metric_wsizey = scale * (s.ymax - s.ymin);
        w.c_fr_x = (s.xmax - s.xmin) / 2 + s.xmin;
        w.c_fr_y = (s.ymax - s.ymin) / 2 + s.ymin;
        w.c_t = 0;
    } else {          // OptimizerLocal(events, e, scale, wsz), :29-33
        w.metric_wsizex = scale * wsz;
        w.metric_wsizey = scale * wsz;
        w.c_fr_x = c_fr_x; w.c_fr_y = c_fr_y; w.c_t = c_t;
    }
    w.scale_img_x = w.metric_wsizex + scale;   // optimizer_sampler.cpp:208-209
    w.scale_img_y = w.metric_wsizey + scale;
    if ((size_t)w.scale_img_x * (size_t)w.scale_img_y > c->cap_px)
        return fail(c, BF_ERR_CAPACITY, "window %d x %d exceeds the image capacity", w.scale_img_x, w.scale_img_y);
    int rc = ensure_lplanes(c);
    if (rc != BF_OK) return rc;
    // a new window lays the planes out afresh
    for (int i = 0; i < 2; ++i) HIP_TRY(c, hipMemsetAsync(c->d_lplane[i], 0, c->cap_px * sizeof(uint32_t), c->stream));
    c->lcur = 0;
    c->lwin = w;
    c->local_window_held();
    if (window_out) *window_out = w;
    return BF_OK;
}

int bf_local_iteration_step(bf_ctx* c, double nx, double ny, double* score, uint8_t* img_out) {
    if (!c || !score) return BF_ERR_ARG;
    if (!c->have_lwin) return fail(c, BF_ERR_STATE, "bf_local_iteration_step before bf_local_set_window");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = local_step(c, nx, ny, score, img_out != nullptr);
    if (rc != BF_OK) return rc;
    if (img_out)
        HIP_TRY(c, hipMemcpy(img_out, c->d_limg, (size_t)c->lwin.scale_img_x * (size_t)c->lwin.scale_img_y,
                             hipMemcpyDeviceToHost));
    return BF_OK;
}

int bf_local_run(bf_ctx* c, int32_t res_x, int32_t res_y, int64_t max_evaluations, bf_local_state* out) {
    if (!c || !out) return BF_ERR_ARG;
    if (!c->have_lwin) return fail(c, BF_ERR_STATE, "bf_local_run before bf_local_set_window");
    HIP_TRY(c, hipSetDevice(c->device));
    const bf_local_window& w = c->lwin;
    bf_local_state st;
    memset(&st, 0, sizeof(st));
    st.dnx = 0.01; st.dny = 0.01;   // optimizer_sampler.cpp:7
    // (NZ * T_DIVIDER * 1000.0) / (10 * scale * FROM_MS(MAX_TIME_MS)), common.h:36,49,60,64
    st.dn_th = (127 * 1 * 1000.0) / (double)(10ull * (unsigned long long)w.scale * 100000000ull);
    *out = st;
    if ((w.scale_img_x < w.scale * res_x / 15) && (w.scale_img_y < w.scale * res_y / 15)) return BF_SKIPPED;   // :9-13
    int rc = local_step(c, st.nx, st.ny, &st.last_score, false);   // :16
    if (rc != BF_OK) return rc;
    st.evaluations = 1;
    while (std::hypot(st.dnx, st.dny) > st.dn_th) {   // :20
        {   // compute_new_nx, :90-102
            const double nx_new = st.nx + st.dnx;
            double new_score;
            if ((rc = local_step(c, nx_new, st.ny, &new_score, false)) != BF_OK) return rc;
            const double dscore = new_score - st.last_score;
            st.last_score = new_score;
            if (dscore <= 0) st.dnx = -st.dnx / 2.0;
            st.nx = nx_new;
        }
        {   // compute_new_ny, :105-117
            const double ny_new = st.ny + st.dny;
            double new_score;
            if ((rc = local_step(c, st.nx, ny_new, &new_score, false)) != BF_OK) return rc;
            const double dscore = new_score - st.last_score;
            st.last_score = new_score;
            if (dscore <= 0) st.dny = -st.dny / 2.0;
            st.ny = ny_new;
        }
        st.evaluations += 2;
        if (max_evaluations > 0 && st.evaluations >= max_evaluations) {
            *out = st;
            return fail(c, BF_ERR_NOCONV, "evaluation cap (%lld) reached", (long long)max_evaluations);
        }
    }
    *out = st;
    return BF_OK;
}

int bf_projection_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* img_out) {
    if (!c || !img_out) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_projection_img before bf_upload_events");
    if (scale < 1 || scale % 2 == 0 || scale > 7) return fail(c, BF_ERR_ARG, "scale must be odd and <= 7 (got %d)", scale);
    if (res_x < 2 || res_y < 2) return fail(c, BF_ERR_ARG, "bad sensor size");
    const size_t px = (size_t)res_x * scale * (size_t)res_y * scale;
    if (px > c->cap_px) return fail(c, BF_ERR_CAPACITY, "image %d x %d exceeds the image capacity", res_x * scale, res_y * scale);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_lplanes(c);
    if (rc != BF_OK) return rc;
    if ((rc = render_projection_img(c, scale, res_x, res_y, show_final, c->d_limg)) != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(img_out, c->d_limg, px, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

}  // extern "C"
