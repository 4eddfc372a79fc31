// bf_operators.cpp -- C-ABI: OptimizerRolling::set_cloud / set_scale (optimizer_rolling.h:248-283) with the per-slice choice of loop and
// scatter format, and the one-to-one AccelLib operators (accel_lib.h:147-178,263-267,310-341,513-615) with the per-event read-backs.
#include "bf_ctx.h"

extern "C" {

int bf_set_cloud(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, bf_window* window_out) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_set_cloud before bf_upload_events");
    if (scale < 1 || scale % 2 == 0 || scale / 2 > kMaxHalfScale)   // optimizer_rolling.h:274
        return fail(c, BF_ERR_ARG, "scale must be odd and <= %d (got %d)", 2 * kMaxHalfScale + 1, scale);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = fold_stats(c);
    if (rc != BF_OK) return rc;
    const SliceStats s = c->stats;
    c->segmentation_dropped();
    // optimizer_rolling.h:252-260: min seeded with RES, max with 0
    int x_min = res_x, y_min = res_y, x_max = 0, y_max = 0;
    if (c->n > 0) {
        if (s.tmin == INT_MIN)
            return fail(c, BF_ERR_ARG, "a slice-local event time does not fit 32 bits (slice longer than 2.1 s?)");
        if (s.xmin < 0 || s.ymin < 0 || s.xmax > 65535 || s.ymax > 65535)
            return fail(c, BF_ERR_ARG, "event coordinates outside [0, 65535]");
        if (s.xmax > x_max) x_max = s.xmax;
        if (s.ymax > y_max) y_max = s.ymax;
        if (s.xmin < x_min) x_min = s.xmin;
        if (s.ymin < y_min) y_min = s.ymin;
    }
    const bf_window w = window_of_box(scale, x_min, x_max, y_min, y_max);
    if (w.scale_img_x <= 0 || w.scale_img_y <= 0) {
        // e.g. an empty slice: x_min = RES_X > x_max = 0.  The reference carries on and run()
        // returns 1 at the window guard (:49-55); no image operator is usable on it.
        c->win = w;
        c->window_set(true);
        memset(&c->hst.model, 0, sizeof(c->hst.model));
        if (window_out) *window_out = w;
        return BF_OK;
    }
    if ((size_t)w.scale_img_x * (size_t)w.scale_img_y > c->cap_px)
        return fail(c, BF_ERR_CAPACITY, "window %d x %d exceeds the image capacity", w.scale_img_x, w.scale_img_y);
    if (w.scale_img_x > 65535 || w.scale_img_y > 65535)   // 16-bit pixel coordinates in the packed moment sums
        return fail(c, BF_ERR_CAPACITY, "window %d x %d: at most 65535 rows / columns", w.scale_img_x, w.scale_img_y);
    int gx, gy;
    stencil_grid(w.scale_img_x, w.scale_img_y, &gx, &gy);
    if (gx * gy > c->cap_blocks) return fail(c, BF_ERR_CAPACITY, "window needs %d tiles > %d", gx * gy, c->cap_blocks);

    // Accumulator packing: count << tbits | sum(t - tmin).  Exact iff both fields can hold the
    // whole slice (no pixel can collect more than all events / all time).
    long long tmin = (c->n > 0) ? (long long)s.tmin : 0;
    unsigned long long span_sum = (c->n > 0) ? (unsigned long long)(s.tsum - tmin * c->n) : 0ull;
    int tbits = bit_length(span_sum);
    if (tbits < 1) tbits = 1;
    int cbits = bit_length((unsigned long long)c->n);
    c->packed = !c->force_split && (tbits + cbits <= 64);
    if (!c->packed) {
        rc = ensure_cplanes(c);
        if (rc != BF_OK) return rc;
        tbits = 64;
    }

    // Event::reset for every event (set_cloud :260).  bf_upload_events already reset p.
    if (!c->p_clean) HIP_TRY(c, hipMemsetAsync(c->set[c->cs].p, 0, (size_t)c->n_pad * sizeof(float2), c->stream));
    // The window and everything the flags say about it change together, once nothing can refuse the call any more: a
    // bf_set_cloud refused above (capacity) leaves the previous window as it was, its `degenerate` included.
    c->win = w;
    c->window_set(false);
    DevState& h = c->hst;
    h.hot.scale = scale;
    h.hot.R = w.scale_img_x; h.hot.C = w.scale_img_y;
    h.hot.wsx = w.metric_wsizex; h.hot.wsy = w.metric_wsizey;
    h.hot.x_sh = (int)w.x_shift;   // double -> int parameter conversion of accel_lib.h:147
    h.hot.y_sh = (int)w.y_shift;
    h.hot.tbits = tbits;
    h.x_shift = w.x_shift; h.y_shift = w.y_shift;
    h.hot.tmin = tmin;
    h.nblocks = gx * gy;
    memset(&h.model, 0, sizeof(h.model));   // a fresh OptimizerRolling has a zero ObjectModel
    h.hot.wp = identity_warp();
    h.hot.it = 0; h.hot.done = 0; h.rc = 0;
    // The slice's bin grids and scatter format (plan_slice); the buffers they need are allocated here, in this order.
    const SlicePlan p = plan_slice(c, w);
    c->planned_binned(p.binned);
    if (c->use_binned) {
        rc = ensure_cplanes(c);
        if (rc == BF_OK) rc = ensure_bin_buffers(c, p.grid);
        if (rc == BF_OK) rc = ensure_ovf_bits(c, w.scale_img_x, w.scale_img_y);
        if (rc != BF_OK) return rc;
        c->grid = p.grid;
    }
    c->planned_one_kernel(false);
    if (p.fused_ok) {
        rc = ensure_cplanes(c);
        if (rc == BF_OK) rc = ensure_bin_buffers(c, p.fgrid);
        if (rc != BF_OK) return rc;
        HIP_TRY(c, c->d_ftab.grow((size_t)p.fgrid.nbr * p.fgrid.nbc * kFusedTabWords));
        for (int i = 0; i < 2; ++i) HIP_TRY(c, c->set[i].p2.grow((size_t)c->cap_events));
        c->fgrid = p.fgrid;
        c->planned_one_kernel(true);
        c->planned_one_kernel_shared(p.fused_shared);
    }
    h.hot.binned = (c->use_binned || c->fused_ok) ? 1 : 0;
    h.hot.pp = 0; h.hot.redo = 0; h.hot.pend = 0; h.last_j = -1;
    h.n_events = (uint32_t)c->n;
    h.hot.bin_tbits = tbits > 62 ? 62 : tbits; h.hot.bin_ok = 1; h.hot.need_rebin = 0; h.hot.rebins = 0; h.ovf_total = 0;
    h.hot.flip = 0;
    c->fmt = 0;
    if (p.fmt == 3) {
        rc = ensure_margin_buffers(c, p.grid);
        if (rc != BF_OK) return rc;
    }
    c->fmt = p.fmt;
    h.hot.fmt = c->fmt;
    c->grid.zw = p.zw;
    h.t_span = (c->n > 0) ? (long long)s.tmax - (long long)s.tmin : 0;
    h.t_abs_max = (c->n > 0) ? std::fmax(std::fabs((double)s.tmin), std::fabs((double)s.tmax)) : 0.0;
    h.r_max = std::hypot((double)(w.x_max - w.x_min), (double)(w.y_max - w.y_min)) + 64.0;
    h.drift_limit = c->opt_bin_predict ? 0.6 * (double)c->grid.D : 1e300;
    if (c->planes_unknown || w.scale_img_x != c->last_R || w.scale_img_y != c->last_C) {
        rc = clear_planes(c);
        if (rc != BF_OK) return rc;
    }
    c->last_R = w.scale_img_x;
    c->last_C = w.scale_img_y;
    // (the device copy of the state is written by whoever uses it next -- bf_run, the AccelLib operators,
    // flush_pending all upload c->hst first; a launch here would only add ~5 us to every slice)
    if (window_out) *window_out = w;
    return BF_OK;
}

// ---- AccelLib operators ----------------------------------------------------------------

// The final warp of bf_run writes its per-event outputs in slot (tile-sorted) order -- coalesced stores instead of
// 16-byte stores scattered through perm[] (31 -> 10 us per 1M events) -- and they are put back into upload order only
// when somebody reads them.
static int materialize_outputs(bf_ctx* c) {
    if (!c->out_sorted) return BF_OK;
    c->outputs_materialised();
    if (!c->has_perm || c->n == 0) return BF_OK;
    HIP_TRY(c, c->d_out_tmp.grow((size_t)c->cap_events));
    const uint32_t* perm = c->set[c->cs].perm;
    launch_unpermute(c->d_nxny, perm, c->d_out_tmp, c->n, c->stream);
    std::swap(c->d_nxny, c->d_out_tmp);
    if (c->uv_valid) {
        launch_unpermute(c->d_uv, perm, c->d_out_tmp, c->n, c->stream);
        std::swap(c->d_uv, c->d_out_tmp);
    }
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// The entry of an operator on the live window: one that is not degenerate, the device set, bf_set_model's warp applied.
static int window_op_begin(bf_ctx* c, const char* name) {
    if (!c) return BF_ERR_ARG;
    if (!c->have_window) return fail(c, BF_ERR_STATE, "%s before bf_set_cloud", name);
    if (c->degenerate) return fail(c, BF_ERR_STATE, "%s on a degenerate (empty) window", name);
    HIP_TRY(c, hipSetDevice(c->device));
    return flush_pending(c);
}

int bf_project_4param_reinit(bf_ctx* c, double dnx_, double dny_, double cx, double cy, double div,
                             double crl) {
    int rc = window_op_begin(c, "bf_project_4param_reinit");
    if (rc != BF_OK) return rc;
    set_warp(c->hst.hot.wp, dnx_, dny_, cx, cy, div, crl);
    launch_set_state(c->d_state, c->hst, c->stream);
    {
        ProfScope ps(c, 0, c->n);
        launch_warp_scatter(ws_args(c, c->cur, 0), true, false, true, c->stream);
    }
    c->events_warped();
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

int bf_project_4param(bf_ctx* c, double dnx_, double dny_, double cx, double cy, double div, double crl) {
    int rc = window_op_begin(c, "bf_project_4param");
    if (rc != BF_OK) return rc;
    rc = materialize_outputs(c);   // (the events' (nx, ny) in upload order, whatever left them)
    if (rc != BF_OK) return rc;
    set_warp(c->hst.hot.wp, dnx_, dny_, cx, cy, div, crl);
    launch_set_state(c->d_state, c->hst, c->stream);
    const bf_ctx::EvSet& e = c->set[c->cs];
    {
        ProfScope ps(c, 0, c->n);
        launch_project_dn(e.xy, e.t, e.p, c->d_nxny, c->has_perm ? e.perm : nullptr, c->n_valid ? 1 : 0, c->d_state, c->n, c->stream);
    }
    c->events_warped();
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

}  // extern "C"

int ctx_time_img_pass(bf_ctx* c, const char* who) {
    int rc = window_op_begin(c, who);
    if (rc != BF_OK) return rc;
    launch_set_state(c->d_state, c->hst, c->stream);
    const int buf = c->cur;
    if (!c->all_noise) {
        ProfScope ps(c, 0, c->n);
        launch_warp_scatter(ws_args(c, buf, 0), false, true, false, c->stream);
    }
    StencilArgs a = st_args(c, buf, 0);
    a.time_out = c->d_time;
    a.count_out = c->d_count;
    a.zero_cplane = c->d_cplane[buf ^ 1];   // may be NULL (never allocated): nothing to clear
    {
        ProfScope ps(c, 1);
        launch_stencil(a, plane_src(c), c->stream, c->n_cus);
    }
    HIP_TRY(c, hipGetLastError());
    c->cur = buf ^ 1;   // the stencil zeroed the other buffer; `buf` is cleared by the next pass
    c->hst.hot.ovf_cnt[buf] = 1;
    c->hst.hot.ovf_cnt[buf ^ 1] = 0;
    return BF_OK;
}

extern "C" {

int bf_get_time_img(bf_ctx* c, float* time_out, uint32_t* count_out) {
    int rc = ctx_time_img_pass(c, "bf_get_time_img");
    if (rc != BF_OK) return rc;
    const size_t P = (size_t)c->win.scale_img_x * (size_t)c->win.scale_img_y;
    if (time_out)
        HIP_TRY(c, hipMemcpyAsync(time_out, c->d_time, P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (count_out)
        HIP_TRY(c, hipMemcpyAsync(count_out, c->d_count, P * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

static int image_pass(bf_ctx* c, const float* d_src, int rows, int cols, bool grads, bool moments) {
    StencilArgs a;
    memset(&a, 0, sizeof(a));
    a.st = c->d_state;
    a.R = rows; a.C = cols; a.scale = 1;
    a.time_in = d_src;
    if (grads) { a.gx_out = c->d_gx; a.gy_out = c->d_gy; }
    if (moments) {   // sums -> exact accumulators; the last work-group forms the model (mode 0)
        if (c->acc_dirty) {
            if (hipMemsetAsync(c->d_acc, 0, 2 * kAccGroups * sizeof(MomentAcc), c->stream) != hipSuccess) return BF_ERR_HIP;
            c->acc_dirty = false;
        }
        a.acc = c->d_acc;
        a.ticket = c->d_ticket;
        a.st_rw = c->d_state;
        a.update_mode = 0;
    }
    ProfScope ps(c, 1);
    launch_stencil(a, StencilSrc::time_image, c->stream);
    return BF_OK;
}

int bf_sobel(bf_ctx* c, const float* img, int32_t rows, int32_t cols, float* grad_x, float* grad_y) {
    if (!c) return BF_ERR_ARG;
    if (!img || !grad_x || !grad_y || rows <= 0 || cols <= 0) return fail(c, BF_ERR_ARG, "bad image");
    const size_t P = (size_t)rows * (size_t)cols;
    if (P > c->cap_px) return fail(c, BF_ERR_CAPACITY, "image %d x %d exceeds capacity", rows, cols);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->d_img, img, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    image_pass(c, c->d_img, rows, cols, true, false);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(grad_x, c->d_gx, P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(grad_y, c->d_gy, P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

int bf_fast_model(bf_ctx* c, const float* img, int32_t rows, int32_t cols, bf_model* model) {
    if (!c) return BF_ERR_ARG;
    if (!model) return fail(c, BF_ERR_ARG, "model is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const float* src = c->d_time;
    if (img) {
        if (rows <= 0 || cols <= 0) return fail(c, BF_ERR_ARG, "bad image");
        const size_t P = (size_t)rows * (size_t)cols;
        if (P > c->cap_px) return fail(c, BF_ERR_CAPACITY, "image %d x %d exceeds capacity", rows, cols);
        HIP_TRY(c, hipMemcpyAsync(c->d_img, img, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
        src = c->d_img;
    } else {
        if (!c->have_window) return fail(c, BF_ERR_STATE, "no resident time image");
        rows = c->win.scale_img_x;
        cols = c->win.scale_img_y;
    }
    int gx, gy;
    stencil_grid(rows, cols, &gx, &gy);
    if (gx * gy > c->cap_blocks) return fail(c, BF_ERR_CAPACITY, "image needs %d tiles", gx * gy);
    DevState tmp = c->hst;
    tmp.hot.R = rows; tmp.hot.C = cols;
    launch_set_state(c->d_state, tmp, c->stream);
    image_pass(c, src, rows, cols, false, true);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bf_model& m = c->h_state[0].model;
    model->cx = m.cx; model->cy = m.cy;
    model->dx = m.dx; model->dy = m.dy;
    model->rot = m.rot; model->div = m.div;
    model->cnt = m.cnt;
    return BF_OK;
}

// The per-event flow in d_uv, in upload order (bf_run with want_uv already produced it in its final warp).
static int ensure_uv(bf_ctx* c) {
    const int rc = materialize_outputs(c);
    if (rc != BF_OK) return rc;
    if (!c->uv_valid) {
        ProfScope ps(c, 3);
        launch_compute_uv(c->d_nxny, c->d_uv, c->n, c->stream);
        c->uv_computed();
    }
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// The per-event flow of the live slice in upload order on the device, as bf_compute_uv_ring would read it back; null when
// no warp has run (Event::reset: zero flow) or the window is degenerate.  For bf_emit_slice (bf_emit.cpp).
int ctx_device_uv(bf_ctx* c, const double2** uv) {
    *uv = nullptr;
    int rc = flush_pending(c);
    if (rc != BF_OK) return rc;
    if (c->n == 0 || !c->n_valid || !c->have_window || c->degenerate) return BF_OK;
    rc = ensure_uv(c);
    if (rc != BF_OK) return rc;
    *uv = c->d_uv;
    return BF_OK;
}

// The per-event (nx, ny) of the live slice in upload order on the device; null when no warp has run or the window is
// degenerate.  For the flow field (bf_flow_abi.cpp), which forms (u, v) at the owning events only.
int ctx_device_nxny(bf_ctx* c, const double2** nxny) {
    *nxny = nullptr;
    int rc = flush_pending(c);
    if (rc != BF_OK) return rc;
    if (c->n == 0 || !c->n_valid || !c->have_window || c->degenerate) return BF_OK;
    rc = materialize_outputs(c);
    if (rc != BF_OK) return rc;
    *nxny = c->d_nxny;
    return BF_OK;
}

// (d_src null: zeros -- Event::reset leaves nx = ny = 0, event.h:57)
static int copy_pairs(bf_ctx* c, const double2* d_src, double* a, double* b) {
    std::vector<double2> tmp((size_t)c->n);
    if (d_src) {
        HIP_TRY(c, hipMemcpyAsync(tmp.data(), d_src, (size_t)c->n * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    for (long long i = 0; i < c->n; ++i) {
        if (a) a[i] = tmp[(size_t)i].x;
        if (b) b[i] = tmp[(size_t)i].y;
    }
    return BF_OK;
}

int bf_writeout_events(bf_ctx* c, double* pr_x, double* pr_y, double* nx, double* ny) {
    int rc = window_op_begin(c, "bf_writeout_events");
    if (rc != BF_OK) return rc;
    if (c->n == 0) return BF_OK;
    rc = materialize_outputs(c);
    if (rc != BF_OK) return rc;
    if (pr_x || pr_y) {
        c->uv_buffer_reused();   // d_uv is the staging buffer of the expanded positions below
        {
            ProfScope ps(c, 3);
            launch_expand_pr(c->set[c->cs].xy, c->set[c->cs].p, c->has_perm ? c->set[c->cs].perm : nullptr,
                             c->d_uv, c->n, c->stream);
        }
        HIP_TRY(c, hipGetLastError());
        rc = copy_pairs(c, c->d_uv, pr_x, pr_y);
        if (rc != BF_OK) return rc;
    }
    if (nx || ny) return copy_pairs(c, c->n_valid ? (const double2*)c->d_nxny : nullptr, nx, ny);
    return BF_OK;
}

int bf_compute_uv(bf_ctx* c, double* u, double* v) {
    int rc = window_op_begin(c, "bf_compute_uv");
    if (rc != BF_OK) return rc;
    if (c->n == 0) return BF_OK;
    if (!c->n_valid) return copy_pairs(c, nullptr, u, v);
    rc = ensure_uv(c);
    return rc != BF_OK ? rc : copy_pairs(c, c->d_uv, u, v);
}

int bf_compute_uv_ring(bf_ctx* c, double* uv_ring, int64_t cap, int64_t first) {
    if (!c) return BF_ERR_ARG;
    if (!c->have_window) return fail(c, BF_ERR_STATE, "bf_compute_uv_ring before bf_set_cloud");
    if (c->degenerate) return fail(c, BF_ERR_STATE, "bf_compute_uv_ring on a degenerate (empty) window");
    if (!uv_ring || cap <= 0 || first < 0 || first >= cap || c->n > cap)
        return fail(c, BF_ERR_ARG, "bad flow ring (cap %lld, first %lld, n %lld)", (long long)cap, (long long)first, c->n);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc != BF_OK) return rc;
    if (c->n == 0) return BF_OK;
    const int64_t n0 = (first + c->n <= cap) ? c->n : cap - first, n1 = c->n - n0;
    if (!c->n_valid) {   // Event::reset state: no flow yet
        memset(uv_ring + 2 * first, 0, (size_t)n0 * 16);
        memset(uv_ring, 0, (size_t)n1 * 16);
        return BF_OK;
    }
    rc = ensure_uv(c);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(uv_ring + 2 * first, c->d_uv, (size_t)n0 * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    if (n1 > 0) HIP_TRY(c, hipMemcpyAsync(uv_ring, c->d_uv + n0, (size_t)n1 * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

}  // extern "C"
