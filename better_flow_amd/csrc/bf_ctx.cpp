// bf_ctx.cpp -- the helpers the C-ABI files share (declared in bf_ctx.h): error text, the profiling fold, warps and windows on the
// host, the buffers allocated on first use, the pending warp, the slice statistics, the held grouping.
#include "bf_ctx.h"

int fail(bf_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        std::lock_guard<std::mutex> g(c->err_mu);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

int prof_fold(bf_ctx* c) {
    if (c->prof_pending.empty()) return BF_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (auto& r : c->prof_pending) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        switch (r.cat) {
            case 0: c->prof.warp_scatter_ms += ms; c->prof.warp_scatter_launches++;
                    c->prof.warp_scatter_events += (uint64_t)r.nev; break;
            case 1: c->prof.stencil_ms += ms; c->prof.stencil_launches++; break;
            case 2: c->prof.update_ms += ms; c->prof.update_launches++; break;
            default: c->prof.other_ms += ms; c->prof.other_launches++; break;
        }
        c->ev_pool.push_back(std::move(r.a));
        c->ev_pool.push_back(std::move(r.b));
    }
    c->prof_pending.clear();
    return BF_OK;
}

long long pad_events(long long n) {
    constexpr long long gran = (long long)kThreads * kEvPerThread;
    return (n + gran - 1) / gran * gran;
}

int bit_length(unsigned long long v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

void set_warp(WarpParams& w, double dnx, double dny, double cx, double cy, double div, double angle) {
    w.dnx = dnx; w.dny = dny; w.cx = cx; w.cy = cy; w.div = div;
    w.c = std::cos(angle);
    w.s = std::sin(angle);
}
void set_model_warp(WarpParams& w, const bf_model& m) {
    set_warp(w, -m.total_dx, -m.total_dy, m.cx, m.cy, m.total_div, -m.total_rot);
}

WarpParams identity_warp() {
    WarpParams w;
    w.dnx = w.dny = w.cx = w.cy = w.div = 0.0;
    w.c = 1.0;
    w.s = 0.0;
    return w;
}

bf_window window_of_box(int scale, int x_min, int x_max, int y_min, int y_max) {
    bf_window w;
    memset(&w, 0, sizeof(w));
    w.scale = scale;
    w.x_min = x_min; w.y_min = y_min; w.x_max = x_max; w.y_max = y_max;
    w.metric_wsizex = scale * (w.x_max - w.x_min);   // :263
    w.metric_wsizey = scale * (w.y_max - w.y_min);   // :264
    w.scale_img_x = w.metric_wsizex + scale;         // :276
    w.scale_img_y = w.metric_wsizey + scale;         // :277
    // :279-282, both "/ 2" are integer divisions
    w.x_shift = -double((w.x_max - w.x_min) / 2 + w.x_min) * double(scale) +
                double(w.metric_wsizex) / 2.0 + scale / 2;
    w.y_shift = -double((w.y_max - w.y_min) / 2 + w.y_min) * double(scale) +
                double(w.metric_wsizey) / 2.0 + scale / 2;
    return w;
}

template <class T> hipError_t grow_zeroed(bf_ctx* c, DevArray<T>& a, size_t n) {
    bool fresh;
    const hipError_t e = a.grow(n, &fresh);
    return (e == hipSuccess && fresh) ? hipMemsetAsync(a, 0, n * sizeof(T), c->stream) : e;
}
template hipError_t grow_zeroed<uint32_t>(bf_ctx*, DevArray<uint32_t>&, size_t);
template hipError_t grow_zeroed<unsigned long long>(bf_ctx*, DevArray<unsigned long long>&, size_t);

int ensure_cplanes(bf_ctx* c) {
    for (int i = 0; i < 2; ++i) HIP_TRY(c, grow_zeroed(c, c->d_cplane[i], c->cap_px));
    return BF_OK;
}

int clear_planes(bf_ctx* c) {
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, hipMemsetAsync(c->d_plane[i], 0, c->cap_px * sizeof(unsigned long long), c->stream));
        if (c->d_cplane[i])
            HIP_TRY(c, hipMemsetAsync(c->d_cplane[i], 0, c->cap_px * sizeof(uint32_t), c->stream));
        if (c->d_ovf_bits[i])
            HIP_TRY(c, hipMemsetAsync(c->d_ovf_bits[i], 0, c->d_ovf_bits[i].size() * sizeof(uint32_t), c->stream));
    }
    c->planes_unknown = false;
    c->cur = 0;
    c->hst.hot.ovf_cnt[0] = c->hst.hot.ovf_cnt[1] = 0;
    return BF_OK;
}

// (a change of R or C clears planes and bitmaps: bf_set_cloud)
int ensure_ovf_bits(bf_ctx* c, int R, int C) {
    const int pitch = (C + 31) / 32 + 3;
    const size_t need = (size_t)R * (size_t)pitch;
    for (int i = 0; i < 2; ++i) {
        bool fresh;
        HIP_TRY(c, c->d_ovf_bits[i].grow(need, &fresh));
        if (fresh) c->planes_unknown = true;   // (fresh bitmaps: cleared with the planes below)
    }
    if (pitch != c->ovf_pitch) c->planes_unknown = true;   // (bits set under another row pitch mean other pixels)
    c->ovf_pitch = pitch;
    return BF_OK;
}

int ensure_second_set(bf_ctx* c) {
    const size_t ne = (size_t)c->cap_events;
    HIP_TRY(c, c->set[1].xy.grow(ne));
    HIP_TRY(c, c->set[1].t.grow(ne));
    HIP_TRY(c, c->set[1].p.grow(ne));
    for (int i = 0; i < 2; ++i) HIP_TRY(c, c->set[i].perm.grow(ne));
    return BF_OK;
}

int ensure_bin_buffers(bf_ctx* c, const BinGrid& g) {
    if (!c->bin_setup_done) {
        if (bin_kernel_setup() != 0) return fail(c, BF_ERR_HIP, "cannot raise the dynamic LDS limit");
        c->bin_setup_done = true;
    }
    const size_t ne = (size_t)c->cap_events;
    HIP_TRY(c, c->d_binid.grow(ne));
    HIP_TRY(c, grow_zeroed(c, c->d_armed, 16));
    const int rc = ensure_second_set(c);
    if (rc != BF_OK) return rc;
    const size_t nb = (size_t)g.nbins + 1;
    HIP_TRY(c, grow_zeroed(c, c->d_hist_cnt, kHistCopies * nb));
    HIP_TRY(c, c->d_bin_start.grow(nb));
    HIP_TRY(c, c->d_cursor.grow(nb));
    HIP_TRY(c, c->d_chdr.grow(nb * 580));   // event lists: 3 LR + 1 <= 577 key offsets per bin ((column zone, row) keys)
    const size_t need = (size_t)g.nbins * (size_t)g.LR * (size_t)g.L;
    HIP_TRY(c, c->d_slabs.grow(need));
    HIP_TRY(c, c->d_cidx.grow(need));
    return BF_OK;
}

// Iteration j of a run adds to margin plane b0 ^ (j & 1) and clears, bin by bin, what the lists say the previous executed launch
// left in the other one (flush_split); the host keeps track of which plane the lists describe.  The lists name pixels by their
// linear index, so what an earlier bin grid left behind is cleared with the earlier grid's list layout before the buffers change
// hands.
int margin_reset(bf_ctx* c) {
    if (c->m_unknown) {
        for (int i = 0; i < 2; ++i)
            if (c->d_mplane[i]) HIP_TRY(c, hipMemsetAsync(c->d_mplane[i], 0, c->cap_px * sizeof(unsigned long long), c->stream));
        if (c->d_mcount) HIP_TRY(c, hipMemsetAsync(c->d_mcount, 0, c->d_mcount.size() * sizeof(uint32_t), c->stream));
        c->m_unknown = false;
    } else if (c->m_dirty_plane >= 0) {
        launch_margin_clean(c->d_mplane[c->m_dirty_plane], c->d_mlist, c->d_mcount, c->m_nbins, c->m_cap, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    c->m_dirty_plane = -1;
    return BF_OK;
}
int ensure_margin_buffers(bf_ctx* c, const BinGrid& g) {
    const int mcap = g.LR * g.L - g.TSR * g.TS;
    if (c->m_unknown || g.nbins != c->m_nbins || mcap != c->m_cap) {
        int rc = margin_reset(c);
        if (rc != BF_OK) return rc;
    }
    for (int i = 0; i < 2; ++i) HIP_TRY(c, grow_zeroed(c, c->d_mplane[i], c->cap_px));
    HIP_TRY(c, grow_zeroed(c, c->d_mcount, (size_t)g.nbins));
    HIP_TRY(c, c->d_mlist.grow((size_t)g.nbins * (size_t)mcap));
    c->m_nbins = g.nbins;
    c->m_cap = mcap;
    return BF_OK;
}

int enqueue_rebin(bf_ctx* c, DevState* st, bool has_perm_at_start, const WarpParams* prewarp, bool fused, int launch_no) {
    ProfScope ps(c, 3);
    launch_rebin(ev_sets(c), has_perm_at_start ? 1 : 0, c->n, st, fused ? c->fgrid : c->grid, c->d_binid, c->d_hist_cnt,
                 c->d_bin_start, c->d_cursor, c->d_armed, prewarp, c->opt_bin_pack_limit, c->stream,
                 fused ? c->d_ftab : nullptr, fused ? lost_flag(c) + (launch_no + 2) % 3 : nullptr);   // (the last pass's word)
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

int flush_pending(bf_ctx* c) {
    if (!c->pending_warp) return BF_OK;
    launch_set_state(c->d_state, c->hst, c->stream);
    {
        ProfScope ps(c, 3);
        launch_warp_scatter(ws_args(c, c->cur, 0), true, false, true, c->stream);
    }
    c->pending_applied();
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// hipEventSynchronize spins here whatever the event's flags say (measured: one full core per waiting thread).
int wait_event_sleeping(bf_ctx* c, hipEvent_t ev) {
    bool waited = false;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) HIP_TRY(c, e);
        waited = true;
        struct timespec ts = {0, 20000};
        nanosleep(&ts, nullptr);
    }
    if (waited) (void)hipGetLastError();   // "not ready" is recorded as the thread's last error: it is not one
    return BF_OK;
}

int fold_stats(bf_ctx* c, const SliceStats* overwritten) {
    // (one folder at a time: with early staging the thread that uploads the NEXT slice into this record's slot folds the current
    // slice's statistics first if nobody has -- bf_upload.cpp: stage_early -- while bf_set_cloud may be doing the same)
    std::lock_guard<std::mutex> lk(c->stats_mu);
    if (c->stats_valid) return BF_OK;
    if (overwritten && (!c->uploaded || c->stats_src != overwritten)) return BF_OK;
    // (the records are in pinned host memory once k_prepare has completed: on the compute stream, or -- early staging -- on the
    // copy stream, usually long ago)
    if (c->stats_event) HIP_TRY(c, hipEventSynchronize(c->stats_event));
    else HIP_TRY(c, hipStreamSynchronize(c->stream));
    const SliceStats* src = c->stats_src ? c->stats_src : c->h_stats;
    SliceStats s = src[0];
    for (int k = 1; k < kPrepBlocks; ++k) {
        const SliceStats& q = src[k];
        if (q.xmin < s.xmin) s.xmin = q.xmin;
        if (q.xmax > s.xmax) s.xmax = q.xmax;
        if (q.ymin < s.ymin) s.ymin = q.ymin;
        if (q.ymax > s.ymax) s.ymax = q.ymax;
        if (q.tmin < s.tmin) s.tmin = q.tmin;
        if (q.tmax > s.tmax) s.tmax = q.tmax;
        s.tsum += q.tsum;
    }
    c->stats = s;
    c->stats_folded();
    return BF_OK;
}

int install_grouping(bf_ctx* c, const int32_t* src, hipMemcpyKind kind, int K) {
    c->grouping_dropped();
    HIP_TRY(c, c->d_group_id.grow((size_t)(c->n > 0 ? c->n : 1)));
    if (c->n > 0) {
        HIP_TRY(c, hipMemcpyAsync(c->d_group_id, src, (size_t)c->n * sizeof(int32_t), kind, c->stream));
        if (kind == hipMemcpyHostToDevice) HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the caller's array is free again)
    }
    c->grouping_held(K);
    return BF_OK;
}
