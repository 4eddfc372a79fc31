// bf_segment_abi.cpp -- C-ABI of the moving-object segmentation (include/bf_accel.h; kernels in bf_segment.hip): bf_segment on the
// live window's time image, bf_segment_get for what it left on the device, bf_label_image for the labelling alone.
#include "bf_ctx.h"

namespace {

// The planes of an R x C image and the scalars; sz and the scalars zeroed on the stream.
int seg_prepare(bf_ctx* c, size_t P) {
    HIP_TRY(c, c->d_seg_lab.grow(P));
    HIP_TRY(c, c->d_seg_sz.grow(P));
    HIP_TRY(c, c->d_seg_nid.grow(P));
    HIP_TRY(c, c->d_seg_scan.grow((size_t)seg_rank_blocks((long long)P)));
    HIP_TRY(c, c->d_seg_dev.grow(1));
    HIP_TRY(c, c->h_seg_dev.grow(1));
    HIP_TRY(c, hipMemsetAsync(c->d_seg_sz, 0, P * sizeof(int32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_seg_dev, 0, sizeof(SegDev), c->stream));
    return BF_OK;
}

// Steps 3 to 5 on the device: labels in d_seg_lab, the table's seg_K rows in d_seg_table, the scalars in h_seg_dev.  One wait
// in the middle: the table is sized from the number of components kept.
int seg_components(bf_ctx* c, const SegMask& m, int R, int C, int connectivity, int min_pixels, const float* T) {
    const long long P = (long long)R * C;
    launch_seg_label(m, R, C, connectivity, c->d_seg_lab, c->d_seg_sz, c->d_seg_dev, c->stream);
    launch_seg_rank(c->d_seg_lab, c->d_seg_sz, c->d_seg_nid, P, min_pixels, c->d_seg_scan, c->d_seg_dev, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_seg_dev, c->d_seg_dev, sizeof(SegDev), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int K = (int)c->h_seg_dev[0].kept;
    HIP_TRY(c, c->d_seg_table.grow((size_t)(K > 0 ? K : 1)));
    launch_seg_table(c->d_seg_lab, c->d_seg_nid, T, c->d_seg_table, K, R, C, c->stream);
    HIP_TRY(c, hipGetLastError());
    c->seg_K = K;
    return BF_OK;
}

bool seg_threshold(double s, long long* q, int* use) {
    if (s != s || std::isinf(s)) return false;
    *use = s >= 0.0;
    *q = 0;
    if (*use) {
        const double v = std::floor(s * 1073741824.0);
        if (v >= 9.0e18) return false;
        *q = (long long)v;
    }
    return true;
}

}  // namespace

extern "C" {

void bf_segment_opts_default(bf_segment_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->above_s = -1.0;
    o->below_s = -1.0;
    o->min_count = 1;
    o->connectivity = 8;
    o->min_pixels = 1;
}

int bf_segment(bf_ctx* c, const bf_segment_opts* opts, bf_segment_info* info) {
    if (!c) return BF_ERR_ARG;
    bf_segment_opts o;
    bf_segment_opts_default(&o);
    if (opts) o = *opts;
    SegMask m;
    memset(&m, 0, sizeof(m));
    if (!seg_threshold(o.above_s, &m.A, &m.use_a) || !seg_threshold(o.below_s, &m.B, &m.use_b))
        return fail(c, BF_ERR_ARG, "bf_segment: a threshold is NaN, infinite or beyond the int64 range");
    if (o.min_count < 1 || o.min_pixels < 1 || (o.connectivity != 4 && o.connectivity != 8))
        return fail(c, BF_ERR_ARG, "bf_segment: min_count %d, min_pixels %d (both >= 1), connectivity %d (4 or 8)", o.min_count,
                    o.min_pixels, o.connectivity);
    c->segmentation_dropped();
    int rc = ctx_time_img_pass(c, "bf_segment");
    if (rc != BF_OK) return rc;
    const int R = c->win.scale_img_x, C = c->win.scale_img_y;
    const size_t P = (size_t)R * (size_t)C;
    if (P > (size_t)INT_MAX) return fail(c, BF_ERR_CAPACITY, "bf_segment: more than 2^31 pixels");
    rc = seg_prepare(c, P);
    if (rc != BF_OK) return rc;
    launch_seg_mean(c->d_time, c->d_count, (long long)P, c->d_seg_dev, c->stream);
    m.T = c->d_time;
    m.cnt = c->d_count;
    m.min_count = (uint32_t)o.min_count;
    rc = seg_components(c, m, R, C, o.connectivity, o.min_pixels, c->d_time);
    if (rc != BF_OK) return rc;
    if (c->n > 0) {
        HIP_TRY(c, c->d_seg_cl.grow((size_t)c->n));
        if (c->all_noise) {   // (the time image skipped every event)
            HIP_TRY(c, hipMemsetAsync(c->d_seg_cl, 0xff, (size_t)c->n * sizeof(int32_t), c->stream));
        } else {
            const bf_ctx::EvSet& e = c->set[c->cs];
            const HotState& h = c->hst.hot;
            SegEvents ev;
            ev.xy = e.xy; ev.p = e.p;
            ev.noise = c->has_noise ? c->d_noise.get() : nullptr;   // (a slice with flags is never re-binned: slot == upload index)
            ev.perm = c->has_perm ? e.perm.get() : nullptr;
            ev.n = c->n;
            ev.scale = h.scale; ev.x_sh = h.x_sh; ev.y_sh = h.y_sh; ev.wsx = h.wsx; ev.wsy = h.wsy; ev.C = C;
            launch_seg_events(ev, c->d_seg_lab, c->d_seg_cl, c->seg_K > 0 ? c->d_seg_table.get() : nullptr, c->stream);
            HIP_TRY(c, hipGetLastError());
        }
    }
    c->segmentation_held();
    if (info) {
        const SegDev& d = c->h_seg_dev[0];
        memset(info, 0, sizeof(*info));
        info->rows = R; info->cols = C;
        info->n1 = (int64_t)d.n1; info->q_sum = d.q_sum; info->q_mean = d.mu;
        info->foreground_pixels = (int32_t)d.fg;
        info->components_found = (int32_t)d.found;
        info->components = (int32_t)d.kept;
    }
    return BF_OK;
}

int bf_segment_get(bf_ctx* c, int32_t* labels_out, bf_component* comps_out, int32_t comps_cap, int32_t* cl_id_out) {
    if (!c) return BF_ERR_ARG;
    if (!c->seg_valid || c->pending_warp || !c->have_window)
        return fail(c, BF_ERR_STATE, "bf_segment_get: no segmentation of the current window is held");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t P = (size_t)c->win.scale_img_x * (size_t)c->win.scale_img_y;
    if (labels_out) HIP_TRY(c, hipMemcpyAsync(labels_out, c->d_seg_lab, P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    const int rows = comps_cap < c->seg_K ? comps_cap : c->seg_K;
    if (comps_out && rows > 0)
        HIP_TRY(c, hipMemcpyAsync(comps_out, c->d_seg_table, (size_t)rows * sizeof(bf_component), hipMemcpyDeviceToHost, c->stream));
    if (cl_id_out && c->n > 0)
        HIP_TRY(c, hipMemcpyAsync(cl_id_out, c->d_seg_cl, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

int bf_label_image(bf_ctx* c, const uint8_t* mask, int32_t rows, int32_t cols, int32_t connectivity, int32_t min_pixels,
                   int32_t* labels_out, bf_component* comps_out, int32_t comps_cap, int32_t* components_out) {
    if (!c) return BF_ERR_ARG;
    if (!mask || rows <= 0 || cols <= 0) return fail(c, BF_ERR_ARG, "bf_label_image: bad image");
    if (min_pixels < 1 || (connectivity != 4 && connectivity != 8))
        return fail(c, BF_ERR_ARG, "bf_label_image: min_pixels %d (>= 1), connectivity %d (4 or 8)", min_pixels, connectivity);
    const size_t P = (size_t)rows * (size_t)cols;
    if (P > c->cap_px || P > (size_t)INT_MAX) return fail(c, BF_ERR_CAPACITY, "image %d x %d exceeds capacity", rows, cols);
    HIP_TRY(c, hipSetDevice(c->device));
    c->segmentation_dropped();   // (the planes change hands)
    int rc = seg_prepare(c, P);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, c->d_seg_mask.grow(P));
    HIP_TRY(c, hipMemcpyAsync(c->d_seg_mask, mask, P, hipMemcpyHostToDevice, c->stream));
    SegMask m;
    memset(&m, 0, sizeof(m));
    m.mask = c->d_seg_mask;
    rc = seg_components(c, m, rows, cols, connectivity, min_pixels, nullptr);
    if (rc != BF_OK) return rc;
    if (labels_out) HIP_TRY(c, hipMemcpyAsync(labels_out, c->d_seg_lab, P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    const int n = comps_cap < c->seg_K ? comps_cap : c->seg_K;
    if (comps_out && n > 0)
        HIP_TRY(c, hipMemcpyAsync(comps_out, c->d_seg_table, (size_t)n * sizeof(bf_component), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (components_out) *components_out = c->seg_K;
    return BF_OK;
}

}  // extern "C"
