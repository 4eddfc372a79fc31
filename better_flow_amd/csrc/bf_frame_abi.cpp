// bf_frame_abi.cpp -- C-ABI of the device-composed frame of --img / --video (include/bf_accel.h, "per-slice frames on the
// device"): four tiles rendered on the context stream (render_projection_img, bf_local_abi.cpp; render_color_time_img, below), the
// mosaic composed by k_frame_compose (bf_frame.hip) straight into a pinned, device-mapped slot in the byte layout of the file,
// and the ticket / wait / release calls around the slots.  The colour-coded time image on its own is bf_color_time_img.
#include "bf_ctx.h"

#include <cmath>
#include <vector>

struct bf_frame {
    int device = 0;
    int res_x = 0, res_y = 0, layouts = 0, slots = 0;
    int R = 0, C = 0, CR = 0, CC = 0;        // tile (3 res_x x 3 res_y), colour source (R + 3 x C + 3)
    int stride = 0;                          // AVI row bytes
    size_t ppm_bytes = 0, avi_bytes = 0;     // one frame per layout
    DevArray<uint8_t> gray[2], colour[2];    // compensated (0) / raw (1) tiles: one set, reused in stream order
    DevArray<int32_t> taps;                  // row0[R] row1[R] col0[C] col1[C]
    DevArray<float> weights;                 // row_w[R] col_w[C]
    MappedArray<uint8_t> ppm, avi;           // slots x one frame
    std::vector<Event> done;                 // per slot: its render and compose have run
    // host bookkeeping, under mu
    std::mutex mu;
    long long issued = 0;
    std::vector<long long> ticket;           // per slot: the ticket it holds, or -1 (free)
    hipStream_t last_stream = nullptr;       // the stream of the newest render, and its slot's event
    hipEvent_t last = nullptr;
};

extern "C" {

// EventFile::color_time_img (event_file.h:649-747) of the live slice into d_bgr ((scale res_x + scale) x (scale res_y + scale)
// x 3 bytes), enqueued on the context stream.  Arguments checked by the callers (scale already mapped from 0 to 11).
int render_color_time_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* d_bgr) {
    ColorGeom g;
    memset(&g, 0, sizeof(g));
    g.scale = scale; g.show_final = show_final ? 1 : 0;
    g.mx = scale * res_x; g.my = scale * res_y;
    g.R = g.mx + scale; g.C = g.my + scale;
    const size_t px = (size_t)g.R * (size_t)g.C;
    int rc = flush_pending(c);   // a pending bf_set_model warp moves the events first
    if (rc != BF_OK) return rc;
    if (c->n > 0) {
        rc = fold_stats(c);
        if (rc != BF_OK) return rc;
        g.t_min = c->stats.tmin;                                             // :659-662: t_max starts at 0
        g.t_range = std::max<long long>(c->stats.tmax, 0) - g.t_min;
    }
    g.x_shift = -double(res_x / 2) * double(scale) + double(g.mx) / 2.0;     // :677-678 with x_min = 0, x_max = RES_X
    g.y_shift = -double(res_y / 2) * double(scale) + double(g.my) / 2.0;
    HIP_TRY(c, c->d_col_planes.grow(c->cap_px * 20));   // 2 x i64 sums + u32 count per pixel
    HIP_TRY(c, hipMemsetAsync(c->d_col_planes, 0, px * 20, c->stream));
    const bf_ctx::EvSet& e = c->set[c->cs];
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(c->d_col_planes.get());
    launch_color_time(e.xy, e.t, e.p, c->has_noise ? c->d_noise : nullptr, c->n, g,
                      reinterpret_cast<uint32_t*>(sums + 2 * px), sums, sums + px, d_bgr, c->stream);
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

int bf_color_time_img(bf_ctx* c, int32_t scale, int32_t res_x, int32_t res_y, int32_t show_final, uint8_t* bgr_out) {
    if (!c || !bgr_out) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_color_time_img before bf_upload_events");
    if (scale == 0) scale = 11;   // event_file.h:650
    if (scale < 1 || scale > 15) return fail(c, BF_ERR_ARG, "scale must be in 1..15 (got %d)", scale);
    if (res_x < 1 || res_y < 1) return fail(c, BF_ERR_ARG, "bad sensor size");
    const size_t px = (size_t)(scale * res_x + scale) * (size_t)(scale * res_y + scale);
    if (px > c->cap_px) return fail(c, BF_ERR_CAPACITY, "image %d x %d exceeds the image capacity", scale * res_x + scale, scale * res_y + scale);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_col_img.grow(c->cap_px * 3));
    int rc = render_color_time_img(c, scale, res_x, res_y, show_final, c->d_col_img);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(bgr_out, c->d_col_img, px * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

}  // extern "C"

namespace {

int frame_slot(const bf_frame* f, long long t) {   // the slot holding ticket t, or -1
    if (t < 0) return -1;
    for (int s = 0; s < f->slots; ++s)
        if (f->ticket[s] == t) return s;
    return -1;
}

// frame_writer.h resize_bilinear's source taps for `dst` samples of `src`: (d + 0.5) * (src / dst) - 0.5, clamped at 0, floor,
// the upper tap clamped to the last sample (compiled with -ffp-contract=off, as the host code is without FMA)
void bilinear_taps(int src, int dst, int32_t* i0, int32_t* i1, float* w) {
    const float sc = (float)src / (float)dst;
    for (int d = 0; d < dst; ++d) {
        float x = ((float)d + 0.5f) * sc - 0.5f;
        if (x < 0) x = 0;
        int i = (int)std::floor(x);
        if (i > src - 1) i = src - 1;
        i0[d] = i; i1[d] = i + 1 < src ? i + 1 : src - 1; w[d] = x - (float)i;
    }
}

int create_failed(bf_ctx* c, hipError_t err, const char* what) {
    return fail(c, err == hipErrorOutOfMemory ? BF_ERR_CAPACITY : BF_ERR_HIP, "bf_frame_create: %s: %s", what, hipGetErrorString(err));
}

}  // namespace

extern "C" {

int bf_frame_create(bf_ctx* c, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_frame** out) {
    if (!c || !out) return BF_ERR_ARG;
    *out = nullptr;
    if (res_x < 2 || res_y < 2 || res_x > 16384 || res_y > 16384 || slots < 1 || slots > 64 || layouts < 1 ||
        (layouts & ~(BF_FRAME_PPM | BF_FRAME_AVI)) != 0)
        return fail(c, BF_ERR_ARG, "bf_frame_create: bad sensor %d x %d, slot count %d or layouts %d", res_x, res_y, slots, layouts);
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<bf_frame> f(new (std::nothrow) bf_frame);   // (a failure below frees what was made)
    if (!f) return fail(c, BF_ERR_CAPACITY, "bf_frame_create: out of host memory");
    f->device = c->device;
    f->res_x = res_x; f->res_y = res_y; f->layouts = layouts; f->slots = slots;
    f->R = 3 * res_x; f->C = 3 * res_y; f->CR = f->R + 3; f->CC = f->C + 3;   // frames are rendered at scale 3 (dvs_flow.h)
    f->stride = (2 * f->C * 3 + 3) & ~3;
    f->ppm_bytes = (size_t)(2 * f->R) * (size_t)(2 * f->C) * 3;
    f->avi_bytes = (size_t)f->stride * (size_t)(2 * f->R);
    hipError_t err;
    for (int i = 0; i < 2; ++i) {
        if ((err = f->gray[i].grow((size_t)f->R * f->C)) != hipSuccess) return create_failed(c, err, "tiles");
        if ((err = f->colour[i].grow((size_t)f->CR * f->CC * 3)) != hipSuccess) return create_failed(c, err, "tiles");
    }
    std::vector<int32_t> taps(2 * (size_t)f->R + 2 * (size_t)f->C);
    std::vector<float> w((size_t)f->R + f->C);
    bilinear_taps(f->CR, f->R, taps.data(), taps.data() + f->R, w.data());
    bilinear_taps(f->CC, f->C, taps.data() + 2 * f->R, taps.data() + 2 * f->R + f->C, w.data() + f->R);
    if ((err = f->taps.grow(taps.size())) != hipSuccess) return create_failed(c, err, "taps");
    if ((err = f->weights.grow(w.size())) != hipSuccess) return create_failed(c, err, "taps");
    HIP_TRY(c, hipMemcpy(f->taps, taps.data(), taps.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(f->weights, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    // (pinned and mapped: k_frame_compose stores the payloads straight into them)
    if ((layouts & BF_FRAME_PPM) && (err = f->ppm.grow(f->ppm_bytes * (size_t)slots)) != hipSuccess) return create_failed(c, err, "PPM slots");
    if ((layouts & BF_FRAME_AVI) && (err = f->avi.grow(f->avi_bytes * (size_t)slots)) != hipSuccess) return create_failed(c, err, "AVI slots");
    f->done.resize((size_t)slots);
    for (Event& e : f->done)
        if ((err = e.create(hipEventDisableTiming)) != hipSuccess) return create_failed(c, err, "events");
    f->ticket.assign((size_t)slots, -1);
    *out = f.release();
    return BF_OK;
}

int bf_frame_destroy(bf_frame* f) {
    if (!f) return BF_ERR_ARG;
    (void)hipSetDevice(f->device);
    for (int s = 0; s < f->slots; ++s)
        if (f->ticket[s] >= 0) (void)hipEventSynchronize(f->done[s]);   // renders in flight write into the slots
    delete f;
    return BF_OK;
}

int bf_frame_render(bf_ctx* c, bf_frame* f, int64_t* ticket_out) {
    if (!c || !f || !ticket_out) return BF_ERR_ARG;
    *ticket_out = -1;
    if (c->device != f->device) return fail(c, BF_ERR_ARG, "bf_frame_render: frame state on device %d, context on device %d", f->device, c->device);
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_frame_render before bf_upload_events");
    if ((size_t)f->CR * (size_t)f->CC > c->cap_px)
        return fail(c, BF_ERR_CAPACITY, "bf_frame_render: the context's image capacity is below %d x %d (the scale-3 colour tile)", f->CR, f->CC);
    std::lock_guard<std::mutex> g(f->mu);
    int slot = -1;
    for (int s = 0; s < f->slots && slot < 0; ++s)
        if (f->ticket[s] < 0) slot = s;
    if (slot < 0) return fail(c, BF_ERR_CAPACITY, "bf_frame_render: all %d frame slots are taken: release one first", f->slots);
    HIP_TRY(c, hipSetDevice(c->device));
    // the tiles are shared by the slots: a render from another stream goes after the newest one
    if (f->last && f->last_stream != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, f->last, 0));
    int rc;
    for (int i = 0; i < 2; ++i) {   // DVS_flow::render_frame: the compensated tiles (show_final) on top, the raw ones below
        const int show_final = i == 0 ? 1 : 0;
        if ((rc = render_projection_img(c, 3, f->res_x, f->res_y, show_final, f->gray[i])) != BF_OK) return rc;
        if ((rc = render_color_time_img(c, 3, f->res_x, f->res_y, show_final, f->colour[i])) != BF_OK) return rc;
    }
    bf::FrameCompose a;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < 2; ++i) { a.gray[i] = f->gray[i]; a.colour[i] = f->colour[i]; }
    a.R = f->R; a.C = f->C; a.CR = f->CR; a.CC = f->CC;
    a.row0 = f->taps; a.row1 = f->taps + f->R; a.col0 = f->taps + 2 * f->R; a.col1 = f->taps + 2 * f->R + f->C;
    a.row_w = f->weights; a.col_w = f->weights + f->R;
    a.ppm = (f->layouts & BF_FRAME_PPM) ? f->ppm + (size_t)slot * f->ppm_bytes : nullptr;
    a.avi = (f->layouts & BF_FRAME_AVI) ? f->avi + (size_t)slot * f->avi_bytes : nullptr;
    a.ppm_dwords = (long long)(f->ppm_bytes / 4);
    a.avi_dwords = (long long)(f->avi_bytes / 4);
    a.stride = f->stride;
    bf::launch_frame_compose(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(f->done[slot], c->stream));
    f->last = f->done[slot];
    f->last_stream = c->stream;
    f->ticket[slot] = f->issued;
    *ticket_out = f->issued++;
    return BF_OK;
}

int bf_frame_wait(bf_ctx* c, bf_frame* f, int64_t ticket, const uint8_t** ppm, const uint8_t** avi) {
    if (!c || !f) return BF_ERR_ARG;
    int slot;
    hipEvent_t done;
    {
        std::lock_guard<std::mutex> g(f->mu);
        slot = frame_slot(f, ticket);
        if (slot < 0) return fail(c, BF_ERR_ARG, "bf_frame_wait: ticket %lld is not in flight (released, or never issued)", (long long)ticket);
        done = f->done[slot];
    }
    HIP_TRY(c, hipSetDevice(f->device));
    HIP_TRY(c, hipEventSynchronize(done));
    if (ppm) *ppm = (f->layouts & BF_FRAME_PPM) ? f->ppm + (size_t)slot * f->ppm_bytes : nullptr;
    if (avi) *avi = (f->layouts & BF_FRAME_AVI) ? f->avi + (size_t)slot * f->avi_bytes : nullptr;
    return BF_OK;
}

int bf_frame_release(bf_frame* f, int64_t ticket) {
    if (!f) return BF_ERR_ARG;
    std::lock_guard<std::mutex> g(f->mu);
    const int slot = frame_slot(f, ticket);
    if (slot < 0) return BF_ERR_ARG;
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->done[slot]);   // (released unwaited: the compose must not write into a slot given out again)
    f->ticket[slot] = -1;
    return BF_OK;
}

int bf_render_frame(bf_ctx* c, int32_t res_x, int32_t res_y, uint8_t* ppm_out, uint8_t* avi_out) {
    if (!c || (!ppm_out && !avi_out)) return BF_ERR_ARG;
    bf_frame* f = nullptr;
    int rc = bf_frame_create(c, res_x, res_y, 1, (ppm_out ? BF_FRAME_PPM : 0) | (avi_out ? BF_FRAME_AVI : 0), &f);
    if (rc != BF_OK) return rc;
    int64_t t = -1;
    const uint8_t *ppm = nullptr, *avi = nullptr;
    if ((rc = bf_frame_render(c, f, &t)) == BF_OK && (rc = bf_frame_wait(c, f, t, &ppm, &avi)) == BF_OK) {
        if (ppm_out) std::memcpy(ppm_out, ppm, f->ppm_bytes);
        if (avi_out) std::memcpy(avi_out, avi, f->avi_bytes);
    }
    (void)bf_frame_destroy(f);
    return rc;
}

}  // extern "C"
