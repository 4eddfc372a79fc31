// flow_field.h -- the per-pixel flow field of a slice and its colour coding, EventFile::color_flow_img
// (event_file.h:318-350), on the host: the restatement of the rule include/bf_accel.h states at bf_flow_field /
// bf_color_flow_img, from per-event read-backs.  It serves two ends: a C-ABI library without those entries (the CPU
// stand-in the tests build) gets its flow frames from here, and it is the host path the device path is timed against.
// Also the Middlebury .flo container of --flow-field.
#ifndef BF_HOST_FLOW_FIELD_H
#define BF_HOST_FLOW_FIELD_H

#include <bf_accel.h>
#include <bf_flow_color.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack them -- the CPU stand-in the tests build --
// and the field is then built here from bf_writeout_events + bf_compute_uv)
extern "C" {
int bf_flow_field(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, int32_t *owner_out, double *u_out, double *v_out) __attribute__((weak));
int bf_color_flow_img(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *bgr_out, uint8_t *hs_out) __attribute__((weak));
int bf_flow_frame_create(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_flow_frame **out) __attribute__((weak));
int bf_flow_frame_destroy(bf_flow_frame *frame) __attribute__((weak));
int bf_flow_frame_render(bf_ctx *ctx, bf_flow_frame *frame, int32_t owner_rule, int64_t *ticket_out) __attribute__((weak));
int bf_flow_frame_wait(bf_ctx *ctx, bf_flow_frame *frame, int64_t ticket, const uint8_t **ppm, const uint8_t **avi, const float **flo) __attribute__((weak));
int bf_flow_frame_release(bf_flow_frame *frame, int64_t ticket) __attribute__((weak));
}

namespace bf {

struct FlowField {
    int rows = 0, cols = 0;        // RES_X x RES_Y; pixel (x, y) at x * cols + y
    std::vector<int32_t> owner;    // upload index of the owning event, -1 without one
    std::vector<double> u, v;      // its (best_u, best_v); 0 without one
    FlowField() {}
    FlowField(int r, int c) : rows(r), cols(c), owner((size_t)r * c, -1), u((size_t)r * c, 0.0), v((size_t)r * c, 0.0) {}
};

// The field from n events in upload order: positions, flow, noise flags (may be null).  owner_rule as in bf_flow_field.
inline FlowField flow_field_from_events(const double *pr_x, const double *pr_y, const double *u, const double *v, const uint8_t *noise,
                                        size_t n, int rows, int cols, int owner_rule) {
    FlowField f(rows, cols);
    for (size_t k = 0; k < n; ++k) {
        // the last assignment wins (event_file.h:337-338): walk towards the owning end
        const size_t i = owner_rule == BF_FLOW_FIRST_UPLOADED ? n - 1 - k : k;
        if (noise && noise[i]) continue;
        const int x = bf_double_to_int_x86(pr_x[i]), y = bf_double_to_int_x86(pr_y[i]);
        if ((x >= rows) || (x < 0) || (y >= cols) || (y < 0)) continue;
        const size_t at = (size_t)x * cols + y;
        f.owner[at] = (int32_t)i; f.u[at] = u[i]; f.v[at] = v[i];
    }
    return f;
}

// ... from the read-backs of a context that holds the slice (n events; `noise`: their flags as uploaded, or null).
// Returns the C-ABI's return code.
inline int flow_field_from_readbacks(bf_ctx *ctx, size_t n, const uint8_t *noise, int rows, int cols, int owner_rule, FlowField &out) {
    std::vector<double> px(n), py(n), u(n), v(n);
    if (n > 0) {
        int rc = bf_writeout_events(ctx, px.data(), py.data(), nullptr, nullptr);
        if (rc >= 0) rc = bf_compute_uv(ctx, u.data(), v.data());
        if (rc < 0) return rc;
    }
    out = flow_field_from_events(px.data(), py.data(), u.data(), v.data(), noise, n, rows, cols, owner_rule);
    return BF_OK;
}

// EventFile::color_flow_img of a field: rows x cols x 3 bytes, B G R; white without an event.  hs (may be null): the H and S
// bytes before the conversion.
inline std::vector<uint8_t> color_flow_img_of(const FlowField &f, std::vector<uint8_t> *hs = nullptr) {
    const size_t px = (size_t)f.rows * f.cols;
    std::vector<uint8_t> bgr(px * 3);
    if (hs) hs->assign(px * 2, 0);
    for (size_t i = 0; i < px; ++i) {
        int H = 0, S = 0;
        if (f.owner[i] >= 0) bf_flow_hs(f.u[i], f.v[i], &H, &S);
        if (hs) { (*hs)[2 * i] = (uint8_t)H; (*hs)[2 * i + 1] = (uint8_t)S; }
        bf_hsv_to_bgr_u8(H, S, 255, &bgr[3 * i]);
    }
    return bgr;
}

// The payload of a Middlebury .flo file of the field: per pixel, row-major, float32 horizontal = v (columns), vertical = u
// (rows) -- the swap -o makes (event_file.h:274-275) --, 1e9 in both without an event.
inline std::vector<float> flo_payload(const FlowField &f) {
    const size_t px = (size_t)f.rows * f.cols;
    std::vector<float> out(2 * px);
    for (size_t i = 0; i < px; ++i) {
        const bool has = f.owner[i] >= 0;
        out[2 * i] = has ? (float)f.v[i] : 1e9f;
        out[2 * i + 1] = has ? (float)f.u[i] : 1e9f;
    }
    return out;
}

// .flo: float32 202021.25 ("PIEH"), int32 width = cols, int32 height = rows, then the payload (little endian)
inline bool write_flo(const std::string &path, int rows, int cols, const float *payload) {
    FILE *fp = std::fopen(path.c_str(), "wb");
    if (!fp) return false;
    const float tag = 202021.25f;
    const int32_t wh[2] = {cols, rows};
    const size_t n = (size_t)rows * (size_t)cols * 2;
    const bool w = std::fwrite(&tag, 4, 1, fp) == 1 && std::fwrite(wh, 4, 2, fp) == 2 && std::fwrite(payload, 4, n, fp) == n;
    return std::fclose(fp) == 0 && w;
}

}  // namespace bf

#endif  // BF_HOST_FLOW_FIELD_H
