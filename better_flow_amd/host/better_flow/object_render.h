// object_render.h -- bf::ObjectRenderer: the picture and the score of a grouping (include/bf_accel.h, "event groups: projection";
// DESIGN section 17): the slice with every event warped by its own group's model -- per pixel the event count, the owning group
// and its colour, per group and overall the integer moments of that image -- and its writers.
//
// Two paths with the same bytes (integers throughout, so equal, not close):
//   project()       bf_project_groups on the context's uploaded slice and held grouping: two kernels and a box sum;
//   project_host()  the same definition on host arrays (slice, ids, models), against any C-ABI: bf::MotionAssigner's host pixel
//                   code gives the events' pixels under each model; planes, box sums, owner, colour and moments are done here.
// render() uploads a slice, holds `ids` as its grouping and takes project() when the linked library has the entry.
#ifndef BF_HOST_OBJECT_RENDER_H
#define BF_HOST_OBJECT_RENDER_H

#include <better_flow/motion_assign.h>

#include <cstdio>
#include <string>

// (weak, as in motion_assign.h)
extern "C" {
int bf_project_groups(bf_ctx *ctx, const bf_project_opts *opts, const bf_model *models, int32_t n_models, uint32_t *count_out,
                      int32_t *label_out, uint8_t *bgr_out, bf_group_score *scores_out, bf_project_info *info) __attribute__((weak));
}

namespace bf {

class ObjectRenderer {
  public:
    bf_project_opts opts;                 // scale, sensor, margin, gain
    // what a projection leaves: R x C counts, labels (-1: no event) and B, G, R bytes, K scores, the info
    std::vector<uint32_t> count;
    std::vector<int32_t> label;
    std::vector<uint8_t> bgr;
    std::vector<bf_group_score> scores;
    bf_project_info info;
    int rows = 0, cols = 0;               // of the three images (info.rows / info.cols are zero for an empty slice)

    ObjectRenderer() : opts(), info() {
        opts.scale = 3;
        opts.sensor_res_x = 180; opts.sensor_res_y = 240;
        opts.gain = 8;
    }

    static bool device_available() { return bf_project_groups != nullptr; }

    // The context's uploaded slice and held grouping (K = models.size() groups) under `models`, on the device.
    int project(bf_ctx *ctx, const std::vector<bf_model> &models) {
        if (!device_available()) return BF_ERR_STATE;
        if (!valid((int)models.size())) return BF_ERR_ARG;
        if (!size_outputs(models.size())) return BF_ERR_CAPACITY;
        return bf_project_groups(ctx, &opts, models.data(), (int32_t)models.size(), count.data(), label.data(), bgr.data(),
                                 scores.data(), &info);
    }

    // The same on host arrays: uploads the slice (the context's held grouping is forgotten, as by every upload).
    int project_host(bf_ctx *ctx, const Slice &s, const std::vector<int32_t> &ids, const std::vector<bf_model> &models) {
        const int K = (int)models.size();
        if (!valid(K) || ids.size() != s.n) return BF_ERR_ARG;
        for (size_t i = 0; i < s.n; ++i)
            if (ids[i] < -1 || ids[i] >= K) return BF_ERR_ARG;
        if (!size_outputs((size_t)K)) return BF_ERR_CAPACITY;
        const MotionAssigner::HostWindow w = MotionAssigner::host_window(opts.scale, opts.sensor_res_x, opts.sensor_res_y, opts.margin);
        const size_t n = s.n, P = (size_t)w.R * (size_t)w.C;
        std::fill(label.begin(), label.end(), -1);
        if (n == 0) return BF_OK;   // N == 0 everywhere, scores and info zero
        int rc = bf_upload_events(ctx, s.fr_x, s.fr_y, s.t_ns, nullptr, (int64_t)n);
        if (rc < 0) return rc;
        static const uint8_t palette[BF_PROJECT_PALETTE_SIZE][3] = BF_PROJECT_PALETTE;
        std::vector<uint32_t> V(P), B(P), row(P), best(P, 0u);
        std::vector<double> px(n), py(n);
        std::vector<int32_t> pix(n);
        int64_t outside = 0;
        for (int k = 0; k < K; ++k) {
            bf_group_score &g = scores[(size_t)k];
            for (size_t i = 0; i < n; ++i) g.events += ids[i] == k;
            if (g.events == 0) continue;   // an empty plane adds nothing to any pixel
            rc = MotionAssigner::host_pixels(ctx, models[(size_t)k], w, opts.sensor_res_x, opts.sensor_res_y, px, py, pix);
            if (rc < 0) return rc;
            std::fill(V.begin(), V.end(), 0u);
            for (size_t i = 0; i < n; ++i)
                if (ids[i] == k && pix[i] >= 0) { ++V[(size_t)pix[i]]; ++g.inside; }
            outside += g.events - g.inside;
            const std::vector<uint32_t> *S = &V;
            if (w.s > 1) {
                MotionAssigner::host_box_sum(V, w, row, B);
                S = &B;
            }
            for (size_t p = 0; p < P; ++p) {
                const uint32_t b = (*S)[p];
                if (!b) continue;
                ++g.pixels_hit;
                if ((int32_t)b > g.max) g.max = (int32_t)b;
                g.sum_sq += (uint64_t)b * b;
                count[p] += b;
                if (b > best[p]) { best[p] = b; label[p] = k; }   // (strictly larger: ties stay with the smaller k)
            }
        }
        for (size_t p = 0; p < P; ++p) {
            const uint32_t N = count[p];
            if (!N) continue;
            ++info.pixels;
            info.sum += N;
            info.sum_sq += (uint64_t)N * N;
            const int32_t k = label[p];
            ++scores[(size_t)k].pixels_owned;
            const uint64_t x = (uint64_t)best[p] * (uint64_t)opts.gain;
            const uint32_t level = x > 255u ? 255u : (uint32_t)x;
            for (int c = 0; c < 3; ++c) bgr[3 * p + c] = (uint8_t)((uint32_t)palette[k % BF_PROJECT_PALETTE_SIZE][c] * level / 255u);
        }
        info.models = K;
        info.rows = w.R; info.cols = w.C;
        for (size_t i = 0; i < n; ++i) info.unassigned += ids[i] == -1;
        info.outside = (int32_t)outside;
        return BF_OK;
    }

    // Uploads the slice, holds `ids` (-1 .. K-1, upload order) as its grouping and projects it under `models`.
    int render(bf_ctx *ctx, const Slice &s, const std::vector<int32_t> &ids, const std::vector<bf_model> &models) {
        if (!device_available() || !bf_set_groups) return project_host(ctx, s, ids, models);
        const int rc = hold_grouping(ctx, s, ids, models.size());
        return rc < 0 ? rc : project(ctx, models);
    }

    // The colour image as a binary PPM (R, G, B), the labels as a 16-bit PGM (id + 1, 0: no event; the format of
    // segments_N.pgm), the scores as text: per group "id events inside pixels_hit pixels_owned max sum_sq", then
    // "info models rows cols unassigned outside pixels sum sum_sq".
    bool write_ppm(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        std::fprintf(f, "P6\n%d %d\n255\n", cols, rows);
        std::vector<uint8_t> row((size_t)cols * 3);
        for (int r = 0; r < rows; ++r) {
            for (int c = 0; c < cols; ++c) {
                const uint8_t *p = &bgr[3 * ((size_t)r * (size_t)cols + (size_t)c)];
                row[3 * (size_t)c] = p[2]; row[3 * (size_t)c + 1] = p[1]; row[3 * (size_t)c + 2] = p[0];
            }
            std::fwrite(row.data(), 1, row.size(), f);
        }
        return std::fclose(f) == 0;
    }
    bool write_label_pgm(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        std::fprintf(f, "P5\n%d %d\n65535\n", cols, rows);
        std::vector<uint8_t> row((size_t)cols * 2);
        for (int r = 0; r < rows; ++r) {
            for (int c = 0; c < cols; ++c) {
                const int32_t id = label[(size_t)r * (size_t)cols + (size_t)c];
                const uint32_t v = id < 0 ? 0u : (uint32_t)id + 1u;
                row[2 * (size_t)c] = (uint8_t)(v >> 8);
                row[2 * (size_t)c + 1] = (uint8_t)(v & 0xffu);
            }
            std::fwrite(row.data(), 1, row.size(), f);
        }
        return std::fclose(f) == 0;
    }
    bool write_scores(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        for (size_t k = 0; k < scores.size(); ++k) {
            const bf_group_score &g = scores[k];
            std::fprintf(f, "%zu %d %d %d %d %d %llu\n", k, (int)g.events, (int)g.inside, (int)g.pixels_hit, (int)g.pixels_owned, (int)g.max,
                         (unsigned long long)g.sum_sq);
        }
        std::fprintf(f, "info %d %d %d %d %d %d %llu %llu\n", (int)info.models, (int)info.rows, (int)info.cols, (int)info.unassigned,
                     (int)info.outside, (int)info.pixels, (unsigned long long)info.sum, (unsigned long long)info.sum_sq);
        return std::fclose(f) == 0;
    }

  private:
    bool valid(int K) const {   // bf_project_groups' argument checks
        return MotionAssigner::host_plane_opts_valid(opts.scale, opts.sensor_res_x, opts.sensor_res_y, opts.margin, K) && opts.gain >= 1;
    }
    // Zeroed outputs of the call's window; false when K planes of it exceed the entry's 2^27 words.
    bool size_outputs(size_t K) {
        const MotionAssigner::HostWindow w = MotionAssigner::host_window(opts.scale, opts.sensor_res_x, opts.sensor_res_y, opts.margin);
        if (!MotionAssigner::host_planes_fit((int)K, w)) return false;
        rows = w.R; cols = w.C;
        const size_t P = (size_t)w.R * (size_t)w.C;
        count.assign(P, 0u);
        label.assign(P, 0);
        bgr.assign(3 * P, 0);
        bf_group_score zero;
        std::memset(&zero, 0, sizeof(zero));
        scores.assign(K, zero);
        std::memset(&info, 0, sizeof(info));
        return true;
    }
};

}  // namespace bf

#endif  // BF_HOST_OBJECT_RENDER_H
