// clustering.h -- moving-object segmentation of a compensated slice on the host side: bf::Segmenter and the writers of its two
// files.  It takes the place of the reference's clustering.h, whose Cluster (an id and a merge, operator+=) is a union-find
// without a user, and fills in the vocabulary Event carries (cl, cl_id = -1, visited: event.h:23-34) WITHOUT touching Event:
// the ids come back as a vector parallel to the events.  The definitions are include/bf_accel.h's ("moving-object
// segmentation"); everything is integer arithmetic, so the two paths below give identical bytes:
//   device  bf_segment + bf_segment_get, when the C-ABI library has them;
//   host    bf_get_time_img + bf_writeout_events and a plain union-find over the pixels -- a C-ABI library without the entries
//           (the CPU stand-in the tests build) gets its segmentation from here, and it is the path the device is timed against.
#ifndef BF_HOST_CLUSTERING_H
#define BF_HOST_CLUSTERING_H

#include <bf_accel.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack them, as in flow_field.h)
extern "C" {
void bf_segment_opts_default(bf_segment_opts *opts) __attribute__((weak));
int bf_segment(bf_ctx *ctx, const bf_segment_opts *opts, bf_segment_info *info) __attribute__((weak));
int bf_segment_get(bf_ctx *ctx, int32_t *labels_out, bf_component *comps_out, int32_t comps_cap, int32_t *cl_id_out) __attribute__((weak));
}

namespace bf {

struct Segmentation {
    bf_segment_info info;
    std::vector<int32_t> labels;          // rows x cols, id or -1
    std::vector<bf_component> comps;      // info.components rows
    std::vector<int32_t> cl_id;           // parallel to the events (upload order)
    Segmentation() : info() {}
};

class Segmenter {
  public:
    bf_segment_opts opts;

    Segmenter() {   // bf_segment_opts_default
        opts.above_s = -1.0; opts.below_s = -1.0;
        opts.min_count = 1; opts.connectivity = 8; opts.min_pixels = 1; opts.reserved = 0;
    }

    static bool device_available() { return bf_segment && bf_segment_get; }

    static int64_t quantise(float t) { return (int64_t)std::floor((double)t * 1073741824.0); }

    // Components of a rows x cols mask (non-zero = foreground): out.labels, out.comps (q: per-pixel q or null), the counts of
    // out.info.  Union-find with the smaller index as the root, so a root is its component's smallest pixel.
    static void label_mask(const std::vector<uint8_t> &mask, int rows, int cols, int connectivity, int min_pixels, const int64_t *q,
                           Segmentation &out) {
        const size_t P = (size_t)rows * cols;
        std::vector<int32_t> parent(P, -1);
        auto find = [&](int32_t a) {
            while (parent[a] != a) {   // (a parent is never larger than its child: the walk descends)
                parent[a] = parent[parent[a]];
                a = parent[a];
            }
            return a;
        };
        auto unite = [&](int32_t a, int32_t b) {
            a = find(a); b = find(b);
            if (a < b) parent[b] = a;
            else if (b < a) parent[a] = b;
        };
        int32_t fg = 0;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const int32_t p = r * cols + c;
                if (!mask[p]) continue;
                ++fg;
                parent[p] = p;
                if (c > 0 && mask[p - 1]) unite(p, p - 1);
                if (r > 0) {
                    if (mask[p - cols]) unite(p, p - cols);
                    if (connectivity == 8) {
                        if (c > 0 && mask[p - cols - 1]) unite(p, p - cols - 1);
                        if (c + 1 < cols && mask[p - cols + 1]) unite(p, p - cols + 1);
                    }
                }
            }
        std::vector<int32_t> size(P, 0), ident(P, -1);
        for (size_t p = 0; p < P; ++p)
            if (mask[p]) ++size[find((int32_t)p)];
        int32_t found = 0, kept = 0;
        out.comps.clear();
        for (size_t p = 0; p < P; ++p) {
            if (!mask[p] || parent[p] != (int32_t)p) continue;
            ++found;
            if (size[p] < min_pixels) continue;
            bf_component k = bf_component();
            k.id = kept; k.first_pixel = (int32_t)p;
            k.row_min = INT_MAX; k.row_max = INT_MIN; k.col_min = INT_MAX; k.col_max = INT_MIN;
            out.comps.push_back(k);
            ident[p] = kept++;
        }
        out.labels.assign(P, -1);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t p = (size_t)r * cols + c;
                if (!mask[p]) continue;
                const int32_t id = ident[find((int32_t)p)];
                out.labels[p] = id;
                if (id < 0) continue;
                bf_component &k = out.comps[id];
                ++k.pixels;
                if (r < k.row_min) k.row_min = r;
                if (r > k.row_max) k.row_max = r;
                if (c < k.col_min) k.col_min = c;
                if (c > k.col_max) k.col_max = c;
                k.row_sum += r; k.col_sum += c;
                if (q) k.q_sum += q[p];
            }
        out.info.rows = rows; out.info.cols = cols;
        out.info.foreground_pixels = fg; out.info.components_found = found; out.info.components = kept;
    }

    // The whole definition from a time image, a count image and the events' positions (n each; noise: flags or null).
    // Returns BF_ERR_ARG for options bf_segment refuses.
    int segment_host(const std::vector<float> &T, const std::vector<uint32_t> &cnt, const bf_window &w, const double *pr_x,
                     const double *pr_y, const uint8_t *noise, size_t n, Segmentation &out) const {
        long long A = 0, B = 0;
        bool use_a = false, use_b = false;
        if (!threshold(opts.above_s, A, use_a) || !threshold(opts.below_s, B, use_b)) return BF_ERR_ARG;
        if (opts.min_count < 1 || opts.min_pixels < 1 || (opts.connectivity != 4 && opts.connectivity != 8)) return BF_ERR_ARG;
        const int rows = w.scale_img_x, cols = w.scale_img_y;
        const size_t P = (size_t)rows * cols;
        out.info = bf_segment_info();
        std::vector<int64_t> q(P);
        int64_t n1 = 0, Q = 0;
        for (size_t p = 0; p < P; ++p) {
            q[p] = quantise(T[p]);
            if (cnt[p] >= 1u) { ++n1; Q += q[p]; }
        }
        int64_t mu = 0;
        if (n1 > 0) {
            mu = Q / n1;
            if (Q % n1 != 0 && Q < 0) --mu;   // floor, not truncation
        }
        std::vector<uint8_t> mask(P, 0);
        for (size_t p = 0; p < P; ++p) {
            if (cnt[p] < (uint32_t)opts.min_count) continue;
            mask[p] = (!use_a && !use_b) || (use_a && q[p] - mu > A) || (use_b && mu - q[p] > B);
        }
        label_mask(mask, rows, cols, opts.connectivity, opts.min_pixels, q.data(), out);
        out.info.n1 = n1; out.info.q_sum = Q; out.info.q_mean = mu;
        out.cl_id.assign(n, -1);
        const int s = w.scale, hs = s / 2, x_sh = (int)w.x_shift, y_sh = (int)w.y_shift;   // (int): accel_lib.h:147
        for (size_t i = 0; i < n; ++i) {
            if (noise && noise[i]) continue;
            const double fx = pr_x[i] * s + x_sh, fy = pr_y[i] * s + y_sh;   // accel_lib.h:154-155
            if (!(fx > -2147483649.0 && fx < 2147483648.0 && fy > -2147483649.0 && fy < 2147483648.0)) continue;
            const int x = (int)fx, y = (int)fy;
            if ((x >= w.metric_wsizex + hs) || (x < hs) || (y >= w.metric_wsizey + hs) || (y < hs)) continue;
            const int32_t id = out.labels[(size_t)x * cols + y];
            out.cl_id[i] = id;
            if (id >= 0) ++out.comps[id].events;
        }
        return BF_OK;
    }

    // The segmentation of the context's live slice (n events, window w as bf_set_cloud returned it; noise: the flags as
    // uploaded, or null).  force_host: the host path even where the library has the device entries.  Returns the C-ABI's code.
    int run(bf_ctx *ctx, const bf_window &w, size_t n, const uint8_t *noise, Segmentation &out, bool force_host = false) const {
        const size_t P = (size_t)w.scale_img_x * (size_t)w.scale_img_y;
        if (device_available() && !force_host) {
            int rc = bf_segment(ctx, &opts, &out.info);
            if (rc < 0) return rc;
            out.labels.assign(P, -1);
            out.comps.assign((size_t)out.info.components, bf_component());
            out.cl_id.assign(n, -1);
            return bf_segment_get(ctx, out.labels.data(), out.comps.data(), out.info.components, out.cl_id.data());
        }
        std::vector<float> T(P);
        std::vector<uint32_t> cnt(P);
        std::vector<double> px(n), py(n);
        int rc = bf_get_time_img(ctx, T.data(), cnt.data());
        if (rc >= 0 && n > 0) rc = bf_writeout_events(ctx, px.data(), py.data(), nullptr, nullptr);
        if (rc < 0) return rc;
        return segment_host(T, cnt, w, px.data(), py.data(), noise, n, out);
    }

  private:
    static bool threshold(double s, long long &q, bool &use) {
        if (s != s || std::isinf(s)) return false;
        use = s >= 0.0;
        q = 0;
        if (use) {
            const double v = std::floor(s * 1073741824.0);
            if (v >= 9.0e18) return false;
            q = (long long)v;
        }
        return true;
    }
};

// One line per component, integers only:
// id first_pixel pixels events row_min row_max col_min col_max row_sum col_sum
// The file holds what is the same from every implementation of the C-ABI: counts, positions and sums of positions.  q_sum and
// the mean of q are left to bf_segment_get / Segmentation: they carry the last bits of the time image, which the reference's
// f32 running sum (accel_lib.h:162) and the device's exact sum round differently (7e-10 relative on a 10 000-event recording),
// while the labels -- strict integer comparisons far from their thresholds on all but a vanishing share of pixels -- agree.
inline bool write_segments_txt(const std::string &path, const Segmentation &s) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# %d x %d, n1 %lld, foreground %d, found %d, kept %d\n", s.info.rows, s.info.cols, (long long)s.info.n1,
                 s.info.foreground_pixels, s.info.components_found, s.info.components);
    for (const bf_component &k : s.comps)
        std::fprintf(f, "%d %d %d %d %d %d %d %d %lld %lld\n", k.id, k.first_pixel, k.pixels, k.events, k.row_min, k.row_max,
                     k.col_min, k.col_max, (long long)k.row_sum, (long long)k.col_sum);
    return std::fclose(f) == 0;
}

// 16-bit binary PGM (big-endian samples): id + 1, 0 = background; ids beyond 65534 are written as 65535.
inline bool write_labels_pgm(const std::string &path, const Segmentation &s) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P5\n%d %d\n65535\n", s.info.cols, s.info.rows);
    std::vector<uint8_t> row((size_t)s.info.cols * 2);
    for (int r = 0; r < s.info.rows; ++r) {
        for (int c = 0; c < s.info.cols; ++c) {
            const int32_t id = s.labels[(size_t)r * s.info.cols + c];
            const uint32_t v = id < 0 ? 0u : (id >= 65535 ? 65535u : (uint32_t)id + 1u);
            row[2 * c] = (uint8_t)(v >> 8);
            row[2 * c + 1] = (uint8_t)(v & 0xffu);
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    return std::fclose(f) == 0;
}

}  // namespace bf

#endif  // BF_HOST_CLUSTERING_H
