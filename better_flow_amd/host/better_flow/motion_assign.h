// motion_assign.h -- bf::MotionAssigner: the assignment step of motion segmentation by motion compensation (every event to the
// one of K candidate models under which it lands on the largest pile of other events; include/bf_accel.h, "event groups:
// assignment") and its alternation with the grouped solve of bf::ObjectTasks -- the membership policy DESIGN section 14 left
// open: assign, refit every group from its current model, assign again, until no id changes.
//
// assign() has two paths with the same ids, scores, counts and info (integers throughout, so equal, not close):
//   device  bf_assign_groups: three kernels on the uploaded slice;
//   host    against a C-ABI without that entry (the CPU stand-in the tests build): per model bf_set_cloud + bf_set_model +
//           bf_writeout_events give the events' positions under the model's warp; the pixels in the assignment's own window,
//           the votes, the box sums and the pick are done here.
// The prior of a round with use_prior is the grouping of the round before it (install), or set_prior()'s.
#ifndef BF_HOST_MOTION_ASSIGN_H
#define BF_HOST_MOTION_ASSIGN_H

#include <better_flow/object_tasks.h>
#include <bf_accel.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack it, as in clustering.h and object_tasks.h)
extern "C" {
int bf_assign_groups(bf_ctx *ctx, const bf_assign_opts *opts, const bf_model *models, int32_t n_models, int32_t *group_id_out,
                     int32_t *score_out, int32_t *counts_out, bf_assign_info *info) __attribute__((weak));
}

namespace bf {

class MotionAssigner {
  public:
    struct Record {                       // one alternation
        int32_t changed;                  // ids the first assignment of the alternation changed
        std::vector<int32_t> counts;      // K + 1 of its last assignment (last: unassigned)
        std::vector<int32_t> iterations;  // per group of the refit; empty: the alternation ended without one
    };

    Refit refit;                          // how alternate() refits; its force_host also takes assign() to the host path
    // what assign() leaves (upload order) ...
    std::vector<int32_t> gid, score, counts;
    bf_assign_info info;
    // ... and alternate(), beside the grouping it was given: one record per alternation
    std::vector<Record> records;

    MotionAssigner() : info() {}

    static bool device_available() { return bf_assign_groups != nullptr; }

    // Uploads the slice; the held grouping is forgotten, as in the C-ABI.
    int upload(bf_ctx *ctx, const Slice &s) {
        n_ = s.n;
        prior_.clear();
        have_prior_ = false;
        return bf_upload_events(ctx, s.fr_x, s.fr_y, s.t_ns, nullptr, (int64_t)s.n);
    }

    // The grouping a round with use_prior starts from (ids -1 .. groups - 1 in upload order), as bf_set_groups.
    int set_prior(bf_ctx *ctx, const std::vector<int32_t> &ids, int32_t groups) {
        if (ids.size() != n_) return BF_ERR_ARG;
        prior_ = ids;
        prior_K_ = groups;
        have_prior_ = true;
        if (device_available() && !refit.force_host && bf_set_groups) return bf_set_groups(ctx, ids.data(), groups);
        return BF_OK;
    }

    // One assignment of the uploaded slice (upload()); fills gid, score, counts, info.
    int assign(bf_ctx *ctx, const std::vector<bf_model> &cand, const bf_assign_opts &o) {
        const size_t K = cand.size();
        gid.assign(n_, 0);
        score.assign(n_, 0);
        counts.assign(K + 1, 0);
        std::memset(&info, 0, sizeof(info));
        int rc;
        if (device_available() && !refit.force_host)
            rc = bf_assign_groups(ctx, &o, cand.data(), (int32_t)K, gid.data(), score.data(), counts.data(), &info);
        else
            rc = assign_host(ctx, cand, o);
        if (rc >= 0 && o.install) {
            prior_ = gid;
            prior_K_ = (int32_t)K;
            have_prior_ = true;
        }
        return rc;
    }

    // Alternates assignment and refit on the slice, starting from g's models: per alternation rounds_per_fit assignments (the
    // very first without a prior, every other with the one before it), then a refit of every group (bf::Refit::refit), warm from
    // its current model.  It ends when the first assignment after a refit changes no id -- the models are then the fit of exactly
    // this membership -- or after max_alternations.  o.use_prior and o.install are set here.  It leaves g's models, ids and counts.
    // from_ids: the very first assignment takes g's ids as its prior (false: it has none).
    int alternate(bf_ctx *ctx, const Slice &s, Grouping &g, bf_assign_opts o, int rounds_per_fit, int max_alternations,
                  bool from_ids = false) {
        records.clear();
        const size_t K = g.models.size();
        bool have = from_ids;
        o.install = 1;
        for (int a = 0; a < max_alternations; ++a) {
            int rc = upload(ctx, s);   // (a refit leaves a subset, or the slice sorted, behind)
            if (rc >= 0 && have) rc = set_prior(ctx, g.gid, (int32_t)K);
            if (rc < 0) return rc;
            Record rec;
            rec.changed = 0;
            for (int r = 0; r < rounds_per_fit; ++r) {
                o.use_prior = have ? 1 : 0;
                rc = assign(ctx, g.models, o);
                if (rc < 0) return rc;
                if (r == 0) rec.changed = info.changed;
                g.gid = gid;
                g.counts = counts;
                have = true;
            }
            rec.counts = counts;
            if (a > 0 && rec.changed == 0) {
                records.push_back(rec);
                break;
            }
            rc = refit.refit(ctx, s, g, rec.iterations);
            if (rc < 0) return rc;
            records.push_back(rec);
        }
        return BF_OK;
    }

    // The host paths' pixel code, shared with bf::ObjectMerger (object_merge.h) and bf::ObjectRenderer (object_render.h).
    struct HostWindow {   // the window of the sensor widened by the margin: optimizer_rolling.h:248-283
        int s, hs, wsx, wsy, R, C, x_sh, y_sh;
    };
    static HostWindow host_window(int scale, int res_x, int res_y, int margin) {
        HostWindow w;
        w.s = scale; w.hs = scale / 2;
        const int s = scale;
        const int x_min = -margin, x_max = res_x - 1 + margin, y_min = -margin, y_max = res_y - 1 + margin;
        w.wsx = s * (x_max - x_min); w.wsy = s * (y_max - y_min);   // :263-264
        w.R = w.wsx + s; w.C = w.wsy + s;                            // :276-277
        const double x_shift = -double((x_max - x_min) / 2 + x_min) * double(s) + double(w.wsx) / 2.0 + s / 2;   // :279-282
        const double y_shift = -double((y_max - y_min) / 2 + y_min) * double(s) + double(w.wsy) / 2.0 + s / 2;
        w.x_sh = (int)x_shift; w.y_sh = (int)y_shift;                // the parameter conversion of accel_lib.h:147
        return w;
    }
    // What bf_assign_groups, bf_merge_scores and bf_project_groups all check of the window's options and the model count
    // (BF_ERR_ARG), and whether K vote planes of the window fit their 2^27 words (BF_ERR_CAPACITY).
    static bool host_plane_opts_valid(int scale, int res_x, int res_y, int margin, int K) {
        return !(scale < 1 || scale % 2 == 0 || scale / 2 > 4 || res_x < 1 || res_y < 1 || res_x > 65536 || res_y > 65536 || margin < 0 ||
                 margin > 65536 || K < 1 || K > 64);
    }
    static bool host_planes_fit(int K, const HostWindow &w) { return (long long)K * w.R * w.C <= (1ll << 27); }
    // pix[i] = the pixel index X * C + Y of uploaded event i under set_model's warp of `m` from the reset state, -1: outside.
    // px, py: room for the events' positions.
    static int host_pixels(bf_ctx *ctx, const bf_model &m, const HostWindow &w, int res_x, int res_y, std::vector<double> &px,
                           std::vector<double> &py, std::vector<int32_t> &pix) {
        // Event::reset, then set_model's warp_reinit (optimizer_rolling.h:289-299)
        int rc = bf_set_cloud(ctx, w.s, res_x, res_y, nullptr);
        if (rc >= 0) rc = bf_set_model(ctx, &m);
        if (rc >= 0) rc = bf_writeout_events(ctx, px.data(), py.data(), nullptr, nullptr);
        if (rc < 0) return rc;
        for (size_t i = 0; i < pix.size(); ++i) {
            const int X = trunc_x86(px[i] * w.s + w.x_sh), Y = trunc_x86(py[i] * w.s + w.y_sh);   // accel_lib.h:154-155
            pix[i] = ((X >= w.wsx + w.hs) || (X < w.hs) || (Y >= w.wsy + w.hs) || (Y < w.hs)) ? -1 : X * w.C + Y;   // :157
        }
        return BF_OK;
    }
    // B = the s x s box sum of V (the splat of accel_lib.h:160-165, gathered): rows, then columns.  row: scratch of R x C.
    static void host_box_sum(const std::vector<uint32_t> &V, const HostWindow &w, std::vector<uint32_t> &row, std::vector<uint32_t> &B) {
        const int R = w.R, C = w.C, hs = w.hs;
        for (int r = 0; r < R; ++r)
            for (int c = 0; c < C; ++c) {
                uint32_t sum = 0;
                for (int d = -hs; d <= hs; ++d)
                    if (c + d >= 0 && c + d < C) sum += V[(size_t)r * C + (size_t)(c + d)];
                row[(size_t)r * C + c] = sum;
            }
        for (int r = 0; r < R; ++r)
            for (int c = 0; c < C; ++c) {
                uint32_t sum = 0;
                for (int d = -hs; d <= hs; ++d)
                    if (r + d >= 0 && r + d < R) sum += row[(size_t)(r + d) * C + c];
                B[(size_t)r * C + c] = sum;
            }
    }

  private:
    // `int x = <double>` as the reference's x86-64 build does it (accel_lib.h:154-155): NaN and anything outside the int range
    // give INT_MIN, which the window test rejects
    static int trunc_x86(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

    int assign_host(bf_ctx *ctx, const std::vector<bf_model> &cand, const bf_assign_opts &o) {
        const int K = (int)cand.size();
        if (!host_plane_opts_valid(o.scale, o.sensor_res_x, o.sensor_res_y, o.margin, K) || o.min_score < 1) return BF_ERR_ARG;
        if (o.use_prior && !have_prior_) return BF_ERR_STATE;
        if (o.use_prior && prior_K_ != K) return BF_ERR_ARG;
        const HostWindow w = host_window(o.scale, o.sensor_res_x, o.sensor_res_y, o.margin);
        const int s = w.s, R = w.R, C = w.C;
        if (!host_planes_fit(K, w)) return BF_ERR_CAPACITY;
        const size_t n = n_, P = (size_t)R * (size_t)C;
        if (n == 0) return BF_OK;
        std::vector<int32_t> best(n, 0), arg(n, 0), pix(n);
        std::vector<uint32_t> V(P), B(P), row(P);
        std::vector<double> px(n), py(n);
        for (int k = 0; k < K; ++k) {
            const int rc = host_pixels(ctx, cand[(size_t)k], w, o.sensor_res_x, o.sensor_res_y, px, py, pix);
            if (rc < 0) return rc;
            std::fill(V.begin(), V.end(), 0u);
            for (size_t i = 0; i < n; ++i)
                if (pix[i] >= 0 && votes(o, i, k)) ++V[(size_t)pix[i]];
            const std::vector<uint32_t> *S = &V;
            if (s > 1) {
                host_box_sum(V, w, row, B);
                S = &B;
            }
            for (size_t i = 0; i < n; ++i) {
                if (pix[i] < 0) continue;
                const int32_t sc = (int32_t)(*S)[(size_t)pix[i]] - (votes(o, i, k) ? 1 : 0);   // leave-one-out
                if (sc > best[i]) { best[i] = sc; arg[i] = k; }   // (strictly larger: ties stay with the smaller k)
            }
        }
        int32_t top = 0, changed = 0;
        for (size_t i = 0; i < n; ++i) {
            const int32_t g = best[i] >= o.min_score ? arg[i] : -1;
            gid[i] = g;
            score[i] = best[i];
            ++counts[(size_t)(g < 0 ? K : g)];
            changed += g != (o.use_prior ? prior_[i] : -1);
            if (best[i] > top) top = best[i];
        }
        info.models = K;
        info.rows = R; info.cols = C;
        info.unassigned = counts[(size_t)K];
        info.assigned = (int32_t)n - counts[(size_t)K];
        info.changed = changed;
        info.max_score = top;
        return BF_OK;
    }

    bool votes(const bf_assign_opts &o, size_t i, int k) const { return !o.use_prior || prior_[i] == k || prior_[i] == -1; }

    size_t n_ = 0;
    std::vector<int32_t> prior_;
    int32_t prior_K_ = 0;
    bool have_prior_ = false;
};

}  // namespace bf

#endif  // BF_HOST_MOTION_ASSIGN_H
