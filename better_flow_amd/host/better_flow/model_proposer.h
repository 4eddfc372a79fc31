// model_proposer.h -- bf::ModelProposer: candidate motion models from the modes of the per-event best flow the exhaustive search
// leaves behind (include/bf_accel.h, "event groups: candidate models") -- the policy for where the candidates
// of bf::MotionAssigner come from, which DESIGN sections 14 and 15 left open.
//
// Two paths with the same proposals, models, info, H and B (integers after the index match, so equal, not close):
//   propose()            bf_propose_models: three kernels on the state bf_global_search left on the device;
//   propose_from_best()  the same definition on host arrays (the per-event state as bf_global_get_events returns it): what a
//                        program without a device runs.
#ifndef BF_HOST_MODEL_PROPOSER_H
#define BF_HOST_MODEL_PROPOSER_H

#include <bf_accel.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack it, as in motion_assign.h)
extern "C" {
int bf_propose_models(bf_ctx *ctx, const bf_global_search_opts *lattice, const bf_propose_opts *opts, bf_model *models_out,
                      bf_proposal *proposals_out, int32_t cap, uint32_t *hist_out, uint32_t *box_out, int64_t planes_cap,
                      bf_propose_info *info) __attribute__((weak));
}

namespace bf {

class ModelProposer {
  public:
    struct Result {
        std::vector<bf_model> models;         // pick order
        std::vector<bf_proposal> proposals;
        bf_propose_info info;
        std::vector<uint32_t> H, B;           // n_x * n_y words each, row i at i * n_y (propose(): only with want_planes)
        Result() : info() {}
    };

    Result result;                            // what propose() leaves

    static bool device_available() { return bf_propose_models != nullptr; }

    static bf_global_search_opts default_lattice() {   // bf_global_search_opts_default (optimizer_global.cpp:106-108)
        bf_global_search_opts o;
        o.x_low = -0.09; o.x_hi = 0.09; o.y_low = -0.04; o.y_hi = 0.04;
        o.x_step = 0.001; o.y_step = 0.001;
        o.nz = 127;
        return o;
    }
    static bf_propose_opts default_opts() {
        bf_propose_opts o;
        std::memset(&o, 0, sizeof(o));
        o.radius = 1; o.suppress = 2; o.max_models = 8; o.min_votes = 1;
        return o;
    }

    // The device entry on the state the context holds (bf_global_set_window + a search over `lattice`).
    int propose(bf_ctx *ctx, const bf_global_search_opts &lattice, const bf_propose_opts &o, bool want_planes = false) {
        result = Result();
        if (!device_available()) return BF_ERR_STATE;
        const size_t cap = (size_t)std::max(o.max_models, 1);
        result.models.resize(cap);
        result.proposals.resize(cap);
        size_t bins = 0;
        if (want_planes) {
            std::vector<double> xs, ys;
            if (!sweep(lattice, xs, ys)) return BF_ERR_ARG;
            bins = xs.size() * ys.size();
            result.H.assign(bins, 0u);
            result.B.assign(bins, 0u);
        }
        const int rc = bf_propose_models(ctx, &lattice, &o, result.models.data(), result.proposals.data(), (int32_t)cap,
                                         want_planes ? result.H.data() : nullptr, want_planes ? result.B.data() : nullptr,
                                         (int64_t)bins, &result.info);
        const size_t P = rc >= 0 ? (size_t)result.info.proposals : 0;
        result.models.resize(P);
        result.proposals.resize(P);
        return rc;
    }

    // The same work on host arrays of n events; the error codes of the device entry's option checks.
    static int propose_from_best(const double *best_nx, const double *best_ny, const double *max_score, size_t n,
                                 const bf_global_search_opts &lattice, const bf_propose_opts &o, Result *out) {
        *out = Result();
        if (o.radius < 0 || o.radius > 8 || o.suppress < 0 || o.suppress > 64 || o.max_models < 1 || o.max_models > 64 ||
            o.min_votes < 1)
            return BF_ERR_ARG;
        std::vector<double> xs, ys;
        if (!sweep(lattice, xs, ys)) return BF_ERR_ARG;
        const long long n_x = (long long)xs.size(), n_y = (long long)ys.size(), bins = n_x * n_y;
        if (bins > (1ll << 22)) return BF_ERR_CAPACITY;
        if (lattice.nz != 127.0) return BF_ERR_ARG;   // (the models are always made here)
        out->info.n_x = n_x; out->info.n_y = n_y;
        out->H.assign((size_t)bins, 0u);
        out->B.assign((size_t)bins, 0u);
        if (n == 0) return BF_OK;
        // votes: exact double equality on both axes
        for (size_t e = 0; e < n; ++e) {
            if (!(max_score[e] > 0.0)) { ++out->info.unscored; continue; }
            const long long i = index_of(xs, best_nx[e]), j = i < 0 ? -1 : index_of(ys, best_ny[e]);
            if (i < 0 || j < 0) { ++out->info.off_lattice; continue; }
            ++out->H[(size_t)(i * n_y + j)];
            ++out->info.voted;
        }
        // smoothing: row sums, then column sums, zero outside the lattice
        const long long r = o.radius;
        std::vector<uint32_t> row((size_t)bins);
        for (long long i = 0; i < n_x; ++i)
            for (long long j = 0; j < n_y; ++j) {
                uint32_t s = 0;
                for (long long d = std::max(0ll, j - r); d <= std::min(n_y - 1, j + r); ++d) s += out->H[(size_t)(i * n_y + d)];
                row[(size_t)(i * n_y + j)] = s;
            }
        for (long long i = 0; i < n_x; ++i)
            for (long long j = 0; j < n_y; ++j) {
                uint32_t s = 0;
                for (long long d = std::max(0ll, i - r); d <= std::min(n_x - 1, i + r); ++d) s += row[(size_t)(d * n_y + j)];
                out->B[(size_t)(i * n_y + j)] = s;
            }
        // the greedy pick: the largest B not within `suppress` of an earlier pick, the lowest index among equals
        std::vector<uint8_t> taken((size_t)bins, 0);
        for (int p = 0; p < o.max_models; ++p) {
            long long best = -1;
            for (long long k = 0; k < bins; ++k)
                if (!taken[(size_t)k] && (best < 0 || out->B[(size_t)k] > out->B[(size_t)best])) best = k;
            if (best < 0 || out->B[(size_t)best] < (uint32_t)o.min_votes) break;
            const long long bi = best / n_y, bj = best % n_y;
            for (long long i = std::max(0ll, bi - o.suppress); i <= std::min(n_x - 1, bi + o.suppress); ++i)
                for (long long j = std::max(0ll, bj - o.suppress); j <= std::min(n_y - 1, bj + o.suppress); ++j)
                    taken[(size_t)(i * n_y + j)] = 1;
            bf_proposal q;
            std::memset(&q, 0, sizeof(q));
            q.nx = xs[(size_t)bi]; q.ny = ys[(size_t)bj];
            compute_uv(q.nx, q.ny, lattice.nz, &q.u, &q.v);
            q.index = best;
            q.votes = (int32_t)out->B[(size_t)best];
            q.peak = (int32_t)out->H[(size_t)best];
            out->proposals.push_back(q);
            out->models.push_back(model_of_flow(q.nx, q.ny));
        }
        out->info.proposals = (int32_t)out->proposals.size();
        return BF_OK;
    }

    // The model whose set_model warp (optimizer_rolling.h:289-299) compensates the flow (nx, ny).
    static bf_model model_of_flow(double nx, double ny) {
        bf_model m;
        std::memset(&m, 0, sizeof(m));
        m.total_dx = -nx;
        m.total_dy = -ny;
        return m;
    }

    // The lattice's values as bf_global_search builds them (optimizer_global.cpp:134-135): repeated double addition.
    static bool sweep(const bf_global_search_opts &o, std::vector<double> &xs, std::vector<double> &ys) {
        if (!(o.x_step > 0) || !(o.y_step > 0) || !(o.x_low < o.x_hi) || !(o.y_low < o.y_hi) || !(o.nz > 0) ||
            !std::isfinite(o.x_hi) || !std::isfinite(o.y_hi))
            return false;
        const size_t limit = (size_t)1 << 26;
        for (double v = o.x_low; v < o.x_hi; v += o.x_step) {
            xs.push_back(v);
            if (xs.size() > limit) return false;
        }
        for (double v = o.y_low; v < o.y_hi; v += o.y_step) {
            ys.push_back(v);
            if (ys.size() > limit) return false;
        }
        return true;
    }

    // Event::compute_uv (event.h:135-142) with the candidate's nz, as bf_global_get_events evaluates it.
    static void compute_uv(double nx, double ny, double nz, double *u, double *v) {
        const double xy_len = std::hypot(nx, ny);
        const double speed = xy_len / (nz / (1000000000 / (1 * 10000)));
        *u = xy_len == 0 ? 0 : speed * nx / xy_len;
        *v = xy_len == 0 ? 0 : speed * ny / xy_len;
    }

  private:
    static long long index_of(const std::vector<double> &vals, double v) {
        const auto it = std::lower_bound(vals.begin(), vals.end(), v);   // (NaN: begin(), and the comparison below fails)
        return (it != vals.end() && *it == v) ? (long long)(it - vals.begin()) : -1;
    }
};

}  // namespace bf

#endif  // BF_HOST_MODEL_PROPOSER_H
