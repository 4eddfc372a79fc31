// object_merge.h -- bf::ObjectMerger: the number of objects (include/bf_accel.h, "event groups: merge gains").
// Start from more candidate models than objects and let the objective, the contrast sum N^2 of the slice under its groups'
// models, say which groups are one motion: gain[b][a] is what the events of group b add to it under model a, so
// gain[b][a] / gain[b][b] is how much of b's contrast survives when b adopts a's model.
//
// scores() has two paths with the same bytes (integers throughout, so equal, not close):
//   scores()       bf_merge_scores on the context's uploaded slice and held grouping;
//   scores_host()  the same definition on host arrays (slice, ids, models), against any C-ABI: bf::MotionAssigner's host pixel
//                  code gives the events' pixels under each model; planes, box sums and gains are done here.
// pick() is the policy: which ordered pair merges next, compared exactly.  reduce() is the loop: dissolve what is empty or too
// small, score, pick, merge, one alternation (bf::MotionAssigner) after every change, until nothing is picked.
#ifndef BF_HOST_OBJECT_MERGE_H
#define BF_HOST_OBJECT_MERGE_H

#include <better_flow/motion_assign.h>

#include <cstdio>
#include <string>

// (weak, as in motion_assign.h)
extern "C" {
int bf_merge_scores(bf_ctx *ctx, const bf_merge_opts *opts, const bf_model *models, int32_t n_models, uint64_t *gain_out,
                    int32_t *inside_out, int32_t *events_out, bf_merge_info *info) __attribute__((weak));
}

namespace bf {

class ObjectMerger {
  public:
    enum Kind { MERGE = 0, DISSOLVE = 1 };
    struct Step {                         // one change of reduce()
        int32_t kind;                     // MERGE: group b took model a's id; DISSOLVE: the events of b went to -1 (a == -1)
        int32_t b, a;                     // ids before the step
        uint64_t gain_ba, gain_bb;        // of the scores the pick was made on (DISSOLVE: 0)
        int32_t events_b, K_after;
    };
    struct Pick {
        bool found, accepted;             // a candidate exists; it reaches num / den
        int32_t b, a;
    };

    bf_merge_opts opts;                   // scale, sensor, margin, targets_per_pass of the scores
    bf_assign_opts assign;                // the alternation's assignment ...
    Refit refit;                          // ... and refit (bf::MotionAssigner); its force_host also takes reduce()'s scores to scores_host()
    int rounds_per_fit = 2;
    // what scores() / scores_host() leave: K x K gains and inside counts, [b * K + a]; K event counts; the info
    std::vector<uint64_t> gain;
    std::vector<int32_t> inside, events;
    bf_merge_info info;
    // what reduce() leaves beside the grouping it was given: the steps; gain, inside, events and info above are the final grouping's
    std::vector<Step> steps;

    ObjectMerger() : opts(), assign(), info() {
        opts.scale = assign.scale = 3;
        opts.sensor_res_x = assign.sensor_res_x = 180; opts.sensor_res_y = assign.sensor_res_y = 240;
        assign.min_score = 1;
    }

    static bool device_available() { return bf_merge_scores != nullptr; }

    // The context's uploaded slice and held grouping (K = ms.size() groups) under `ms`, on the device.
    int scores(bf_ctx *ctx, const std::vector<bf_model> &ms) {
        if (!device_available()) return BF_ERR_STATE;
        if (!valid((int)ms.size())) return BF_ERR_ARG;
        size_outputs(ms.size());
        return bf_merge_scores(ctx, &opts, ms.data(), (int32_t)ms.size(), gain.data(), inside.data(), events.data(), &info);
    }

    // The same on host arrays: uploads the slice (the context's held grouping is forgotten, as by every upload).
    int scores_host(bf_ctx *ctx, const Slice &s, const std::vector<int32_t> &ids, const std::vector<bf_model> &ms) {
        const int K = (int)ms.size();
        if (!valid(K) || ids.size() != s.n) return BF_ERR_ARG;
        for (size_t i = 0; i < s.n; ++i)
            if (ids[i] < -1 || ids[i] >= K) return BF_ERR_ARG;
        const MotionAssigner::HostWindow w = MotionAssigner::host_window(opts.scale, opts.sensor_res_x, opts.sensor_res_y, opts.margin);
        if (!MotionAssigner::host_planes_fit(K, w)) return BF_ERR_CAPACITY;
        size_outputs((size_t)K);
        const size_t n = s.n, P = (size_t)w.R * (size_t)w.C, Ks = (size_t)K;
        if (n == 0) return BF_OK;   // everything zero
        int rc = bf_upload_events(ctx, s.fr_x, s.fr_y, s.t_ns, nullptr, (int64_t)n);
        if (rc < 0) return rc;
        std::vector<std::vector<uint32_t>> members(Ks);   // per group its events' upload indices
        for (size_t i = 0; i < n; ++i) {
            if (ids[i] >= 0) members[(size_t)ids[i]].push_back((uint32_t)i);
            else ++info.unassigned;
        }
        std::vector<uint32_t> V(P), T(P), row(P), N(P, 0u);
        std::vector<std::vector<uint32_t>> B(Ks);         // the base planes of the groups that have events
        std::vector<double> px(n), py(n);
        std::vector<int32_t> pix(n);
        // T = the plane of group b's events under the pixels in `pix`; returns the events inside
        auto plane_of = [&](size_t b) {
            int32_t in = 0;
            std::fill(V.begin(), V.end(), 0u);
            for (uint32_t i : members[b])
                if (pix[i] >= 0) { ++V[(size_t)pix[i]]; ++in; }
            if (w.s > 1) MotionAssigner::host_box_sum(V, w, row, T);
            else T = V;
            return in;
        };
        for (size_t b = 0; b < Ks; ++b) {
            events[b] = (int32_t)members[b].size();
            if (members[b].empty()) continue;   // an empty plane adds nothing to any pixel
            rc = MotionAssigner::host_pixels(ctx, ms[b], w, opts.sensor_res_x, opts.sensor_res_y, px, py, pix);
            if (rc < 0) return rc;
            plane_of(b);
            B[b] = T;
            for (size_t p = 0; p < P; ++p) N[p] += T[p];
        }
        for (size_t p = 0; p < P; ++p) {
            info.sum += N[p];
            info.sum_sq += (uint64_t)N[p] * N[p];
        }
        for (size_t a = 0; a < Ks; ++a) {
            rc = MotionAssigner::host_pixels(ctx, ms[a], w, opts.sensor_res_x, opts.sensor_res_y, px, py, pix);
            if (rc < 0) return rc;
            for (size_t b = 0; b < Ks; ++b) {
                if (members[b].empty()) continue;
                const int32_t in = plane_of(b);
                inside[b * Ks + a] = in;
                if (!in) continue;
                uint64_t g = 0;
                const std::vector<uint32_t> &own = B[b];
                for (size_t p = 0; p < P; ++p) {
                    const uint64_t t = T[p];
                    if (t) g += t * (2ull * ((uint64_t)N[p] - own[p]) + t);   // (wraps by definition)
                }
                gain[b * Ks + a] = g;
            }
        }
        info.models = K;
        info.rows = w.R; info.cols = w.C;
        info.passes = passes_of(K, w.R, w.C);
        return BF_OK;
    }

    // The pair that merges next.  Candidates are the ordered pairs (b, a), b != a, with events[b] >= 1, gain[b][b] > 0 and
    // events[a] > events[b], or events[a] == events[b] and a < b: a group only ever dissolves into one with at least as many
    // events (the refit does not minimise this sum, so a fragment can keep more than all of its contrast under a smaller
    // fragment's model).  The largest gain[b][a] / gain[b][b] wins, compared by cross-multiplication in 128 bits; among equals
    // the smallest b, then the smallest a.  It is accepted when gain[b][a] * den >= gain[b][b] * num.
    static Pick pick(const std::vector<uint64_t> &gain, const std::vector<int32_t> &events, uint64_t num, uint64_t den) {
        typedef unsigned __int128 u128;
        const size_t K = events.size();
        Pick best = {false, false, -1, -1};
        uint64_t best_ba = 0, best_bb = 1;
        for (size_t b = 0; b < K; ++b) {
            const uint64_t bb = gain[b * K + b];
            if (events[b] < 1 || bb == 0) continue;
            for (size_t a = 0; a < K; ++a) {
                if (a == b) continue;
                if (!(events[a] > events[b] || (events[a] == events[b] && a < b))) continue;
                const uint64_t ba = gain[b * K + a];
                // (strictly larger: equal ratios stay with the smaller b, then the smaller a)
                if (!best.found || (u128)ba * best_bb > (u128)best_ba * bb) {
                    best.found = true;
                    best.b = (int32_t)b; best.a = (int32_t)a;
                    best_ba = ba; best_bb = bb;
                }
            }
        }
        if (best.found) best.accepted = (u128)best_ba * den >= (u128)best_bb * num;
        return best;
    }

    // The loop, from g's models and ids on the slice, on g itself (origin: per final group its index among the start models).  Repeats:
    //   1. every group with no event or with fewer than dissolve_below events is removed (ids -> -1), ids and models are
    //      compacted, and if anything was removed, one alternation follows and the loop starts over;
    //   2. bf_set_groups, scores(), pick(); it ends with no accepted pick or one group;
    //   3. b is relabelled a, model b is dropped, ids and models are compacted, one alternation.
    // One alternation: rounds_per_fit assignments with the current ids as the prior, then one grouped refit warm from the
    // current models (MotionAssigner::alternate from g's ids, one alternation).  At most max_steps rounds.
    int reduce(bf_ctx *ctx, const Slice &s, Grouping &g, uint64_t num, uint64_t den, int32_t dissolve_below, int max_steps) {
        if (g.gid.size() != s.n || den == 0) return BF_ERR_ARG;
        g.reset_origin();
        steps.clear();
        bool scored = false;
        for (int round = 0; round < max_steps; ++round) {
            const size_t K = g.models.size();
            g.count_ids();
            std::vector<int32_t> drop;
            for (size_t k = 0; k < K; ++k)
                if (g.counts[k] == 0 || g.counts[k] < dissolve_below) drop.push_back((int32_t)k);
            scored = false;
            if (!drop.empty()) {
                for (size_t j = 0; j < drop.size(); ++j) {
                    const Step st = {DISSOLVE, drop[j], -1, 0, 0, g.counts[(size_t)drop[j]], (int32_t)(K - 1 - j)};
                    steps.push_back(st);
                }
                g.compact(drop);
                if (g.models.empty()) break;
                const int rc = one_alternation(ctx, s, g);
                if (rc < 0) return rc;
                continue;   // (the alternation may have emptied a group)
            }
            int rc = score_current(ctx, s, g);
            if (rc < 0) return rc;
            scored = true;
            const Pick p = pick(gain, events, num, den);
            if (K == 1 || !p.found || !p.accepted) break;
            const Step st = {MERGE, p.b, p.a, gain[(size_t)p.b * K + (size_t)p.a], gain[(size_t)p.b * K + (size_t)p.b],
                             events[(size_t)p.b], (int32_t)(K - 1)};
            steps.push_back(st);
            for (size_t i = 0; i < g.gid.size(); ++i)
                if (g.gid[i] == p.b) g.gid[i] = p.a;
            g.compact(std::vector<int32_t>(1, p.b));
            rc = one_alternation(ctx, s, g);
            if (rc < 0) return rc;
            scored = false;
        }
        g.count_ids();
        if (!scored) {   // (max_steps ran out behind a change, or nothing is left)
            if (g.models.empty()) size_outputs(0);
            else {
                const int rc = score_current(ctx, s, g);
                if (rc < 0) return rc;
            }
        }
        return BF_OK;
    }

    // "merge|dissolve b a gain_ba gain_bb events_b K_after" per step, then "info K sum_sq" of the final grouping.
    static bool write_steps(const std::string &path, const std::vector<Step> &steps, size_t K, uint64_t sum_sq) {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        for (const Step &st : steps)
            std::fprintf(f, "%s %d %d %llu %llu %d %d\n", st.kind == MERGE ? "merge" : "dissolve", (int)st.b, (int)st.a,
                         (unsigned long long)st.gain_ba, (unsigned long long)st.gain_bb, (int)st.events_b, (int)st.K_after);
        std::fprintf(f, "info %d %llu\n", (int)K, (unsigned long long)sum_sq);
        return std::fclose(f) == 0;
    }

    // info.passes of bf_merge_scores with targets_per_pass = opts.targets_per_pass.
    int passes_of(int K, int R, int C) const {
        long long A = (1ll << 27) / ((long long)K * R * C);
        if (A > K) A = K;
        if (opts.targets_per_pass >= 1 && A > opts.targets_per_pass) A = opts.targets_per_pass;
        return (int)((K + A - 1) / A);
    }

  private:
    bool valid(int K) const {   // bf_merge_scores' argument checks
        return MotionAssigner::host_plane_opts_valid(opts.scale, opts.sensor_res_x, opts.sensor_res_y, opts.margin, K) &&
               opts.targets_per_pass >= 0;
    }
    void size_outputs(size_t K) {
        gain.assign(K * K, 0);
        inside.assign(K * K, 0);
        events.assign(K, 0);
        std::memset(&info, 0, sizeof(info));
    }
    int one_alternation(bf_ctx *ctx, const Slice &s, Grouping &g) {
        MotionAssigner ma;
        ma.refit = refit;
        return ma.alternate(ctx, s, g, assign, rounds_per_fit, 1, true);
    }
    int score_current(bf_ctx *ctx, const Slice &s, const Grouping &g) {
        if (!device_available() || refit.force_host || !bf_set_groups) return scores_host(ctx, s, g.gid, g.models);
        const int rc = hold_grouping(ctx, s, g.gid, g.models.size());   // (a refit leaves a subset behind)
        return rc < 0 ? rc : scores(ctx, g.models);
    }
};

}  // namespace bf

#endif  // BF_HOST_OBJECT_MERGE_H
