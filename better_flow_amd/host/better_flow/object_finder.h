// object_finder.h -- bf::ObjectFinder: the moving objects of one slice without a hint from the caller:
//   1. bf_global_set_window + bf_global_search over a lattice: every event's sharpest candidate;
//   2. bf::ModelProposer::propose: the modes of that per-event best flow as K candidate models;
//   3. bf::MotionAssigner::alternate from them: assignment and grouped refit until no id changes;
//   4. (merge_num > 0) bf::ObjectMerger::reduce: groups that are one motion are merged, so the K proposed is "at most K"
//      (DESIGN section 18).
// With hold_flow it ends with every event's flow under its own object's model held on the device (bf_hold_groups, DESIGN
// section 19): the per-object median flow comes from there, and the context is left holding the slice, the grouping and that flow
// for the readers of the held flow (bf_global_get_flow, bf_global_flow_field, bf_global_render_flow_frame, ...).
// It needs the device library: the CPU stand-in the tests build has no bf_global_*.  Against a C-ABI that lacks an entry find()
// returns BF_ERR_STATE and `error` names the entry.
#ifndef BF_HOST_OBJECT_FINDER_H
#define BF_HOST_OBJECT_FINDER_H

#include <better_flow/model_proposer.h>
#include <better_flow/motion_assign.h>
#include <better_flow/object_merge.h>

#include <cstdio>
#include <string>

// (weak, as in model_proposer.h)
extern "C" {
int bf_global_search(bf_ctx *ctx, const bf_global_search_opts *opts, bf_global_result *out, int64_t *surface_out,
                     int64_t surface_cap) __attribute__((weak));
int bf_hold_groups(bf_ctx *ctx, const bf_model *models, int32_t n_models) __attribute__((weak));
int bf_group_flow_medians(bf_ctx *ctx, double *u_med, double *v_med, int32_t *counts) __attribute__((weak));
int bf_global_get_flow(bf_ctx *ctx, double *nx, double *ny, double *u, double *v, double *pr_x, double *pr_y) __attribute__((weak));
int bf_global_render_flow_frame(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t owner_rule, uint8_t *ppm_out, uint8_t *avi_out,
                                float *flo_out) __attribute__((weak));
}

namespace bf {

class ObjectFinder {
  public:
    // the search (its window and lattice), the proposal, the alternation (the assignment's window) and every refit (`refit`)
    int search_scale = 1, search_wsize = 5;
    bf_global_search_opts lattice;
    bf_propose_opts propose;
    bf_assign_opts assign;
    Refit refit;
    int rounds_per_fit = 2, max_alternations = 5;
    // merging (bf::ObjectMerger::reduce after the alternation): a group adopts another's model when it keeps merge_num /
    // merge_den of its contrast; merge_num == 0: off, nothing changes.  A group below dissolve_below events is dissolved.
    uint64_t merge_num = 0, merge_den = 1;
    int32_t dissolve_below = 0;
    int merge_max_steps = 64;
    // false: the groups' median flows come from one upload and write-out per group, and the context is left holding the last
    // group's events.  true: hold_grouping() under the search's window, then held_flows(); the context is left holding the slice,
    // the grouping and the held flow.  When no group is left (nothing scored, or the merger dissolved every group) there is no
    // model to hold a flow under: find() returns BF_OK with empty models and flows as without hold_flow, nothing is held, and the
    // readers of the held flow return BF_ERR_STATE (every path to that end has uploaded events since any earlier hold).
    bool hold_flow = false;

    // what find() leaves: the grouping (K models, the ids in upload order, K + 1 counts, per group the proposal it started
    // from), the proposals the models started from and one record per alternation
    Grouping grouping;
    std::vector<bf_proposal> proposals;
    std::vector<MotionAssigner::Record> records;
    std::vector<double> flow_u, flow_v;   // per group: the median (u, v) in px / s of its events under its model's warp
    std::vector<ObjectMerger::Step> steps;   // (merging) what reduce() did, and the final grouping's contrast sum N^2
    uint64_t merged_sum_sq = 0;
    std::string error;

    ObjectFinder() : lattice(ModelProposer::default_lattice()), propose(ModelProposer::default_opts()), assign() {
        assign.scale = 3;
        assign.sensor_res_x = 180; assign.sensor_res_y = 240;
        assign.margin = 0; assign.min_score = 1;
    }

    // The entry the linked C-ABI lacks, or null.
    static const char *missing_entry(bool merging = false, bool holding = false) {
        if (!bf_propose_models) return "bf_propose_models";
        if (!bf_global_search || !bf_global_set_window) return "bf_global_search";
        if (!MotionAssigner::device_available()) return "bf_assign_groups";
        if (merging && !ObjectMerger::device_available()) return "bf_merge_scores";
        if (holding && (!bf_hold_groups || !bf_group_flow_medians || !bf_set_groups)) return "bf_hold_groups";
        return nullptr;
    }

    int find(bf_ctx *ctx, const Slice &s) { const int rc = group(ctx, s); return rc < 0 ? rc : flows(ctx, s); }
    // find() in its parts, for a caller with its own use of the context before the flows (bf::ObjectTracker): up to the grouping ...
    int group(bf_ctx *ctx, const Slice &s) {
        if (const int rc = begin()) return rc;
        int rc = bf_upload_events(ctx, s.fr_x, s.fr_y, s.t_ns, nullptr, (int64_t)s.n);
        if (rc >= 0) rc = bf_global_set_window(ctx, search_scale, search_wsize, nullptr);
        if (rc >= 0) rc = bf_global_search(ctx, &lattice, nullptr, nullptr, 0);
        ModelProposer mp;
        if (rc >= 0) rc = mp.propose(ctx, lattice, propose);
        if (rc < 0) return fail(ctx, rc, error);
        proposals = mp.result.proposals;
        return refine(ctx, s, mp.result.models);
    }
    // ... or without the search: the alternation starts from `candidates` (the previous slice's models: bf::ObjectTracker's warm
    // path) instead of from proposals; no bf_global_set_window, bf_global_search or bf_propose_models runs.  Everything after
    // the candidates is group()'s own code; `proposals` stays empty and origin[k] is the candidate group k started from.
    int group_from(bf_ctx *ctx, const Slice &s, const std::vector<bf_model> &candidates) {
        if (const int rc = begin()) return rc;
        return refine(ctx, s, candidates);
    }
    // ... the groups' median flows as hold_flow says ...
    int flows(bf_ctx *ctx, const Slice &s) {
        const bool hold = hold_flow && !grouping.models.empty();   // (no group: group_flows does nothing)
        int rc = hold ? hold_grouping(ctx, s, grouping.gid, grouping.models.size(), search_scale, search_wsize) : group_flows(ctx, s);
        if (rc >= 0 && hold) rc = held_flows(ctx);
        return rc < 0 ? fail(ctx, rc, error) : BF_OK;
    }
    // ... and, on a context that holds the slice, the search's window and the grouping, the held flow and its medians: every event
    // under its own group's model on the device, the medians by its select (include/bf_accel.h, "the held flow of a grouping").
    int held_flows(bf_ctx *ctx) {
        int rc = bf_hold_groups(ctx, grouping.models.data(), (int32_t)grouping.models.size());
        if (rc >= 0) rc = bf_group_flow_medians(ctx, flow_u.data(), flow_v.data(), nullptr);
        return rc;
    }

    // objects_N.txt: one line per group -- id, events, the median (u, v) of its events under its model in px / s, the model's
    // fields (cx cy dx dy rot div cnt total_dx total_dy total_rot total_div), the votes of the proposal it started from --, then a
    // last line "unassigned <events>".  False: the file cannot be opened.
    bool write_objects(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        for (size_t k = 0; k < grouping.models.size(); ++k) {
            const bf_model &m = grouping.models[k];
            std::fprintf(f, "%zu %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %u %.17g %.17g %.17g %.17g %d\n", k, (int)grouping.counts[k],
                         flow_u[k], flow_v[k], m.cx, m.cy, m.dx, m.dy, m.rot, m.div, (unsigned)m.cnt, m.total_dx, m.total_dy,
                         m.total_rot, m.total_div, (size_t)grouping.origin[k] < proposals.size() ? (int)proposals[(size_t)grouping.origin[k]].votes : 0);
        }
        std::fprintf(f, "unassigned %d\n", grouping.counts.empty() ? 0 : (int)grouping.counts.back());
        std::fclose(f);
        return true;
    }
    // objects_N.events.txt: per event of the slice "t x y group u v", (u, v)[n] its held flow.
    bool write_events(const std::string &path, const Slice &s, const std::vector<double> &u, const std::vector<double> &v) const {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        for (size_t i = 0; i < s.n; ++i)
            std::fprintf(f, "%d %d %d %d %.9f %.9f\n", (int)s.t_ns[i], (int)s.fr_x[i], (int)s.fr_y[i], (int)grouping.gid[i], u[i], v[i]);
        return std::fclose(f) == 0;
    }

    static int fail(bf_ctx *ctx, int rc, std::string &error) {   // rc, with the context's message in `error`
        const char *m = bf_last_error(ctx);
        error = m ? m : "";
        return rc;
    }

  private:
    int begin() {
        grouping = Grouping();
        proposals.clear(); records.clear(); flow_u.clear(); flow_v.clear(); steps.clear(); error.clear();
        merged_sum_sq = 0;
        if (const char *m = missing_entry(merge_num > 0, hold_flow)) {
            error = std::string("bf::ObjectFinder: the linked library has no ") + m;
            return BF_ERR_STATE;
        }
        return BF_OK;
    }
    // From the candidates: the alternation, the merger when it is on.
    int refine(bf_ctx *ctx, const Slice &s, const std::vector<bf_model> &candidates) {
        grouping = Grouping(candidates, s.n);
        if (grouping.models.empty()) return BF_OK;   // nothing scored: no object
        MotionAssigner ma;
        ma.refit = refit;
        int rc = ma.alternate(ctx, s, grouping, assign, rounds_per_fit, max_alternations);
        if (rc < 0) return fail(ctx, rc, error);
        records = ma.records;
        if (merge_num > 0) {
            ObjectMerger om;
            om.opts.scale = assign.scale;
            om.opts.sensor_res_x = assign.sensor_res_x; om.opts.sensor_res_y = assign.sensor_res_y;
            om.opts.margin = assign.margin;
            om.assign = assign;
            om.refit = refit;
            om.rounds_per_fit = rounds_per_fit;
            rc = om.reduce(ctx, s, grouping, merge_num, merge_den, dissolve_below, merge_max_steps);
            if (rc < 0) return fail(ctx, rc, error);
            steps = om.steps;
            merged_sum_sq = om.info.sum_sq;
        }
        flow_u.assign(grouping.models.size(), 0.0);   // (filled by flows() or held_flows(); an empty group keeps 0)
        flow_v.assign(grouping.models.size(), 0.0);
        return BF_OK;
    }

    // Per group its events alone under set_model's warp of its model (optimizer_rolling.h:289-299), Event::compute_uv of
    // what that leaves, and the median per axis (the mean of the two middle values of an even count).
    int group_flows(bf_ctx *ctx, const Slice &s) {
        const Grouping &g = grouping;
        std::vector<int32_t> x, y, t;
        std::vector<double> nx, ny, u, v;
        for (size_t k = 0; k < g.models.size(); ++k) {
            s.subset(g.gid, (int32_t)k, x, y, t);
            if (x.empty()) continue;
            bf_window w;
            int rc = bf_upload_events(ctx, x.data(), y.data(), t.data(), nullptr, (int64_t)x.size());
            if (rc >= 0) rc = bf_set_cloud(ctx, refit.fit.scale, refit.fit.sensor_res_x, refit.fit.sensor_res_y, &w);
            if (rc >= 0) rc = bf_set_model(ctx, &g.models[k]);
            nx.assign(x.size(), 0.0); ny.assign(x.size(), 0.0);
            if (rc >= 0) rc = bf_writeout_events(ctx, nullptr, nullptr, nx.data(), ny.data());
            if (rc < 0) return rc;
            u.resize(x.size()); v.resize(x.size());
            for (size_t i = 0; i < x.size(); ++i) ModelProposer::compute_uv(nx[i], ny[i], 127.0, &u[i], &v[i]);
            flow_u[k] = median(u);
            flow_v[k] = median(v);
        }
        return BF_OK;
    }
    static double median(std::vector<double> &a) {
        std::sort(a.begin(), a.end());
        const size_t m = a.size() / 2;
        return a.size() % 2 ? a[m] : 0.5 * (a[m - 1] + a[m]);
    }
};

}  // namespace bf

#endif  // BF_HOST_OBJECT_FINDER_H
