// object_tasks.h -- bf::ObjectTasks: the reference's queue of (events, model) tasks (dvs_flow.h:200-231, "designed for many
// objects") over ONE slice.  push() a task -- the indices of its events in the slice and, optionally, the model to start
// from --, then run(): every task gets its own OptimizerRolling (set_cloud on its events alone, set_model, run), as
// include/bf_accel.h's "event groups" block defines it.  Two paths with the same models, return codes, iteration counts and
// per-event (nx, ny):
//   device  bf_set_groups + bf_run_groups: one upload, one launch, one work-group per task;
//   host    against a C-ABI without those entries (the CPU stand-in the tests build), the queue executed one task after the
//           other as the reference would: upload the subset, bf_set_cloud, bf_set_model, bf_run, bf_writeout_events.
// An event belongs to at most one task (a second push of the same index is BF_ERR_ARG on either path).  A task without a
// model starts cold; when only some tasks carry one, the others start from the zero model, whose set_model warp is the
// identity.  The device path reports BF_ERR_CAPACITY in the info of a task whose window exceeds the LDS; the host path has no
// such limit.  With `wide` the device path sets bf_set_option "groups_wide" around its bf_run_groups: such a task is then solved
// in the same call by the chip-wide loop, unless its window exceeds the context's image capacity (include/bf_accel.h, "wide
// groups").  No membership policy lives here: which events form an object is the caller's decision.  bf::Refit, below it, is how
// a whole grouping is refit through the queue.
#ifndef BF_HOST_OBJECT_TASKS_H
#define BF_HOST_OBJECT_TASKS_H

#include <bf_accel.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack them, as in flow_field.h and clustering.h)
extern "C" {
int bf_set_groups(bf_ctx *ctx, const int32_t *group_id, int32_t groups) __attribute__((weak));
int bf_global_set_window(bf_ctx *ctx, int32_t scale, int32_t metric_wsize, bf_global_window *out) __attribute__((weak));
int bf_set_groups_from_segments(bf_ctx *ctx, int32_t *groups_out) __attribute__((weak));
int bf_run_groups(bf_ctx *ctx, const bf_group_opts *opts, const bf_model *warm, int32_t warm_count, bf_model *models_out,
                  bf_run_info *infos_out, bf_group_info *groups_out) __attribute__((weak));
}

namespace bf {

// What the host classes of the object pipeline hand each other: bf::Slice, the events of one slice as the caller's arrays, and
// bf::Grouping, which of them form which object under which model; hold_grouping() is the one place that puts both on a context.
struct Slice {                            // borrowed for the duration of a call
    const int32_t *fr_x, *fr_y, *t_ns;
    size_t n;

    // The events i with ids[i] == k, in the slice's order, into x, y, t; where (may be null): their indices in the slice.
    void subset(const std::vector<int32_t> &ids, int32_t k, std::vector<int32_t> &x, std::vector<int32_t> &y, std::vector<int32_t> &t,
                std::vector<size_t> *where = nullptr) const {
        x.clear(); y.clear(); t.clear(); if (where) where->clear();
        for (size_t i = 0; i < n; ++i) {
            if (ids[i] != k) continue;
            x.push_back(fr_x[i]); y.push_back(fr_y[i]); t.push_back(t_ns[i]);
            if (where) where->push_back(i);
        }
    }
};

struct Grouping {
    std::vector<bf_model> models;         // K groups
    std::vector<int32_t> gid;             // per event of the slice, upload order: -1 (unassigned) .. K - 1
    std::vector<int32_t> counts;          // K + 1 (last: unassigned)
    std::vector<int32_t> origin;          // per group: its index among the models the grouping started from

    Grouping() {}
    Grouping(const std::vector<bf_model> &start, size_t n) : models(start), gid(n, -1) {   // no event assigned yet
        reset_origin();
        count_ids();
    }
    void reset_origin() {
        origin.resize(models.size());
        for (size_t k = 0; k < origin.size(); ++k) origin[k] = (int32_t)k;
    }
    void count_ids() {
        counts.assign(models.size() + 1, 0);
        for (size_t i = 0; i < gid.size(); ++i) ++counts[gid[i] < 0 ? models.size() : (size_t)gid[i]];
    }
    // Without the groups in `drop` (ascending): their events -> -1, the others renumbered in order.
    void compact(const std::vector<int32_t> &drop) {
        const size_t K = models.size();
        std::vector<int32_t> to(K, 0);
        std::vector<bf_model> kept;
        std::vector<int32_t> kept_origin;
        size_t d = 0;
        for (size_t k = 0; k < K; ++k) {
            if (d < drop.size() && drop[d] == (int32_t)k) { to[k] = -1; ++d; continue; }
            to[k] = (int32_t)kept.size();
            kept.push_back(models[k]);
            kept_origin.push_back(origin[k]);
        }
        for (size_t i = 0; i < gid.size(); ++i)
            if (gid[i] >= 0) gid[i] = to[(size_t)gid[i]];
        models.swap(kept);
        origin.swap(kept_origin);
    }
};

// The slice on the context with `ids` (-1 .. groups - 1, upload order) as its grouping: the upload, bf_global_set_window when a
// flow is going to be held under the grouping (window_scale != 0), bf_set_groups.  Needs the device library's bf_set_groups.
inline int hold_grouping(bf_ctx *ctx, const Slice &s, const std::vector<int32_t> &ids, size_t groups, int window_scale = 0, int window_wsize = 0) {
    if (ids.size() != s.n) return BF_ERR_ARG;
    int rc = bf_upload_events(ctx, s.fr_x, s.fr_y, s.t_ns, nullptr, (int64_t)s.n);
    if (rc >= 0 && window_scale != 0) rc = bf_global_set_window(ctx, window_scale, window_wsize, nullptr);
    if (rc >= 0) rc = bf_set_groups(ctx, ids.data(), (int32_t)groups);
    return rc;
}

class ObjectTasks {
  public:
    bf_group_opts opts;                   // scale, set_cloud's seeds, run()'s guards and caps: shared by the tasks
    // what run() leaves: one entry per task, and (nx, ny) per event of the slice (0 for an event of no task)
    std::vector<bf_model> models;
    std::vector<bf_run_info> infos;
    std::vector<double> nx, ny;
    bool wide = false;                    // device path: "groups_wide" = 1 for its bf_run_groups (the host path has no LDS limit)
    bool force_host = false;              // the host path even where the library has the device entries

    ObjectTasks() {   // the reference's constants (common.h:39-40, optimizer_rolling.h:57)
        opts.scale = 3;
        opts.sensor_res_x = opts.guard_res_x = 180;
        opts.sensor_res_y = opts.guard_res_y = 240;
        opts.min_events = 1000;
        opts.max_iter = -1;
        opts.hard_iter_cap = 100000;
    }

    static bool device_available() { return bf_set_groups && bf_run_groups; }

    size_t size() const { return ids_.size(); }
    void clear() { ids_.clear(); warm_.clear(); has_warm_.clear(); }

    // a task: the indices of its events in the slice run() will be given, and the model it starts from (null: cold)
    size_t push(const std::vector<int32_t> &event_ids, const bf_model *model = nullptr) {
        ids_.push_back(event_ids);
        bf_model m;
        std::memset(&m, 0, sizeof(m));
        if (model) m = *model;
        warm_.push_back(m);
        has_warm_.push_back(model != nullptr);
        return ids_.size() - 1;
    }

    // Solves the queue on the slice (fr_x, fr_y, t_ns)[n]; ctx: a context with room for n events.  Returns BF_OK or the first error
    // of the C-ABI; a task's own outcome (BF_OK, BF_SKIPPED, BF_ERR_NOCONV, BF_ERR_CAPACITY) is in infos[k].rc.
    int run(bf_ctx *ctx, const int32_t *fr_x, const int32_t *fr_y, const int32_t *t_ns, size_t n) {
        const Slice s = {fr_x, fr_y, t_ns, n};
        const size_t K = ids_.size();
        std::vector<int32_t> gid(n, -1);
        for (size_t k = 0; k < K; ++k)
            for (int32_t i : ids_[k]) {
                if (i < 0 || (size_t)i >= n || gid[(size_t)i] != -1) return BF_ERR_ARG;
                gid[(size_t)i] = (int32_t)k;
            }
        bool any_warm = false;
        for (size_t k = 0; k < K; ++k) any_warm = any_warm || has_warm_[k];
        models.assign(K, bf_model());
        infos.assign(K, bf_run_info());
        nx.assign(n, 0.0);
        ny.assign(n, 0.0);
        if (device_available() && !force_host) {
            int rc = hold_grouping(ctx, s, gid, K);
            if (rc >= 0 && wide) rc = bf_set_option(ctx, "groups_wide", 1);
            if (rc >= 0) {
                rc = bf_run_groups(ctx, &opts, any_warm ? warm_.data() : nullptr, any_warm ? (int32_t)K : 0, models.data(),
                                   infos.data(), nullptr);
                if (wide) (void)bf_set_option(ctx, "groups_wide", 0);   // (off again: the option is this queue's, not the context's other callers')
            }
            if (rc >= 0 && n > 0) rc = bf_writeout_events(ctx, nullptr, nullptr, nx.data(), ny.data());
            return rc < 0 ? rc : BF_OK;
        }
        bf_run_opts ro;
        bf_run_opts_default(&ro);
        ro.max_iter = opts.max_iter; ro.min_events = opts.min_events;
        ro.res_x = opts.guard_res_x; ro.res_y = opts.guard_res_y;
        ro.hard_iter_cap = opts.hard_iter_cap;
        std::vector<int32_t> sx, sy, st;
        std::vector<size_t> where;
        std::vector<double> snx, sny;
        for (size_t k = 0; k < K; ++k) {
            s.subset(gid, (int32_t)k, sx, sy, st, &where);   // (in the slice's order, whatever order they were pushed in)
            bf_run_info skipped = bf_run_info();
            skipped.rc = BF_SKIPPED;
            skipped.x_divider = skipped.y_divider = 1.0f;
            skipped.rot_divider = skipped.div_divider = 10000.0f;
            if (where.empty()) {   // (run() returns 1 on fewer than min_events events; nothing to warp)
                models[k] = warm_[k];
                infos[k] = skipped;
                continue;
            }
            int rc = bf_upload_events(ctx, sx.data(), sy.data(), st.data(), nullptr, (int64_t)sx.size());
            bf_window w;
            if (rc >= 0) rc = bf_set_cloud(ctx, opts.scale, opts.sensor_res_x, opts.sensor_res_y, &w);
            if (rc >= 0 && any_warm) rc = bf_set_model(ctx, &warm_[k]);
            if (rc < 0) return rc;
            models[k] = warm_[k];
            infos[k] = skipped;
            rc = bf_run(ctx, &ro, &models[k], &infos[k]);
            if (rc < 0 && rc != BF_ERR_NOCONV) return rc;
            infos[k].rc = rc;
            snx.assign(where.size(), 0.0);
            sny.assign(where.size(), 0.0);
            rc = bf_writeout_events(ctx, nullptr, nullptr, snx.data(), sny.data());
            if (rc < 0) return rc;
            for (size_t j = 0; j < where.size(); ++j) { nx[where[j]] = snx[j]; ny[where[j]] = sny[j]; }
        }
        return BF_OK;
    }

  private:
    std::vector<std::vector<int32_t>> ids_;
    std::vector<bf_model> warm_;
    std::vector<bool> has_warm_;
};

// How a grouping's groups are refit, stated once: the top-level caller fills one, and bf::MotionAssigner, bf::ObjectMerger and
// bf::ObjectFinder hold it.
struct Refit {
    bf_group_opts fit;                    // the refit's scale, seeds, guards and caps (ObjectTasks::opts)
    bool wide = false;                    // ObjectTasks::wide: no group then exceeds the LDS, and `helper` is not touched
    // borrowed: a second context with room for the slice, on which a group that came back BF_ERR_CAPACITY is refit one after the other
    bf_ctx *helper = nullptr;             // (null: it keeps its model)
    bool force_host = false;              // the host paths of the refit (ObjectTasks::force_host) and of the assignment

    Refit() { fit = ObjectTasks().opts; }

    // Every group of g refit on its events of the slice, warm from its model (a group a guard skipped keeps it); its iterations.
    int refit(bf_ctx *ctx, const Slice &s, Grouping &g, std::vector<int32_t> &iterations) const {
        const size_t K = g.models.size();
        std::vector<std::vector<int32_t>> ids(K);
        for (size_t i = 0; i < s.n; ++i)
            if (g.gid[i] >= 0) ids[(size_t)g.gid[i]].push_back((int32_t)i);
        ObjectTasks q;
        q.opts = fit;
        q.wide = wide;
        q.force_host = force_host;
        for (size_t k = 0; k < K; ++k) q.push(ids[k], &g.models[k]);
        int rc = q.run(ctx, s.fr_x, s.fr_y, s.t_ns, s.n);
        if (rc < 0) return rc;
        iterations.assign(K, 0);
        std::vector<size_t> large;
        for (size_t k = 0; k < K; ++k) {
            iterations[k] = q.infos[k].iterations;
            if (q.infos[k].rc == BF_OK) g.models[k] = q.models[k];
            else if (q.infos[k].rc == BF_ERR_CAPACITY && helper) large.push_back(k);
        }
        if (large.empty()) return BF_OK;
        ObjectTasks one;
        one.opts = fit;
        one.force_host = true;
        for (size_t k : large) one.push(ids[k], &g.models[k]);
        rc = one.run(helper, s.fr_x, s.fr_y, s.t_ns, s.n);
        if (rc < 0) return rc;
        for (size_t j = 0; j < large.size(); ++j) {
            iterations[large[j]] = one.infos[j].iterations;
            if (one.infos[j].rc == BF_OK) g.models[large[j]] = one.models[j];
        }
        return BF_OK;
    }
};

}  // namespace bf

#endif  // BF_HOST_OBJECT_TASKS_H
