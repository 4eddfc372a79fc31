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
// groups").  No membership policy lives here: which events form an object is the caller's decision.
#ifndef BF_HOST_OBJECT_TASKS_H
#define BF_HOST_OBJECT_TASKS_H

#include <bf_accel.h>

#include <cstdint>
#include <cstring>
#include <vector>

// (weak: the host classes also link against C-ABI implementations that lack them, as in flow_field.h and clustering.h)
extern "C" {
int bf_set_groups(bf_ctx *ctx, const int32_t *group_id, int32_t groups) __attribute__((weak));
int bf_set_groups_from_segments(bf_ctx *ctx, int32_t *groups_out) __attribute__((weak));
int bf_run_groups(bf_ctx *ctx, const bf_group_opts *opts, const bf_model *warm, int32_t warm_count, bf_model *models_out,
                  bf_run_info *infos_out, bf_group_info *groups_out) __attribute__((weak));
}

namespace bf {

class ObjectTasks {
  public:
    bf_group_opts opts;                   // scale, set_cloud's seeds, run()'s guards and caps: shared by the tasks
    // what run() leaves: one entry per task, and (nx, ny) per event of the slice (0 for an event of no task)
    std::vector<bf_model> models;
    std::vector<bf_run_info> infos;
    std::vector<double> nx, ny;
    bool wide = false;                    // device path: "groups_wide" = 1 for its bf_run_groups (the host path has no LDS limit)

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

    // Solves the queue on the slice (fr_x, fr_y, t_ns)[n]; ctx: a context with room for n events.  force_host: the host path
    // even where the library has the device entries.  Returns BF_OK or the first error of the C-ABI; a task's own outcome
    // (BF_OK, BF_SKIPPED, BF_ERR_NOCONV, BF_ERR_CAPACITY) is in infos[k].rc.
    int run(bf_ctx *ctx, const int32_t *fr_x, const int32_t *fr_y, const int32_t *t_ns, size_t n, bool force_host = false) {
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
            int rc = bf_upload_events(ctx, fr_x, fr_y, t_ns, nullptr, (int64_t)n);
            if (rc >= 0) rc = bf_set_groups(ctx, gid.data(), (int32_t)K);
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
        std::vector<double> snx, sny;
        for (size_t k = 0; k < K; ++k) {
            // the task's events in the slice's order, whatever order they were pushed in
            sx.clear(); sy.clear(); st.clear();
            std::vector<size_t> where;
            for (size_t i = 0; i < n; ++i)
                if (gid[i] == (int32_t)k) {
                    where.push_back(i);
                    sx.push_back(fr_x[i]); sy.push_back(fr_y[i]); st.push_back(t_ns[i]);
                }
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

}  // namespace bf

#endif  // BF_HOST_OBJECT_TASKS_H
