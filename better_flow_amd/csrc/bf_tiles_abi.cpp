// bf_tiles_abi.cpp -- C-ABI: optimizers over parts of one uploaded slice -- the grid of per-tile optimizers (BASELINE config 4:
// bf_run_tiles, bf_run_tiles_many), the grid of contrast-score windows (bf_local_run_tiles) and the queue of event groups
// (bf_set_groups, bf_set_groups_from_segments, bf_run_groups).  All of them sort the slice's events into the other event set, by
// sensor tile or by group, and run one work-group per part on its own events; what they share is stated once below.
#include "bf_ctx.h"

namespace {

// The option checks of a sorted run (`who`: the entry's name in the one text that names it); Opts: bf_tile_opts / bf_group_opts.
template <class Opts> int sorted_run_check(bf_ctx* c, const char* who, const Opts& o) {
    if (o.scale < 1 || o.scale % 2 == 0 || o.scale / 2 > kMaxHalfScale) return fail(c, BF_ERR_ARG, "scale must be odd");
    if (o.sensor_res_x < 1 || o.sensor_res_y < 1) return fail(c, BF_ERR_ARG, "bad sensor size");
    if (c->has_noise) return fail(c, BF_ERR_ARG, "%s does not take a noise mask", who);
    return BF_OK;
}

// The second event set and the counting sort's histogram (zeroed on stream `s` when new), starts and cursors for nb buckets.
int sort_buffers(bf_ctx* c, int nb, hipStream_t s) {
    const int rc = ensure_second_set(c);
    if (rc != BF_OK) return rc;
    bool fresh;
    HIP_TRY(c, c->d_tile_hist.grow((size_t)nb + 1, &fresh));
    if (fresh) HIP_TRY(c, hipMemsetAsync(c->d_tile_hist, 0, (size_t)(nb + 1) * 4, s));
    HIP_TRY(c, c->d_tile_start.grow((size_t)nb + 1));
    HIP_TRY(c, c->d_tile_cursor.grow((size_t)nb + 1));
    return BF_OK;
}

// A fresh OptimizerRolling with a zero model, as a device state.
template <class Opts> DevState reset_state(const Opts& o) {
    DevState tmpl;
    memset(&tmpl, 0, sizeof(tmpl));
    tmpl.x_div = tmpl.y_div = 1.0f;           // optimizer_rolling.h:61-63
    tmpl.rot_div = tmpl.div_div = 10000.0f;
    tmpl.max_iter = o.max_iter;
    tmpl.hard_cap = o.hard_iter_cap;
    tmpl.hot.wp = identity_warp();
    return tmpl;
}

// The optimizer launch's arguments: the sorted events in `dst`, their parts' starts in d_tile_start, the states in d_tile_states.
template <class Opts> TileArgs tile_args(bf_ctx* c, const bf_ctx::EvSet& dst, const Opts& o, long long max_px) {
    TileArgs a;
    a.xy = dst.xy; a.t = dst.t; a.p = dst.p; a.perm = dst.perm;
    a.nxny = c->d_nxny;
    a.tile_start = c->d_tile_start;
    a.states = c->d_tile_states;
    a.scale = o.scale;
    a.seed_res_x = o.sensor_res_x; a.seed_res_y = o.sensor_res_y;
    a.guard_res_x = o.guard_res_x; a.guard_res_y = o.guard_res_y;
    a.min_events = o.min_events;
    a.max_px = (int32_t)max_px;
    return a;
}

// Everything of bf_run_tiles ahead of the optimizer launch, on stream `s` (the context's own, or the batch's): buffers, the
// tiles' zero-model states, the counting sort of the slice's events by sensor tile.  Fills the launch's arguments.
int tiles_prepare(bf_ctx* c, const bf_tile_opts* o, hipStream_t s, TileArgs& a, bool rolling = true) {
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_run_tiles before bf_upload_events");
    if (o->grid_rows < 1 || o->grid_cols < 1 || (long long)o->grid_rows * o->grid_cols > 16384)
        return fail(c, BF_ERR_ARG, "bad tile grid %d x %d", o->grid_rows, o->grid_cols);
    int rc = sorted_run_check(c, "bf_run_tiles", *o);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int nt = o->grid_rows * o->grid_cols;
    if ((rc = sort_buffers(c, nt, s)) != BF_OK) return rc;
    HIP_TRY(c, c->d_tile_states.grow((size_t)nt));
    // LDS image capacity: the largest window a tile can have
    const int tr = (o->sensor_res_x + o->grid_rows - 1) / o->grid_rows + 1;
    const int tc = (o->sensor_res_y + o->grid_cols - 1) / o->grid_cols + 1;
    const long long max_px = (long long)(o->scale * tr + o->scale) * (o->scale * tc + o->scale);
    if (rolling && max_px * 16 > 156 * 1024)   // (the rolling optimizer's planes; bf_local_run_tiles sizes its own window)
        return fail(c, BF_ERR_CAPACITY, "a tile window of up to %lld pixels does not fit the LDS", max_px);

    launch_fill_states(c->d_tile_states, reset_state(*o), nt, s);

    TileGrid g;
    g.rows = o->grid_rows; g.cols = o->grid_cols; g.res_x = o->sensor_res_x; g.res_y = o->sensor_res_y;
    const bf_ctx::EvSet& src = c->set[c->cs];
    const bf_ctx::EvSet& dst = c->set[c->cs ^ 1];
    {
        ProfScope ps(c, 3);
        if (launch_tile_sort(src.xy, src.t, c->has_perm ? src.perm : nullptr, c->n, g, c->d_tile_hist, c->d_tile_start,
                             c->d_tile_cursor, dst.xy, dst.t, dst.p, dst.perm, s) != 0)
            return fail(c, BF_ERR_HIP, "cannot configure the tile sort for %d tiles", nt);
    }
    // The sort is enqueued: from here on the events ARE in the other set, sorted by sensor tile, whatever becomes of the rest of
    // the call.  So plan_slice's bin grids are given up here, with the set flip, and not at the read-back as they once were: a
    // call refused or failed in between (a window too large for the LDS in bf_local_run_tiles, a later slice of
    // bf_run_tiles_many refused, a HIP error) must not leave a context that claims image-tile bins for events sorted otherwise.
    c->sorted_outside_plan();
    a = tile_args(c, dst, *o, max_px);
    return BF_OK;
}

// The tiles' final states (already on the host) into the caller's arrays, and the context's flags after a tile run.
void tiles_collect(bf_ctx* c, const std::vector<DevState>& st, int nt, bf_model* models_out, bf_run_info* infos_out) {
    for (int i = 0; i < nt; ++i) {
        if (models_out) models_out[i] = st[(size_t)i].model;
        if (infos_out) {
            bf_run_info inf;
            memset(&inf, 0, sizeof(inf));
            inf.rc = st[(size_t)i].rc;
            inf.iterations = st[(size_t)i].hot.it;
            inf.x_divider = st[(size_t)i].x_div; inf.y_divider = st[(size_t)i].y_div;
            inf.rot_divider = st[(size_t)i].rot_div; inf.div_divider = st[(size_t)i].div_div;
            infos_out[i] = inf;
        }
    }
    c->tile_run_collected();   // per-event read-back (bf_compute_uv / bf_writeout_events) is valid now
}

// One wide group of bf_run_groups ("groups_wide", include/bf_accel.h): slots beg .. beg + n of the sorted set `dst` through the
// chip-wide loop on the inner context -- gather, bf_upload_events_device, bf_set_cloud, bf_set_model when warm, bf_run with the
// group options' mapping (object_tasks.h: ObjectTasks::run), and the per-event results back into the outer context.  Everything
// is enqueued on the one stream both contexts use.  BF_ERR_NOCONV of a run that ended is the group's own outcome (out.info.rc);
// any other inner error fails the call with the inner message.
struct WideResult {
    bf_model model;
    bf_run_info info;
};
int run_wide_group(bf_ctx* c, const bf_ctx::EvSet& dst, const bf_group_opts& o, int g, uint32_t beg, uint32_t n, const bf_model* warm,
                   WideResult& out) {
    int rc = ensure_wide_inner(c);
    if (rc != BF_OK) return rc;
    bf_ctx* in = c->wide_inner;
    auto inner_failed = [&](int code, const char* step) {
        char msg[sizeof(in->err)];
        snprintf(msg, sizeof(msg), "%s", bf_last_error(in));
        return fail(c, code, "bf_run_groups: wide group %d, %s: %s", g, step, msg);
    };
    bf_ctx::UploadSlot& stage = in->up.slot[0];   // (the blocking uploads' columns: the inner context takes no asynchronous upload)
    launch_group_gather(dst.xy, dst.t, beg, n, stage.x, stage.y, stage.t, c->stream);
    HIP_TRY(c, hipGetLastError());
    if ((rc = bf_upload_events_device(in, stage.x, stage.y, stage.t, (int64_t)n)) != BF_OK) return inner_failed(rc, "upload");
    if ((rc = bf_set_cloud(in, o.scale, o.sensor_res_x, o.sensor_res_y, nullptr)) != BF_OK) return inner_failed(rc, "bf_set_cloud");
    if (warm && (rc = bf_set_model(in, warm)) != BF_OK) return inner_failed(rc, "bf_set_model");
    bf_run_opts ro;
    bf_run_opts_default(&ro);
    ro.max_iter = o.max_iter;
    ro.min_events = o.min_events;
    ro.res_x = o.guard_res_x; ro.res_y = o.guard_res_y;
    ro.hard_iter_cap = o.hard_iter_cap;
    memset(&out, 0, sizeof(out));
    out.info.iterations = -1;   // (a run that ends says how many it took)
    rc = bf_run(in, &ro, &out.model, &out.info);
    const bool ended = out.info.iterations >= 0;
    if (!(rc == BF_OK || rc == BF_SKIPPED || (rc == BF_ERR_NOCONV && ended))) return inner_failed(rc, "bf_run");
    // what bf_writeout_events would read on the inner context: a warp still pending applied, then the products in the inner
    // order and (nx, ny) wherever the run left them
    if ((rc = flush_pending(in)) != BF_OK) return inner_failed(rc, "the pending warp");
    const bf_ctx::EvSet& is = in->set[in->cs];
    WideBack b;
    b.in_perm = in->has_perm ? is.perm.get() : nullptr;
    b.in_p = is.p;
    b.in_nxny = in->n_valid ? in->d_nxny.get() : nullptr;
    b.in_nxny_by_slot = (in->out_sorted && in->has_perm) ? 1 : 0;
    b.beg = beg; b.n = n;
    b.out_perm = dst.perm;
    b.out_p = dst.p;
    b.out_nxny = c->d_nxny;
    launch_group_scatter_back(b, c->stream);
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

}  // namespace

extern "C" {

int bf_run_tiles(bf_ctx* c, const bf_tile_opts* o, bf_model* models_out, bf_run_info* infos_out) {
    if (!c || !o) return BF_ERR_ARG;
    TileArgs a;
    int rc = tiles_prepare(c, o, c->stream, a);
    if (rc != BF_OK) return rc;
    const int nt = o->grid_rows * o->grid_cols;
    {
        ProfScope ps(c, 0, c->n);
        if (launch_tile_optimizer(a, nt, c->stream) != 0) return fail(c, BF_ERR_HIP, "cannot configure the tile kernel");
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<DevState> st((size_t)nt);
    HIP_TRY(c, hipMemcpyAsync(st.data(), c->d_tile_states, (size_t)nt * sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    tiles_collect(c, st, nt, models_out, infos_out);
    return BF_OK;
}

// The tile grids of n slices -- one per context, each uploaded -- in ONE launch on the first context's stream
// (k_tile_optimizer_many): work-groups claim (slice, tile) pairs from a device counter, so the straggler tiles of the first
// slices run under the bulk of the later ones without a stream (and a hardware queue) per slice.
int bf_run_tiles_many(bf_ctx* const* ctxs, int32_t n, const bf_tile_opts* o, bf_model* models_out, bf_run_info* infos_out) {
    if (!ctxs || n < 1 || !o || !ctxs[0]) return BF_ERR_ARG;
    bf_ctx* lead = ctxs[0];
    if (n > 4096) return fail(lead, BF_ERR_ARG, "at most 4096 slices per call (got %d)", n);
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return fail(lead, BF_ERR_ARG, "context %d is NULL", i);
        if (ctxs[i]->device != lead->device) return fail(lead, BF_ERR_ARG, "context %d lives on another device", i);
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return fail(lead, BF_ERR_ARG, "context %d appears twice (one slice per context)", i);
    }
    HIP_TRY(lead, hipSetDevice(lead->device));
    const int nt = o->grid_rows * o->grid_cols;
    HIP_TRY(lead, lead->d_many_args.grow((size_t)n * sizeof(TileArgs) + 64));
    HIP_TRY(lead, lead->h_many_args.grow((size_t)n));
    TileArgs* host_args = lead->h_many_args;
    TileArgs* dev_args = reinterpret_cast<TileArgs*>(lead->d_many_args.get());
    uint32_t* counter = reinterpret_cast<uint32_t*>(dev_args + n);   // (not owned: the claim counter behind the arguments)
    // every slice's preparation on the lead's stream, behind whatever its own context's stream still holds for it
    for (int i = 0; i < n; ++i) {
        bf_ctx* c = ctxs[i];
        if (c != lead) {
            HIP_TRY(c, hipEventRecord(c->poll_ev[0], c->stream));
            HIP_TRY(lead, hipStreamWaitEvent(lead->stream, c->poll_ev[0], 0));
        }
        TileArgs a;
        const int rc = tiles_prepare(c, o, lead->stream, a);
        if (rc != BF_OK) {
            if (c != lead) fail(lead, rc, "slice %d: %s", i, c->err);
            (void)hipStreamSynchronize(lead->stream);
            return rc;
        }
        host_args[i] = a;
    }
    HIP_TRY(lead, hipMemcpyAsync(dev_args, host_args, (size_t)n * sizeof(TileArgs), hipMemcpyHostToDevice, lead->stream));
    HIP_TRY(lead, hipMemsetAsync(counter, 0, sizeof(uint32_t), lead->stream));
    {
        long long ev = 0;
        for (int i = 0; i < n; ++i) ev += ctxs[i]->n;
        ProfScope ps(lead, 0, ev);
        if (launch_tile_optimizer_many(dev_args, n, nt, o->scale, host_args[0].max_px, counter, lead->n_cus, lead->stream) != 0)
            return fail(lead, BF_ERR_HIP, "cannot configure the tile kernel");
    }
    HIP_TRY(lead, hipGetLastError());
    std::vector<DevState> st((size_t)n * (size_t)nt);
    for (int i = 0; i < n; ++i)
        HIP_TRY(lead, hipMemcpyAsync(st.data() + (size_t)i * nt, ctxs[i]->d_tile_states, (size_t)nt * sizeof(DevState),
                                     hipMemcpyDeviceToHost, lead->stream));
    HIP_TRY(lead, hipStreamSynchronize(lead->stream));   // (everything of every slice is complete: the other contexts' streams need no event)
    for (int i = 0; i < n; ++i) {
        std::vector<DevState> one(st.begin() + (size_t)i * nt, st.begin() + (size_t)(i + 1) * nt);
        tiles_collect(ctxs[i], one, nt, models_out ? models_out + (size_t)i * nt : nullptr, infos_out ? infos_out + (size_t)i * nt : nullptr);
    }
    return BF_OK;
}

// A grid of OptimizerLocal windows, one per sensor tile, each on the tile's own events (k_local_tile_optimizer, bf_local.hip).
int bf_local_run_tiles(bf_ctx* c, const bf_local_tile_opts* o, bf_local_state* states_out, int32_t* rc_out) {
    if (!c || !o) return BF_ERR_ARG;
    if (o->wsz < 1) return fail(c, BF_ERR_ARG, "wsz must be >= 1");
    if (o->scale < 1 || o->scale % 2 == 0 || o->scale > 7)   // optimizer_sampler.cpp:206 (odd); the Gaussian is stated to 7
        return fail(c, BF_ERR_ARG, "scale must be odd and <= 7 (got %d)", o->scale);
    bf_tile_opts to;
    memset(&to, 0, sizeof(to));
    to.grid_rows = o->grid_rows; to.grid_cols = o->grid_cols; to.scale = o->scale;
    to.sensor_res_x = o->sensor_res_x; to.sensor_res_y = o->sensor_res_y;
    to.guard_res_x = o->guard_res_x; to.guard_res_y = o->guard_res_y;
    TileArgs ta;
    int rc = tiles_prepare(c, &to, c->stream, ta, false);   // (the counting sort by sensor tile; the rolling optimizers' states are not used)
    if (rc != BF_OK) return rc;
    const int nt = o->grid_rows * o->grid_cols;
    HIP_TRY(c, c->d_ltile.grow((size_t)nt * (sizeof(bf_local_state) + sizeof(int32_t))));
    bf_local_state* d_states = reinterpret_cast<bf_local_state*>(c->d_ltile.get());
    int32_t* d_rcs = reinterpret_cast<int32_t*>(d_states + nt);   // (not owned: behind the states in d_ltile)
    TileGrid g;
    g.rows = o->grid_rows; g.cols = o->grid_cols; g.res_x = o->sensor_res_x; g.res_y = o->sensor_res_y;
    {
        ProfScope ps(c, 0, c->n);
        const int lr = launch_local_tile_optimizer(ta.xy, ta.t, ta.tile_start, d_states, d_rcs, g, o->scale, o->wsz, o->guard_res_x,
                                                   o->guard_res_y, (long long)o->max_evaluations, c->stream);
        if (lr == -3) return fail(c, BF_ERR_CAPACITY, "a window of %d x %d pixels does not fit the LDS", o->scale * o->wsz + o->scale, o->scale * o->wsz + o->scale);
        if (lr != 0) return fail(c, BF_ERR_HIP, "cannot configure the window kernel");
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<bf_local_state> st((size_t)nt);
    std::vector<int32_t> rcs((size_t)nt);
    HIP_TRY(c, hipMemcpyAsync(st.data(), d_states, (size_t)nt * sizeof(bf_local_state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rcs.data(), d_rcs, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < nt; ++i) {
        if (states_out) states_out[i] = st[(size_t)i];
        if (rc_out) rc_out[i] = rcs[(size_t)i];
    }
    // the events are now sorted by sensor tile (reset products, permutation kept); no per-event result was written
    c->local_tile_run_collected();
    return BF_OK;
}

// ---- Event groups: the reference's queue of (events, model) tasks over one uploaded slice (bf_accel.h, "event groups") ----

int bf_set_groups(bf_ctx* c, const int32_t* group_id, int32_t groups) {
    if (!c) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_set_groups before bf_upload_events");
    if (groups < 0 || (c->n > 0 && !group_id)) return fail(c, BF_ERR_ARG, "bf_set_groups: %d groups, ids %p", groups, (const void*)group_id);
    if ((long long)groups + 1 > 16384) return fail(c, BF_ERR_CAPACITY, "bf_set_groups: %d groups + 1 exceed the sort's 16384 buckets", groups);
    for (long long i = 0; i < c->n; ++i)
        if (group_id[i] < -1 || group_id[i] >= groups)
            return fail(c, BF_ERR_ARG, "bf_set_groups: event %lld has id %d outside -1 .. %d", i, group_id[i], groups - 1);
    HIP_TRY(c, hipSetDevice(c->device));
    return install_grouping(c, group_id, hipMemcpyHostToDevice, groups);
}

int bf_set_groups_from_segments(bf_ctx* c, int32_t* groups_out) {
    if (!c) return BF_ERR_ARG;
    if (!c->seg_valid || c->pending_warp || !c->have_window)
        return fail(c, BF_ERR_STATE, "bf_set_groups_from_segments: no segmentation of the current window is held");
    if ((long long)c->seg_K + 1 > 16384)
        return fail(c, BF_ERR_CAPACITY, "bf_set_groups_from_segments: %d components + 1 exceed the sort's 16384 buckets", c->seg_K);
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = install_grouping(c, c->d_seg_cl, hipMemcpyDeviceToDevice, c->seg_K);   // (the context's own plane: the grouping outlives the segmentation)
    if (rc != BF_OK) return rc;
    if (groups_out) *groups_out = c->seg_K;
    return BF_OK;
}

int bf_run_groups(bf_ctx* c, const bf_group_opts* o, const bf_model* warm, int32_t warm_count, bf_model* models_out,
                  bf_run_info* infos_out, bf_group_info* groups_out) {
    if (!c || !o) return BF_ERR_ARG;
    if (!c->uploaded) return fail(c, BF_ERR_STATE, "bf_run_groups before bf_upload_events");
    if (!c->groups_valid) return fail(c, BF_ERR_STATE, "bf_run_groups: no grouping of the uploaded slice is held");
    const int K = c->groups_K;
    int rc = sorted_run_check(c, "bf_run_groups", *o);
    if (rc != BF_OK) return rc;
    if (!(warm_count == 0 || warm_count == 1 || warm_count == K) || (warm_count > 0 && !warm))
        return fail(c, BF_ERR_ARG, "bf_run_groups: %d warm models for %d groups (0, 1 or one per group)", warm_count, K);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int nb = K + 1;   // buckets: the groups, then the events of none
    if ((rc = sort_buffers(c, nb, s)) != BF_OK) return rc;
    HIP_TRY(c, c->d_tile_states.grow((size_t)(K > 0 ? K : 1)));
    HIP_TRY(c, c->d_group_box.grow((size_t)(K > 0 ? K : 1) * 4));
    HIP_TRY(c, c->d_group_order.grow((size_t)(K > 0 ? K : 1)));
    HIP_TRY(c, c->d_group_counter.grow(1));

    const bf_ctx::EvSet& src = c->set[c->cs];
    const bf_ctx::EvSet& dst = c->set[c->cs ^ 1];
    {
        ProfScope ps(c, 3);
        if (launch_group_sort(src.xy, src.t, c->has_perm ? src.perm : nullptr, c->n, c->d_group_id, K, c->d_tile_hist,
                              c->d_tile_start, c->d_tile_cursor, dst.xy, dst.t, dst.p, dst.perm, s) != 0)
            return fail(c, BF_ERR_HIP, "cannot configure the sort for %d groups", K);
        launch_group_boxes(dst.xy, dst.perm, c->d_group_id, c->d_tile_start, c->n, K, c->d_group_box, s);
    }
    HIP_TRY(c, hipGetLastError());
    c->sorted_outside_plan();   // (deliberately here, not at the read-back: see tiles_prepare)

    // the groups' event counts and boxes: what the windows will be, which of them run, the LDS they need
    std::vector<uint32_t> start((size_t)nb + 1);
    std::vector<int32_t> box((size_t)K * 4);
    HIP_TRY(c, hipMemcpyAsync(start.data(), c->d_tile_start, ((size_t)nb + 1) * 4, hipMemcpyDeviceToHost, s));
    if (K > 0) HIP_TRY(c, hipMemcpyAsync(box.data(), c->d_group_box, (size_t)K * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const int sc = o->scale;
    long long max_px = 1;
    std::vector<bf_group_info> gi((size_t)K);
    std::vector<int> wide;   // the groups the chip-wide loop solves (bf_rules::group_route)
    c->groups_wide = 0;
    for (int g = 0; g < K; ++g) {
        const int n = (int)(start[(size_t)g + 1] - start[(size_t)g]);
        int x_min = o->sensor_res_x, y_min = o->sensor_res_y, x_max = 0, y_max = 0;   // optimizer_rolling.h:252-253
        if (n > 0) {
            x_min = std::min(x_min, box[4 * (size_t)g]); x_max = std::max(x_max, box[4 * (size_t)g + 1]);
            y_min = std::min(y_min, box[4 * (size_t)g + 2]); y_max = std::max(y_max, box[4 * (size_t)g + 3]);
        }
        const int R = sc * (x_max - x_min) + sc, C = sc * (y_max - y_min) + sc;
        bf_group_info& q = gi[(size_t)g];
        memset(&q, 0, sizeof(q));
        q.events = n;
        q.row_min = x_min; q.row_max = x_max; q.col_min = y_min; q.col_max = y_max;
        q.rows = R; q.cols = C;
        // where the group is solved: a group the guards skip needs no planes, the launch's LDS is the largest window that runs
        // in it, a wide group is marked for the caller
        bf_rules::GroupFacts f;
        f.rows = R; f.cols = C; f.events = n; f.scale = sc;
        f.guard_res_x = o->guard_res_x; f.guard_res_y = o->guard_res_y; f.min_events = o->min_events;
        f.lds_budget = kGroupLdsBudget;
        f.max_rows = c->max_rows; f.max_cols = c->max_cols;
        f.wide = c->opt_groups_wide;
        const bf_rules::GroupRoute route = bf_rules::group_route(f);
        if (route.path == bf_rules::GroupPath::lds) max_px = std::max(max_px, route.lds_bytes / 16);
        if (route.path == bf_rules::GroupPath::wide) {
            wide.push_back(g);
            q.reserved = 1;
        }
    }
    if (groups_out) for (int g = 0; g < K; ++g) groups_out[g] = gi[(size_t)g];

    if (K > 0) {
        const DevState tmpl = reset_state(*o);
        auto warm_state = [&](const bf_model& m) {   // bf_set_model (optimizer_rolling.h:289-299) on the reset state
            DevState w = tmpl;
            w.model = m;
            set_model_warp(w.hot.wp, m);
            return w;
        };
        // the claim order: descending event count, so that the longest loops start first
        std::vector<uint32_t> order((size_t)K);
        for (int g = 0; g < K; ++g) order[(size_t)g] = (uint32_t)g;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return gi[a].events > gi[b].events; });
        HIP_TRY(c, hipMemcpyAsync(c->d_group_order, order.data(), (size_t)K * 4, hipMemcpyHostToDevice, s));
        std::vector<DevState> warm_st;
        if (warm_count == K && K > 1) {
            warm_st.resize((size_t)K);
            for (int g = 0; g < K; ++g) warm_st[(size_t)g] = warm_state(warm[g]);
            HIP_TRY(c, hipMemcpyAsync(c->d_tile_states, warm_st.data(), (size_t)K * sizeof(DevState), hipMemcpyHostToDevice, s));
        } else {
            launch_fill_states(c->d_tile_states, warm_count > 0 ? warm_state(warm[0]) : tmpl, K, s);
        }
        HIP_TRY(c, hipStreamSynchronize(s));   // (order and warm_st are pageable and leave scope below)
        HIP_TRY(c, hipMemsetAsync(c->d_group_counter, 0, sizeof(uint32_t), s));

        const TileArgs a = tile_args(c, dst, *o, max_px);   // (the largest window that runs: the others are skipped, or BF_ERR_CAPACITY in their own rc)
        ProfScope ps(c, 0, c->n);
        int per_cu = 0;
        if (launch_group_optimizer(a, c->d_group_order, K, warm_count > 0, c->d_group_counter, c->n_cus, s, &per_cu) != 0)
            return fail(c, BF_ERR_HIP, "cannot configure the group kernel");
        c->groups_lds = (int)(max_px * 16);
        c->groups_per_cu = per_cu;
    }
    // the wide groups, one after the other behind the LDS groups' launch (which left them what set_model left), longest first
    std::stable_sort(wide.begin(), wide.end(), [&](int a, int b) { return gi[(size_t)a].events > gi[(size_t)b].events; });
    std::vector<WideResult> wres(wide.size());
    for (size_t k = 0; k < wide.size(); ++k) {
        const int g = wide[k];
        const bf_model* wm = warm_count == 0 ? nullptr : &warm[warm_count == K ? g : 0];
        if ((rc = run_wide_group(c, dst, *o, g, start[(size_t)g], (uint32_t)gi[(size_t)g].events, wm, wres[k])) != BF_OK) return rc;
    }
    c->groups_wide = (int)wide.size();
    launch_group_rest(dst.perm, c->d_tile_start, K, c->d_nxny, s);
    HIP_TRY(c, hipGetLastError());
    std::vector<DevState> st((size_t)K);
    if (K > 0) HIP_TRY(c, hipMemcpyAsync(st.data(), c->d_tile_states, (size_t)K * sizeof(DevState), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    tiles_collect(c, st, K, models_out, infos_out);
    for (size_t k = 0; k < wide.size(); ++k) {   // the inner run's outcome in place of the kernel's BF_ERR_CAPACITY
        if (models_out) models_out[wide[k]] = wres[k].model;
        if (infos_out) infos_out[wide[k]] = wres[k].info;
    }
    return BF_OK;
}

}  // extern "C"
