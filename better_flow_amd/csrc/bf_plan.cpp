// bf_plan.cpp -- which loop a slice runs: bin grids and scatter format per slice (plan_slice), loop form, home of the update and
// scatter sizing per run (plan_run).  Every rule is a measured crossover, and the measurement stands next to it.
#include "bf_ctx.h"

SlicePlan plan_slice(const bf_ctx* c, const bf_window& w) {
    SlicePlan p;
    const int scale = w.scale;
    // Tile-binned scatter: usable when there is no noise mask and the bin grid fits the kernels' LDS.  Its own
    // per-bin packing is decided on the device by the counting sort (k_bin_scan), with the overflow path as fallback.
    BinGrid& g = p.grid;
    // Tile shape: one work-group per bin.  Cost model of one iteration (calibrated on config 2, in us):
    //   waves of work-groups x events per tile x 1.7 ns   (the fullest CU sets the length of the scatter kernel)
    // + slab pixels x 2.3 ps                               (every slab pixel is written and re-read)
    // over widths {16, 32, 64} (a power of two) and heights {32 .. 128}; ties go to the larger tile.  Small dense
    // images get small tiles (enough bins to fill the CUs), large images large ones (less margin overhead).
    // (the margin: kBinMargin, even; BF_DEBUG_MARGIN overrides it for tests)
    const int bin_margin = bf_rules::bin_margin(c->dbg_margin);
    const bf_rules::BinShape shape = bf_rules::bin_shape(c->n, w.scale_img_x, w.scale_img_y, c->n_cus, bin_margin);
    g.TS = shape.TS;
    g.TSR = shape.TSR;
    g.lg = 0;
    while ((1 << g.lg) < g.TS) ++g.lg;
    g.nbc = shape.nbc;
    g.D = shape.D;   // <= 2 x 2 bins per pixel
    g.L = g.TS + 2 * g.D;
    g.LR = g.TSR + 2 * g.D;
    g.mul_r = (uint32_t)(0x100000000ull / (unsigned)g.TSR) + 1u;
    g.mul_l = (uint32_t)(0x100000000ull / (unsigned)g.L) + 1u;
    g.mul_h = (uint32_t)(0x100000000ull / (unsigned)(g.L / 2 > 0 ? g.L / 2 : 1)) + 1u;
    g.nbr = shape.nbr;
    g.nbins = shape.nbins;
    // Density rule: every iteration writes and re-reads one slab pixel (8 B x (L / TS)^2) per image pixel, a global
    // atomic costs ~48 ns per event; below ~1 event per 12 pixels the plain atomic scatter is the faster one
    // (measured: 300k events on a 3550 x 6350 image, 0.41 vs 0.66 ms per iteration).
    // ... on an image of tens of megapixels: the event-list form of the binned loop follows the events, and up to the
    // 8.3 M pixels of a 1280x720 sensor at scale 3 it beats the atomics for sparse slices too (20k .. 500k events:
    // 640x480 22 .. 28 us per iteration against 31 .. 40, 1280x720 48 .. 64 against 62 .. 86).
    const bool dense = (double)w.scale_img_x * (double)w.scale_img_y < 12.0 * (double)c->n ||
                       (double)w.scale_img_x * (double)w.scale_img_y <= 9.0e6;
    p.binned = (c->opt_binned == 2 || (c->opt_binned == 1 && dense)) && !c->force_split && !c->has_noise && c->n > 0 &&
               c->cap_events < (1ll << 29) &&   // (32-bit byte offsets into the event arrays: ld_idx)
               bf_rules::bin_grid_ok(shape, w.scale_img_x);
    // (<= 8192 bins x <= 156 KB: slabs, tiled image and margin plane stay below 2^31 bytes -- the stencil kernel's buffer loads
    // carry 32-bit byte offsets, buf_ld_u64)

    // The one-kernel iteration (k_fused_pass; used by bf_run unless the context is co-scheduled with others): image
    // tiles of 32 x 64 pixels -- 64 x 64 when the nine sort keys per tile would not fit the counting sort -- and a
    // margin D that keeps a tile's edge strips (H + D wide, H = scale / 2 + 1) from overlapping.
    // Where it pays (measured on MI355X, one context, cold runs; us per iteration fused / best two-kernel or atomic loop):
    //   240x180: 50k events 16.1 / 22.0, 200k 17.9 / 19.6, 400k 20.5 / 18.2;   346x260: 20k 16.0 / 17.1, 50k 15.9 / 19.6,
    //   100k 17.5 / 23.1, 200k 17.8 / 20.2, 400k 19.6 / 20.3, 1M 26.8 / 19.7;   640x480: 20k .. 400k 31 .. 38 / 22 .. 34.
    // The events of a tile's edge strips are warped by up to four work-groups (2.1 x the events at D = 8) and a
    // dense slice meets in few LDS words, so "auto" takes it for slices of at most one event per two image pixels on
    // images up to 1.2 M pixels; a launch chain half as long is what it buys there.
    const double Pimg = (double)w.scale_img_x * (double)w.scale_img_y;
    const bool fused_pays = Pimg <= 1.2e6 && 2.0 * (double)c->n <= Pimg;
    if ((c->opt_fused == 2 || (c->opt_fused == 1 && fused_pays)) && c->opt_binned != 0 && !c->force_split && !c->has_noise && c->n > 0 && scale / 2 <= 4 &&
        w.scale_img_x < (1 << 20) && (long long)c->n < (1ll << 31)) {
        BinGrid& f = p.fgrid;
        const int Hh = scale / 2 + 1;
        auto tiles = [&](int rows) { return ((w.scale_img_x + rows - 1) / rows) * ((w.scale_img_y + 63) / 64); };
        const int rows = tiles(32) * kFusedZones <= 8192 ? 32 : 64;
        int Dm = c->dbg_margin > 0 ? c->dbg_margin : kFusedMargin;
        if (Dm > rows / 2 - Hh) Dm = rows / 2 - Hh;
        if (Dm >= 1 && tiles(rows) * kFusedZones <= 8192) {
            f.TS = 64; f.lg = 6; f.TSR = rows; f.D = Dm; f.fz = Hh + Dm;
            f.nbc = (w.scale_img_y + 63) / 64;
            f.nbr = (w.scale_img_x + rows - 1) / rows;
            f.nbins = f.nbr * f.nbc * kFusedZones;   // sort keys
            f.mul_r = (uint32_t)(0x100000000ull / (unsigned)f.TSR) + 1u;
            p.fused_ok = true;
            // Contexts that share the GPU: with dense slices the two loop kernels are bandwidth-bound and the tail-update
            // form keeps the CUs full, so the two-kernel loop stays; sparse slices remain launch-bound even with eight
            // contexts in flight (346x260, 2 / 4 / 8 contexts: 50k events 12.4 / 11.4 / 10.6 us per iteration and slice
            // against 16.7 / 14.6 / 12.8; 200k events 11.8 / 9.3 / 9.4 against 13.3 / 9.2 / 9.1).
            p.fused_shared = c->opt_fused == 2 || 8.0 * (double)c->n <= Pimg;
        }
    }

    // Dense slabs or event lists.  A dense slice (one event per four pixels or more) merges its events in the bin's LDS
    // tile and writes the tile.  A sparse one writes lists, work and traffic following the events: one entry per EVENT
    // and no LDS tile (a 1280x720 sensor with 1M events -- the tile of such a bin would fill the CU's LDS and leave one
    // work-group per CU).  "auto" decides once per slice: the kernels are compiled per format.  Measured per iteration
    // (dense / events): 1280x720 scale 3: 90 / 68 us; 640x480 scale 3: 44 / 52.  (A third form -- lists merged per pixel
    // in the LDS tile, for small sensors at large scales: 346x260 scale 7 61 against 96 / 103 us -- was removed in round 5:
    // no BASELINE configuration took it, and every form multiplies the bit-identity matrix.)
    const bool lists_ok = p.binned && bf_rules::bin_format_ok(shape, 2);    // 16-bit tile-local pixel indices
    const int mode = lists_ok ? c->opt_bin_compact : 0;
    if (mode == 2 || (mode == 1 && 4.0 * (double)c->n < Pimg)) p.fmt = 2;
    // Dense slices: the bin's own pixels + a margin plane instead of whole-tile slabs (flush_split).  It moves 0.6 x the
    // slab bytes and a quarter of the stencil kernel's loads; "auto" takes it where that is what the iteration
    // waits for -- a context that has the GPU to itself (update at the scatter head) on an image of >= 1.5 M
    // pixels: 640x480 scale 3, 1M events: K1 14.7 -> 11.3 us, iteration 37.2 -> 32.9 us.  At 346x260 the loop is a
    // latency chain and nothing moves (18.8 us either way); with the update in the stencil tail ("co_schedule") the
    // lean scatter kernel LOSES 1.7 us per launch (8.0 -> 9.7 us at 346x260, value 196 -> 178 Mevents/s).
    const bool split_pays = !c->opt_co_schedule && Pimg >= 1.5e6;
    if (p.fmt == 0 && p.binned && (c->opt_bin_split == 2 || (c->opt_bin_split == 1 && split_pays)) &&
        bf_rules::bin_format_ok(shape, 3))   // (D a power of two)
        p.fmt = 3;
    // Event lists on 64-column bins (every sensor of BASELINE.json's configurations): entries sorted by (column zone,
    // row), so that a stencil tile gathers from the bins beside its own only the zone that faces it (bf_scatter.hip,
    // "event lists").  zw: the columns of a bin's tile a box sum of the neighbouring stencil tile can reach.
    if (p.fmt == 2 && g.TS == 64 && g.L >= 2 * (g.D + scale / 2 + 1)) p.zw = g.D + scale / 2 + 1;
    return p;
}

// The loop form and the update's home: bf_rules::loop_choice (bf_plan_rules.h) of the facts below.  Why its thresholds are what they are:
// One slice context alone on the GPU: the one-kernel iteration when the slice qualifies (plan_slice), else the
// two-kernel tile-binned loop when the slice is dense enough for it, else global atomics.
// The persistent form of the one-kernel loop (bf_loop.hip): the work-groups stay resident over many iterations and
// exchange their moment sums through memory -- for a context that has the GPU to itself (two such kernels from two
// contexts could each hold half of the CUs and wait for the other half), when all tiles can be resident at once.
// A cold run re-bins a dozen times in its first iterations, and every re-bin ends a launch of the persistent kernel with
// a host round trip (measured on 50 000 events, 240x180: 25 us per iteration against 17); a warm-started slice of a stream
// -- the reference's own mode, ~115 iterations and one or two re-bins -- is where it pays (11.1 against 12.2 us per
// iteration all in): "auto" takes it for warm starts.  (else: one launch per iteration)
// Delta scatter (bf_kernels.hip: k_warp_scatter_delta), a form of the global-atomic loop: any slice without a noise mask can
// take it, and it then stands in for whichever loop the slice would run.  "auto" takes it where it was measured against the
// loop it replaces (experiments/round_8.md): cold runs of contexts that share the GPU ("co_schedule") on slices that would
// run the two-kernel loop on dense slabs by "auto"'s own choice, with packed planes and at least one event per image pixel
// -- config 2 under four contexts 218 -> 240 Mevents/s: the loop is bound by bytes there, and the slab hand-off is half of
// them.  A context alone (a latency chain: 101.5 against 102 Mevents/s, no gain), warm starts (a handful of iterations
// would pay for a full first scatter of global atomics) and the event-list geometries keep their loops; so does a
// context whose loop an option forces.  Nor a run capped below 200 iterations: the run's first two launches -- the full
// scatter and the first warp, which moves every event -- cost ~0.3 ms more than the tile-binned loop's (max_iter = 10 under
// four contexts: 0.69 -> 1.03 ms per slice), and an iteration saves ~3 us.
// Where the model / loop update runs.  One slice context alone: at the head of the next warp+scatter launch (every
// work-group for itself; shortest iteration).  Several contexts sharing the GPU ("co_schedule"): in the last
// work-group of the stencil kernel -- a serial tail on ONE CU that the other contexts' kernels fill, instead of
// ~1.5 us on all 256 CUs.  (the one-kernel loop has no other form than the head)
// A third home ("sep_update", round 6): contexts that share the GPU run the lean scatter kernel and a stencil kernel that
// only ACCUMULATES (no drain of its atomics, no ticket, no serial tail), and the update is a kernel of its own
// (k_finish_update: one wave) ahead of every scatter launch, on ONE state buffer (nobody reads the state while that kernel
// writes it).  Bookkeeping -- accumulator parities, overflow slots, when a snapshot is behind a re-bin -- is the head
// form's.  A stencil work-group that has to see its fifteen atomics acknowledged and then wait for its ticket holds its LDS and a
// wave slot ~1 us longer -- 10 % of its life: with thousands of work-groups per launch (event lists: 8100 tiles at 1280x720)
// the third launch per iteration is the cheaper way (stencil kernel 42.7 -> 37.9 us under co_schedule, config 5's batch +2.7 %);
// with a few hundred (config 2: 752) the launch costs more than the tickets (bench 206.7 -> 200.9): "auto" takes it for event
// lists only.  Same bits either way.
bf_rules::LoopFacts loop_facts(const bf_ctx* c, int max_iter, bool for_run) {
    bf_rules::LoopFacts f;
    f.opt_binned = c->opt_binned; f.opt_fused = c->opt_fused; f.opt_persist = c->opt_persist; f.opt_delta = c->opt_delta;
    f.opt_sep_update = c->opt_sep_update; f.co_schedule = c->opt_co_schedule;
    f.pixels = (double)c->win.scale_img_x * (double)c->win.scale_img_y;
    f.n = c->n; f.max_iter = max_iter;
    f.has_noise = c->has_noise; f.packed = c->packed; f.warm = c->pending_warp; f.live_ctx = g_live_ctx[c->device & 63].load();
    f.grid_ok = c->use_binned; f.fused_ok = c->fused_ok; f.fused_shared = c->fused_shared; f.fmt = c->fmt;
    // (the device is asked -- an occupancy query, the kernel's code object loaded -- only where its answer decides: not for a run delta scatter takes)
    f.resident = !bf_rules::persistent_ok(f) || (for_run && bf_rules::delta_ok(f)) || fused_loop_resident(c->win.scale / 2, c->fgrid.TSR, c->n_cus, c->fgrid.nbr * c->fgrid.nbc);
    return f;
}

RunPlan plan_run(bf_ctx* c, const bf_run_opts& o) {
    RunPlan p;
    const bf_rules::LoopChoice choice = bf_rules::loop_choice(loop_facts(c, o.max_iter, true));
    p.form = choice.form; p.home = choice.home;
    // (g_live_ctx only knows this process: another process's kernels -- or anything else that keeps work-groups from becoming
    // resident -- shows as a launch that gives up after 0.2 s.  The context then stays away from the kernel for a while.)
    if (p.loop_kernel() && c->persist_skip > 0) { --c->persist_skip; p.form = RunPlan::Form::one_kernel; }
    // Tile-binned mode sorts the events by the tile of their CURRENT target, so a warm-start
    // warp (bf_set_model) is applied before the sort rather than inside the first iteration.
    p.warm_start = c->pending_warp;
    p.prewarp = p.bin_grid() && c->pending_warp;   // fused into the first counting sort (k_bin_count<true>)
    p.first_warp = c->pending_warp && !p.prewarp;
    // (the persistent loop re-bins AT the request -- it returns for it --, the other loops one or two batches of launches
    // after it: the same effective threshold)
    if (p.bin_grid()) p.drift_limit = c->opt_bin_predict ? (p.loop_kernel() ? 0.85 : 0.6) * (double)(p.one_kernel() ? c->fgrid.D : c->grid.D) : 1e300;
    // Work-group size of the scatter kernel (bf_rules::scatter_size).  Dense tiles: 1024 threads for a context that
    // has the GPU to itself and bins of thousands of events (8.0 against 8.9 us per launch at config 2; at 640x480, bins of
    // ~1500 events, 512 threads: 11.7 against 17.4 us), 512 for contexts sharing the GPU ("co_schedule": a
    // 1024-thread work-group with its 51 KB tile needs half a CU's wave slots free at once and waits for them while the other
    // contexts' kernels hold a few each -- 16.7 instead of 8.0 us under four contexts; with 512 threads 170 -> 190 Mevents/s).
    // Event lists over thousands of small bins -- 1280x720 at scale 3: 1620 bins of ~600 events, six per CU -- run 256-thread
    // work-groups (16.6 against 18.6 us per scatter launch there at 1 M events, 8.2 against 13.3 at 100 k); with a couple of
    // bins per CU -- 640x480, 540 bins -- 512 threads stay ahead (6.3 against 8.2).  (512 rather than 1024 where a bin holds a few
    // hundred events -- large images --: twice as many bins in flight per CU, 84 instead of 91 us per iteration at 1280x720.)
    if (p.two_kernel()) {
        // events a scatter thread keeps in flight:
        // (event lists: registers, not LDS, set the occupancy there -- two events per thread keep four work-groups on a
        // CU, and a bin above the pass size takes a second pass; measured at 1280x720: 512 x 2 69.8 us, 512 x 4 73.5)
        // (dense tiles: a pass should cover the AVERAGE bin, fuller bins take a second pass -- sizing it for 1.5 x the
        // average left half of every thread's slots empty at 640x480: 512 x 8 19.9 us, 512 x 4 15.3 us)
        // (... and between two and four, two up to 2.83 -- the geometric middle: bins of ~2100 events on 1024 threads ran
        // 15.3 us with four events per thread, half of every thread's slots empty, against 12.1 us with two and a second pass
        // for the fuller bins; measured at 1M events on 440 / 520 / 560 x 480 sensors)
        // (dense slabs on 512-thread work-groups with bins of thousands of events -- config 2 under "co_schedule": 272 bins, 3673
        // events on average, 4912 in the fullest -- : the pass covers the FULLEST bin, ~1.35 x the average; with 8 per thread two
        // thirds of the bins took a second pass: 8.45 -> 8.13 us per launch alone, 8.2 -> 7.8 under four contexts)
        // (event lists, update in the stencil tail, thousands of small bins on 256 threads -- 1280x720: 1620 bins, 608 events on average,
        // 877 in the fullest: four per thread cover every bin in one pass, 14.3-14.6 -> 13.5 us per launch; the head form, whose
        // registers also hold the update, loses with four: 14.8 -> 16.5)
        // (the arithmetic of all of the above: bf_plan_rules.h)
        const bf_rules::ScatterSize k1 = bf_rules::scatter_size(c->fmt, p.head(), c->grid.nbins, c->n, c->n_cus);
        p.bin_threads = k1.threads;
        p.ev_per_thread = k1.per_thread;
    }
    // A warm start that is expected to converge in a handful of iterations (the previous one did) is polled batch by batch,
    // the final warp riding along: "quick".  One that is expected to run long -- the reference's own ring: ~115 iterations per
    // warm-started slice -- is fed and polled like a cold run: two-iteration batches with a blocking poll each cost it a
    // host round trip every other iteration (22 instead of 14 us per iteration on a 50 000-event slice).
    p.quick_warm = p.warm_start && c->warm_iters_hint < 3 * o.poll_interval;
    // A tile-binned run that is not a quick warm start reads its progress from the pinned snapshot (bf_run.cpp: wait_snapshot).
    // ... and so does delta scatter, whose stencil kernel writes the same snapshot.
    p.snap_polled = (p.bin_grid() || p.kept_plane()) && !p.quick_warm;
    return p;
}
