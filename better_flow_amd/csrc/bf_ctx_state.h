// bf_ctx_state.h -- what a context knows about the slice it holds, as plain flags, and every change of them as a named transition:
// no bf_ctx, no HIP, nothing to include.  bf_ctx derives from SliceState, so the C-ABI files read `c->n_valid` as before; they
// WRITE the flags through the transitions below and nowhere else (a grep for `c->flag = ` finds this header only), so that two
// entries which do the same thing to the events cannot leave the context in two different states.
// tests/cpp/test_ctx_state.cpp walks every state these transitions can reach and holds it to the invariants the readers rely on.
#pragma once

namespace bf_state {

struct SliceState {
    // ---- the slice ----
    bool uploaded = false;           // a slice is held (bf_upload_events / a committed asynchronous upload)
    bool stats_valid = false;        // its k_prepare statistics are folded (bf_ctx::stats)
    bool all_noise = false;          // bf_run's window guard marked every event as noise
    // ---- the window ----
    bool have_window = false;        // bf_set_cloud ran on the slice (or a tile / group run left per-event results)
    bool degenerate = false;         // window with R <= 0 or C <= 0 (empty slice)
    bool pending_warp = false;       // bf_set_model's warp not applied yet
    // ---- the events and their per-event outputs ----
    bool p_clean = false;            // p is all zero (Event::reset state): set by the upload, cleared by any warp
    bool n_valid = false;            // d_nxny holds the n of the last warp
    bool uv_valid = false;           // d_uv holds compute_uv of that n (fused into bf_run's final warp)
    bool out_sorted = false;         // d_nxny (and d_uv) are in slot order: un-permute with set[cs].perm before reading back
    int cs = 0;                      // set holding the live events
    bool has_perm = false;           // set[cs] is permuted; perm[] gives the upload index
    // ---- which loops the slice may run (plan_slice, decided in bf_set_cloud) ----
    bool use_binned = false;
    bool fused_ok = false;
    bool fused_shared = false;       // ... and the one-kernel loop is also the one to take when the context shares the GPU
    // ---- what is held about the slice beside the events ----
    bool seg_valid = false;          // a segmentation of the current window (an upload, bf_set_cloud and every warp drop it)
    bool groups_valid = false;       // a grouping of the uploaded slice (every upload drops it)
    int groups_K = 0;
    bool glob_valid = false;         // bf_global_set_window ran on the slice uploaded now
    bool have_lwin = false;          // a window of the contrast-score optimiser

    // The events are in Event::reset state: zero products, no per-event output.
    void events_reset() { p_clean = true; n_valid = false; uv_valid = false; out_sorted = false; }
    // A warp moved the events and wrote (nx, ny) in upload order.
    void events_warped() { p_clean = false; seg_valid = false; n_valid = true; uv_valid = false; out_sorted = false; }

    // A new slice is staged in set[0] (k_prepare wrote p = 0).
    void slice_uploaded() {
        cs = 0; has_perm = false;
        events_reset();
        uploaded = true;
        stats_valid = false; all_noise = false;
        have_window = false; pending_warp = false;
        seg_valid = false; groups_valid = false; glob_valid = false; have_lwin = false;
    }
    void stats_folded() { stats_valid = true; }
    void all_noise_marked() { all_noise = true; }

    // bf_set_cloud gave the slice its window.  On a degenerate one nothing can be warped; a usable one starts from reset events.
    void window_set(bool degenerate_) {
        have_window = true; degenerate = degenerate_;
        pending_warp = false; seg_valid = false;
        if (!degenerate_) { all_noise = false; events_reset(); }
    }
    // plan_slice's decisions for that window: a decision, not a transition, but written here like everything else.
    void planned_binned(bool ok) { use_binned = ok; }
    void planned_one_kernel(bool ok) { fused_ok = ok; }
    void planned_one_kernel_shared(bool shared) { fused_shared = shared; }

    void warp_pending() { pending_warp = true; }                     // bf_set_model
    void pending_applied() { pending_warp = false; events_warped(); }   // flush_pending

    // bf_run: the loop warps the events (its first half, before anything is launched) ...
    void run_began() { p_clean = false; seg_valid = false; pending_warp = false; }
    // ... the device chose which set holds the tile-sorted events ...
    void sorted_by_plan(int set) { cs = set; has_perm = true; }
    // ... and its final warp left the outputs in slot order, the flow with them if asked for.
    void run_ended(bool want_uv) { n_valid = true; uv_valid = want_uv; out_sorted = true; }

    // Somebody other than the loop's plan sorted the events into the other set (by sensor tile, by group): the bin grids of
    // plan_slice no longer describe them.
    void sorted_outside_plan() { cs ^= 1; has_perm = true; use_binned = false; fused_ok = false; }
    // A tile or group run has been read back: every event warped by its tile's model, per-event read-back valid from here on.
    void tile_run_collected() { events_warped(); pending_warp = false; have_window = true; degenerate = false; }
    // A grid of contrast-score windows has been read back: reset products in sorted order, no per-event result, planes reused.
    void local_tile_run_collected() { events_reset(); pending_warp = false; have_lwin = false; }

    void outputs_materialised() { out_sorted = false; }   // d_nxny / d_uv un-permuted into upload order
    void uv_computed() { uv_valid = true; }
    void uv_buffer_reused() { uv_valid = false; }         // d_uv served as a staging buffer

    void segmentation_held() { seg_valid = true; }
    void segmentation_dropped() { seg_valid = false; }
    void grouping_held(int K) { groups_K = K; groups_valid = true; }
    void grouping_dropped() { groups_valid = false; }
    void local_window_held() { have_lwin = true; }
    void local_window_dropped() { have_lwin = false; }
    void global_window_held() { glob_valid = true; }
    void global_window_dropped() { glob_valid = false; }
};

}  // namespace bf_state
