"""The per-cell form of OptimizerGlobal's sweep (bf_global_search_cells) on the device, next to bf_global_search:

  * the default sweep (180 x 80 candidates) on the 52 000-event 240 x 180 slice of scripts/global_search_bench.py, scale 5,
    window 21: bf_global_search, and bf_global_search_cells with 8 x 8- and 32 x 32-pixel cells, with and without a surface
    buffer; ms per sweep (best of --reps) and the ratio to bf_global_search;
  * config 4's input (1M events, 346 x 260, the injected flow of scripts/config4_tiles.py, scale 3, window 15) on 32 x 32
    cells of 11 x 8 pixels and on coarser grids, over a range that holds the injected flow: ms per slice, the median per-cell
    (u, v), the share of non-empty cells within 2 grid steps of the truth in both components, and within the flow that moves
    an event by one pixel of the scaled image over the slice (1 / (scale * duration) px/s: what one slice can resolve).

Prints one JSON line.  --quick: the 32 x 32-pixel-cell sweep of the first part only, once (for a profiler run)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

NZ = 127.0
STEP_PX_S = 0.001 / NZ * 1e5   # one candidate step in px/s (Event::compute_uv)


def timed(acc, scale, mw, cells, reps, run):
    """best-of-reps seconds of run() from a fresh window (and grid); the warm-up run first"""
    times = []
    for rep in range(reps + 1):
        acc.global_set_window(scale, mw)
        t0 = time.perf_counter()
        if cells:
            acc.global_set_cells(*cells)      # the sort is part of a slice's cost
        out = run()
        if rep:
            times.append(time.perf_counter() - t0)
    return min(times), times, out


def default_sweep(reps, quick):
    H, W, scale, mw = 180, 240, 5, 21
    sl = synth.make_slice(52000, H, W, 0.03, seed=1)
    acc = accel.Accel(device=0, max_events=len(sl["t"]))
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    res = {"events": int(len(sl["t"])), "sensor": [H, W], "scale": scale, "metric_wsize": mw, "legs": []}
    base = None
    if not quick:
        base, all_, (r, _) = timed(acc, scale, mw, None, reps, lambda: acc.global_search(want_surface=False))
        res["candidates"] = int(r.n_x * r.n_y)
        res["legs"].append({"call": "bf_global_search", "ms": round(base * 1e3, 2), "ms_all": [round(t * 1e3, 2) for t in all_]})
    for rows, cols in ((32, 32),) if quick else ((8, 8), (32, 32)):
        for surface in (False,) if quick else (False, True):
            best, all_, (r, cells, _) = timed(acc, scale, mw, (H, W, rows, cols), 1 if quick else reps,
                                              lambda: acc.global_search_cells(want_surface=surface))
            leg = {"call": "bf_global_search_cells", "cell": [rows, cols], "cells": int(cells.size), "surface": surface,
                   "ms": round(best * 1e3, 2), "ms_all": [round(t * 1e3, 2) for t in all_]}
            if base:
                leg["ratio_to_global_search"] = round(best / base, 3)
            res["legs"].append(leg)
    acc.close()
    return res


def config4(reps):
    N, H, W, scale, mw, G, dur = 1000000, 260, 346, 3, 15, 32, 0.030
    sl = synth.make_slice(N, H, W, dur, seed=1)
    tu, tv = sl["velocity"]                                   # px/s, (rows, columns)
    cx, cy = round(tu * NZ * 1e-5, 3), round(tv * NZ * 1e-5, 3)   # the candidate next to it
    opts = accel.Accel.global_search_opts(x_low=cx - 0.045, x_hi=cx + 0.045, y_low=cy - 0.05, y_hi=cy + 0.05)
    acc = accel.Accel(device=0, max_events=len(sl["t"]))
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    res = {"events": int(len(sl["t"])), "sensor": [H, W], "scale": scale, "metric_wsize": mw, "injected_px_s": [tu, tv],
           "range_nx": [opts.x_low, opts.x_hi], "range_ny": [opts.y_low, opts.y_hi],
           "range_px_s": [[opts.x_low / NZ * 1e5, opts.x_hi / NZ * 1e5], [opts.y_low / NZ * 1e5, opts.y_hi / NZ * 1e5]], "grids": []}
    tol, px = 2 * STEP_PX_S, 1.0 / (scale * dur)
    res["two_steps_px_s"], res["one_image_pixel_px_s"] = tol, px
    for k in (1, 2, 4, 8):                                     # 32 x 32 cells of 11 x 8 pixels, then coarser
        rows, cols = (H // G) * k, -(-W // G) * k          # 8 x 11 pixels: 33 x 32 cells, the last row ragged
        best, all_, (r, cells, _) = timed(acc, scale, mw, (H, W, rows, cols), reps, lambda: acc.global_search_cells(opts))
        has = cells["events"] > 0
        u, v = cells["best_u"][has], cells["best_v"][has]
        res["candidates"] = int(r.n_x * r.n_y)
        res["grids"].append({"cell": [rows, cols], "grid": list(cells.shape), "non_empty": int(has.sum()),
                             "events_per_cell_median": float(np.median(cells["events"][has])),
                             "ms_per_slice": round(best * 1e3, 1), "ms_all": [round(t * 1e3, 1) for t in all_],
                             "median_uv_px_s": [float(np.median(u)), float(np.median(v))],
                             "within_2_steps": float(np.mean((np.abs(u - tu) <= tol) & (np.abs(v - tv) <= tol))),
                             "within_1_image_pixel": float(np.mean((np.abs(u - tu) <= px) & (np.abs(v - tv) <= px))),
                             "worst_abs_error_px_s": [float(np.abs(u - tu).max()), float(np.abs(v - tv).max())],
                             "slice_best_nx_ny": [r.best_nx, r.best_ny]})
    acc.close()
    return res


def main():
    quick = "--quick" in sys.argv
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    out = {"default_sweep_50k": default_sweep(reps, quick)}
    if not quick:
        out["config4"] = config4(max(1, reps - 1))
    print(json.dumps({"global_search_cells": out}))


if __name__ == "__main__":
    main()
