"""The coarse-to-fine and seeded per-cell search (bf_global_search_cells_pyramid) next to the exhaustive per-cell sweep
(bf_global_search_cells), on the inputs of scripts/global_cells_bench.py:

  * config 4's input (1M events, 346 x 260, scale 3, window 15, 33 x 32 cells of 8 x 11 pixels) over the 90 x 100 lattice
    that holds the injected flow: the exhaustive sweep, the pyramid, and the seeded search on a second slice of the same
    motion from the pyramid's answers on the first; per leg the candidates evaluated (per level and in total), ms (best
    of --reps), ms per evaluated candidate, and the accuracy columns of DESIGN.md's config-4 table;
  * the same three on the 52 000-event 240 x 180 slice, default lattice (180 x 80), scale 5, window 21, 32 x 32-pixel
    cells (timing only: the default range does not reach that slice's motion);
  * the pyramid alone over a wide lattice that needs no knowledge of the truth (+-500 px/s around zero, step 0.001) on
    config 4's input; the exhaustive sweep is not run there: its cost is quoted as candidates x the measured time per
    candidate of the 90 x 100 sweep, marked extrapolated.

Writes profiles/global_pyramid_bench.json (--out to change) and prints the same JSON line.  --quick: config 4's pyramid
leg only, once (for a profiler run)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

NZ = 127.0
STEP_PX_S = 0.001 / NZ * 1e5   # one lattice step in px/s (Event::compute_uv)


def timed(acc, scale, mw, cells, reps, run):
    """best-of-reps seconds of run() from a fresh window and grid (the sort is part of a slice's cost); a warm-up run first"""
    times = []
    for rep in range(reps + 1):
        acc.global_set_window(scale, mw)
        t0 = time.perf_counter()
        acc.global_set_cells(*cells)
        out = run()
        if rep:
            times.append(time.perf_counter() - t0)
    return min(times), times, out


def accuracy(cells, truth, scale, dur):
    has = cells["events"] > 0
    u, v = cells["best_u"][has], cells["best_v"][has]
    tu, tv = truth
    tol, px = 2 * STEP_PX_S, 1.0 / (scale * dur)
    return {"non_empty": int(has.sum()), "median_uv_px_s": [float(np.median(u)), float(np.median(v))],
            "within_2_steps": float(np.mean((np.abs(u - tu) <= tol) & (np.abs(v - tv) <= tol))),
            "within_1_image_pixel": float(np.mean((np.abs(u - tu) <= px) & (np.abs(v - tv) <= px))),
            "cells_lost_vs_2_steps": int(np.sum(~((np.abs(u - tu) <= tol) & (np.abs(v - tv) <= tol))))}


def leg(name, best, all_, n_eval, info=None, acc_cols=None, **kw):
    out = {"call": name, "ms": round(best * 1e3, 2), "ms_all": [round(t * 1e3, 2) for t in all_], "evaluated": int(n_eval),
           "us_per_candidate": round(best * 1e6 / max(n_eval, 1), 2)}
    if info is not None:
        out["level_count"] = [int(v) for v in list(info.level_count)[:info.levels_run]]
        out["lattice"] = [int(info.n_x), int(info.n_y)]
    if acc_cols:
        out.update(acc_cols)
    out.update(kw)
    return out


def three_searches(sl_a, sl_b, sensor, scale, mw, cell, opts, pyr, seeded_pyr, reps, truth=None, dur=0.03, quick=False):
    """exhaustive, pyramid and seeded (slice b from slice a's pyramid answers) over one lattice"""
    H, W = sensor
    grid = (H, W) + cell
    acc = accel.Accel(device=0, max_events=max(len(sl_a["t"]), len(sl_b["t"])))
    acc.upload_events(sl_a["fr_x"], sl_a["fr_y"], sl_a["t"])
    legs = []
    if not quick:
        best, all_, (r, cells, _) = timed(acc, scale, mw, grid, reps, lambda: acc.global_search_cells(opts))
        legs.append(leg("bf_global_search_cells", best, all_, r.n_x * r.n_y,
                        acc_cols=accuracy(cells, truth, scale, dur) if truth else None, lattice=[int(r.n_x), int(r.n_y)]))
    best, all_, (r, cells, ev, _, info) = timed(acc, scale, mw, grid, 1 if quick else reps,
                                                lambda: acc.global_search_cells_pyramid(opts, **pyr))
    legs.append(leg("bf_global_search_cells_pyramid", best, all_, info.evaluated, info,
                    accuracy(cells, truth, scale, dur) if truth else None, setting=pyr))
    if not quick:
        seeds = np.where(cells["events"] > 0, cells["best_index"], -1)
        acc.upload_events(sl_b["fr_x"], sl_b["fr_y"], sl_b["t"])
        best, all_, (r, cells, ev, _, info) = timed(acc, scale, mw, grid, reps,
                                                    lambda: acc.global_search_cells_pyramid(opts, seeds=seeds, **seeded_pyr))
        legs.append(leg("bf_global_search_cells_pyramid seeded", best, all_, info.evaluated, info,
                        accuracy(cells, truth, scale, dur) if truth else None, setting=seeded_pyr))
        ex = legs[0]   # (the seeded leg runs on slice b, of the same size and motion: its ratio is against slice a's sweep)
        for l in legs[1:]:
            l["ratio_to_exhaustive"] = round(l["ms"] / ex["ms"], 4)
            l["share_of_lattice"] = round(l["evaluated"] / ex["evaluated"], 4)
        legs[2]["ratio_note"] = "against the exhaustive sweep of the first slice (the second has the same size and motion)"
    acc.close()
    return legs


def config4(reps, quick, pyr, seeded_pyr, wide_pyr):
    N, H, W, scale, mw, G, dur = 1000000, 260, 346, 3, 15, 32, 0.030
    sl_a = synth.make_slice(N, H, W, dur, seed=1)
    sl_b = synth.make_slice(N, H, W, dur, seed=2)               # the next slice: the same motion, other events
    tu, tv = sl_a["velocity"]
    cx, cy = round(tu * NZ * 1e-5, 3), round(tv * NZ * 1e-5, 3)
    opts = accel.Accel.global_search_opts(x_low=cx - 0.045, x_hi=cx + 0.045, y_low=cy - 0.05, y_hi=cy + 0.05)
    cell = (H // G, -(-W // G))                                 # 8 x 11 pixels: 33 x 32 cells
    res = {"events": [int(len(sl_a["t"])), int(len(sl_b["t"]))], "sensor": [H, W], "scale": scale, "metric_wsize": mw,
           "cell": list(cell), "injected_px_s": [tu, tv], "two_steps_px_s": 2 * STEP_PX_S,
           "one_image_pixel_px_s": 1.0 / (scale * dur),
           "legs": three_searches(sl_a, sl_b, (H, W), scale, mw, cell, opts, pyr, seeded_pyr, reps, (tu, tv), dur, quick)}
    if quick:
        return res
    lim = round(500.0 * NZ * 1e-5, 3)                           # +-500 px/s
    wide = accel.Accel.global_search_opts(x_low=-lim, x_hi=lim, y_low=-lim, y_hi=lim)
    acc = accel.Accel(device=0, max_events=len(sl_a["t"]))
    acc.upload_events(sl_a["fr_x"], sl_a["fr_y"], sl_a["t"])
    best, all_, (r, cells, ev, _, info) = timed(acc, scale, mw, (H, W) + cell, reps,
                                                lambda: acc.global_search_cells_pyramid(wide, **wide_pyr))
    acc.close()
    w = leg("bf_global_search_cells_pyramid", best, all_, info.evaluated, info, accuracy(cells, (tu, tv), scale, dur),
            setting=wide_pyr, range_px_s=[-500.0, 500.0])
    per = res["legs"][0]["us_per_candidate"]
    w["exhaustive_extrapolated_s"] = round(info.n_x * info.n_y * per * 1e-6, 1)
    w["exhaustive_extrapolated_from"] = "%d x %d candidates x %.2f us (the 90 x 100 sweep's measured time per candidate)" % (
        info.n_x, info.n_y, per)
    res["wide_lattice"] = w
    return res


def default_50k(reps, pyr, seeded_pyr):
    H, W, scale, mw = 180, 240, 5, 21
    sl_a = synth.make_slice(52000, H, W, 0.03, seed=1)
    sl_b = synth.make_slice(52000, H, W, 0.03, seed=2)
    return {"events": [int(len(sl_a["t"])), int(len(sl_b["t"]))], "sensor": [H, W], "scale": scale, "metric_wsize": mw,
            "cell": [32, 32],
            "legs": three_searches(sl_a, sl_b, (H, W), scale, mw, (32, 32), accel.Accel.global_search_opts(), pyr, seeded_pyr, reps)}


def main():
    quick = "--quick" in sys.argv
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "global_pyramid_bench.json")
    pyr = dict(levels=3, factor=4, radius=2)
    seeded = dict(levels=1, factor=2, radius=2)
    wide = dict(levels=3, factor=4, radius=2)                   # stride 16: inside the +-14 steps over which a cell's peak is flat
    out = {"config4": config4(reps, quick, pyr, seeded, wide)}
    if not quick:
        out["default_sweep_50k"] = default_50k(reps, pyr, seeded)
    line = json.dumps({"global_search_cells_pyramid": out})
    if not quick:
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
