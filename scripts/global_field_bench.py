"""One interpolated-field projection (bf_global_project_field) next to one piecewise projection (bf_global_project_cells)
with the same grid, on the inputs of scripts/global_piecewise_bench.py:

  * the 52 000-event 240 x 180 slice, scale 5, window 21, with 8 x 8- and 32 x 32-pixel cells;
  * config 4's input (1M events, 346 x 260, scale 3, window 15) with 8 x 11-pixel cells (33 x 32 of them).

The grid is the injected flow's lattice point plus a ramp of a few lattice steps over the cells, so that the field call
really interpolates; the two calls render different images (a uniform grid, with which they must agree bit for bit, is
checked first).  A repeat is --inner calls of each, alternating, every call ending in its own stream synchronise; ms per
call, best of --reps (3) after one warm-up repeat, for the sum alone, with the image, current_scores and cell sums copied
back, and with the per-event outputs (nx, ny, u, v) on top of those.  Writes profiles/global_field_bench.json (--out to change)
and prints the same JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

NZ = 127.0


def one_input(sl, sensor, scale, mw, cell_shapes, reps, inner):
    H, W = sensor
    tu, tv = sl["velocity"]
    nx, ny = round(tu * NZ * 1e-5, 3), round(tv * NZ * 1e-5, 3)        # the lattice point nearest the injected flow
    acc = accel.Accel(device=0, max_events=len(sl["t"]))
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    acc.global_set_window(scale, mw)
    out = {"events": int(len(sl["t"])), "sensor": [H, W], "scale": scale, "metric_wsize": mw, "candidate": [nx, ny],
           "calls_per_repeat": inner, "grids": []}
    for cell in cell_shapes:
        g = acc.global_set_cells(H, W, *cell)
        shape = (g.n_cell_x, g.n_cell_y)
        ux, uy = np.full(shape, nx), np.full(shape, ny)
        a, b = acc.global_project_cells(ux, uy), acc.global_project_field(ux, uy)
        if not (a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
                and np.array_equal(a[3], b[3])):
            raise RuntimeError("bf_global_project_field with a uniform grid differs from bf_global_project_cells")
        ramp_x = np.linspace(-0.002, 0.002, shape[1])[None, :] * np.ones(shape)      # +-2 lattice steps across the columns
        ramp_y = np.linspace(-0.001, 0.001, shape[0])[:, None] * np.ones(shape)
        cx, cy = ux + ramp_x, uy + ramp_y
        entry = {"cell": list(cell), "cells": [int(g.n_cell_x), int(g.n_cell_y)],
                 "S_pw": int(acc.global_project_cells(cx, cy, want_img=False, want_scores=False)[2]),
                 "S_f": int(acc.global_project_field(cx, cy, want_img=False, want_scores=False)[2])}
        for name, want, events in (("sum_only", False, False), ("with_image_and_scores", True, False),
                                   ("with_image_scores_and_events", True, True)):
            t_pw, t_f = [], []
            for rep in range(reps + 1):                               # (repeat 0 warms up)
                a = b = 0.0
                for _ in range(inner):
                    t0 = time.perf_counter()
                    acc.global_project_cells(cx, cy, want_img=want, want_scores=want, want_cell_sums=want)
                    t1 = time.perf_counter()
                    acc.global_project_field(cx, cy, want_img=want, want_scores=want, want_cell_sums=want, want_events=events)
                    t2 = time.perf_counter()
                    a += t1 - t0
                    b += t2 - t1
                if rep:
                    t_pw.append(a / inner)
                    t_f.append(b / inner)
            entry[name] = {"project_cells_ms": round(min(t_pw) * 1e3, 4), "project_field_ms": round(min(t_f) * 1e3, 4),
                           "project_cells_ms_all": [round(t * 1e3, 4) for t in t_pw],
                           "project_field_ms_all": [round(t * 1e3, 4) for t in t_f],
                           "ratio": round(min(t_f) / min(t_pw), 4)}
        out["grids"].append(entry)
    acc.close()
    return out


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    inner = int(sys.argv[sys.argv.index("--inner") + 1]) if "--inner" in sys.argv else 100
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "global_field_bench.json")
    out = {"slice_52k": one_input(synth.make_slice(52000, 180, 240, 0.03, seed=1), (180, 240), 5, 21, [(8, 8), (32, 32)], reps, inner),
           "config4": one_input(synth.make_slice(1000000, 260, 346, 0.03, seed=1), (260, 346), 3, 15, [(8, 11)], reps, inner)}
    line = json.dumps({"global_project_field": out})
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
