"""One piecewise projection (bf_global_project_cells) next to one bf_global_project_all on the same slice and window:

  * the 52 000-event 240 x 180 slice, scale 5, window 21, with 8 x 8- and 32 x 32-pixel cells;
  * config 4's input (1M events, 346 x 260, scale 3, window 15) with 8 x 11-pixel cells (33 x 32 of them).

Every cell gets the injected flow's lattice point, so both calls render the same image and return the same sum (checked:
the identity of include/bf_accel.h).  A repeat is --inner calls of each, alternating, every call ending in its own stream
synchronise; ms per call, best of --reps (3) after one warm-up repeat, once for the sum alone and once with the image and
current_scores copied back.  Writes profiles/global_piecewise_bench.json (--out to change) and prints the same JSON line."""
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
        nc = g.n_cell_x * g.n_cell_y
        cx, cy = np.full(nc, nx), np.full(nc, ny)
        S, img, sc = acc.global_project_all(nx, ny)
        pimg, psc, S_pw, sums = acc.global_project_cells(cx, cy)
        if not (S == S_pw == int(sums.sum()) and np.array_equal(img, pimg) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32))):
            raise RuntimeError("bf_global_project_cells with one candidate differs from bf_global_project_all")
        entry = {"cell": list(cell), "cells": [int(g.n_cell_x), int(g.n_cell_y)], "S": int(S)}
        for name, want in (("sum_only", False), ("with_image_and_scores", True)):
            t_all, t_pw = [], []
            for rep in range(reps + 1):                               # (repeat 0 warms up)
                a = b = 0.0
                for _ in range(inner):
                    t0 = time.perf_counter()
                    acc.global_project_all(nx, ny, want_img=want, want_scores=want)
                    t1 = time.perf_counter()
                    acc.global_project_cells(cx, cy, want_img=want, want_scores=want, want_cell_sums=want)
                    t2 = time.perf_counter()
                    a += t1 - t0
                    b += t2 - t1
                if rep:
                    t_all.append(a / inner)
                    t_pw.append(b / inner)
            entry[name] = {"project_all_ms": round(min(t_all) * 1e3, 4), "project_cells_ms": round(min(t_pw) * 1e3, 4),
                           "project_all_ms_all": [round(t * 1e3, 4) for t in t_all],
                           "project_cells_ms_all": [round(t * 1e3, 4) for t in t_pw],
                           "ratio": round(min(t_pw) / min(t_all), 4)}
        out["grids"].append(entry)
    acc.close()
    return out


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    inner = int(sys.argv[sys.argv.index("--inner") + 1]) if "--inner" in sys.argv else 100
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "global_piecewise_bench.json")
    out = {"slice_52k": one_input(synth.make_slice(52000, 180, 240, 0.03, seed=1), (180, 240), 5, 21, [(8, 8), (32, 32)], reps, inner),
           "config4": one_input(synth.make_slice(1000000, 260, 346, 0.03, seed=1), (260, 346), 3, 15, [(8, 11)], reps, inner)}
    line = json.dumps({"global_project_cells": out})
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
