"""OptimizerGlobal's default sweep (180 x 80 candidates, optimizer_global.cpp:104-150) on the device: ms per sweep and
us per candidate on two slices, the numpy restatement's per-candidate time on the CPU for the ratio, and a byte model
of one candidate.  Prints one JSON line.  --quick: the 50k slice only, one timed sweep (for a profiler run)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import global_ref as G  # noqa: E402
from better_flow_amd import accel, synth  # noqa: E402


def model(w, n_acc, n):
    """Bytes of one candidate through G1 / G2 / G3 (two 32-bit planes of the bordered image, the events twice)."""
    P = w.scale_bordered_img_x * w.scale_bordered_img_y
    halo = ((32 + w.metric_wsize - 1 + 4 * (w.scale // 2)) * (64 + w.metric_wsize - 1 + 4 * (w.scale // 2))) / (32 * 64)
    b = {
        "memset_points": 4 * P,
        "g1_events_read": 8 * n, "g1_point_atomics": 4 * n_acc,
        "g2_points_read": int(4 * P * halo), "g2_window_write": 4 * P,
        "g3_events_read": 8 * n, "g3_window_gather": 4 * n_acc,
    }
    b["total"] = sum(b.values())
    return b


def sweep(label, n, h, wd, scale, mw, reps, cpu_cands):
    sl = synth.make_slice(n, h, wd, 0.03, seed=1)
    ev = (sl["fr_x"], sl["fr_y"], sl["t"])
    acc = accel.Accel(device=0, max_events=len(sl["t"]))
    acc.upload_events(*ev)
    w = acc.global_set_window(scale, mw)
    acc.global_search(want_surface=False)                  # warm-up: buffers, code objects
    times = []
    for _ in range(reps):
        acc.global_set_window(scale, mw)
        t0 = time.perf_counter()
        r, _ = acc.global_search(want_surface=False)
        times.append(time.perf_counter() - t0)
    acc.close()
    k = r.n_x * r.n_y
    best = min(times)
    out = {"slice": label, "events": int(len(sl["t"])), "scale": scale, "metric_wsize": mw, "candidates": int(k),
           "bordered_img": [w.scale_bordered_img_x, w.scale_bordered_img_y],
           "ms_per_sweep": round(best * 1e3, 2), "ms_per_sweep_all": [round(t * 1e3, 2) for t in times],
           "us_per_candidate": round(best / k * 1e6, 2), "best": [r.best_nx, r.best_ny, int(r.best_sum)]}
    if cpu_cands:
        ref = G.Global(*ev, scale=scale, metric_wsize=mw)
        ref.project_all(0.0, 0.0)
        t0 = time.perf_counter()
        for i in range(cpu_cands):
            ref.project_all(0.001 * i, -0.0005 * i)
        cpu = (time.perf_counter() - t0) / cpu_cands
        out["cpu_restatement_ms_per_candidate"] = round(cpu * 1e3, 1)
        out["cpu_over_gpu"] = round(cpu / (best / k), 0)
    _, _, ok = G.pixels(*G.project(*ev, 0.0, 0.0), G.window(ev[0], ev[1], scale, mw))
    m = model(w, int(ok.sum()), len(sl["t"]))
    out["model_bytes_per_candidate"] = m
    out["model_GBps_at_measured"] = round(m["total"] * k / best / 1e9, 1)
    return out


def main():
    quick = "--quick" in sys.argv
    res = [sweep("50k_240x180", 52000, 180, 240, 5, 21, 1 if quick else 3, 0 if quick else 5)]
    if not quick:
        res.append(sweep("1M_346x260", 1040000, 260, 346, 5, 21, 2, 2))
    print(json.dumps({"global_search": res}))


if __name__ == "__main__":
    main()
