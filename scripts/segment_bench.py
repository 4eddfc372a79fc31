"""The moving-object segmentation (bf_segment) on the device, next to the pass it extends:

  * a 1M-event 346 x 260 slice at scale 3 (image 783 x 1041) and a 1M-event 1280 x 720 slice at scale 1, events resident,
    compensated with 0.8 of the true flow (so that the time image has structure): bf_get_time_img without read-back, and
    bf_segment -- the same pass plus the segmentation -- with both thresholds at 4 ms (min_count 2, min_pixels 4, 8-connected)
    and with no threshold (regions of activity); ms per call, best of --reps after a warm-up, and the ratio to the pass;
  * bf::Segmenter's host path on the same machine and context (tests/cpp/test_segment.cpp built against the library: the
    read-backs of bf_get_time_img / bf_writeout_events and the union-find on the host), on the 346 x 260 slice.

Prints one JSON line and writes it to profiles/segment_bench.json.  --quick: one bf_segment per shape (for a profiler run)."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

DUR = 0.030
LEGS = {"thresholds_4ms": dict(above_s=0.004, below_s=0.004, min_count=2, connectivity=8, min_pixels=4),
        "activity": dict(above_s=-1.0, below_s=-1.0, min_count=1, connectivity=8, min_pixels=1)}


def best_of(reps, fn, sync):
    times = []
    for rep in range(reps + 1):                      # the first run warms up (buffers grown on first use)
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if rep:
            times.append(time.perf_counter() - t0)
    return min(times), times, out


def shape(H, W, scale, reps, quick):
    sl = synth.make_slice(1000000, H, W, DUR, seed=1)
    acc = accel.Accel(device=0, max_events=len(sl["t"]), max_rows=scale * H + scale, max_cols=scale * W + scale)
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    w = acc.set_cloud(scale, H, W)
    nx, ny = 0.8 * sl["velocity"][0] * 1.27e-3, 0.8 * sl["velocity"][1] * 1.27e-3
    acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    sync = lambda: acc._chk(acc.L.bf_synchronize(acc.h))
    res = {"events": int(len(sl["t"])), "sensor": [H, W], "scale": scale, "image": [int(w.scale_img_x), int(w.scale_img_y)], "legs": {}}
    if quick:
        for name, o in LEGS.items():
            acc.segment(**o)
        acc.close()
        return res, sl, (nx, ny)
    base, all_, _ = best_of(reps, lambda: acc.get_time_img(want_time=False, want_count=False), sync)
    res["time_img_pass_ms"] = round(base * 1e3, 4)
    res["time_img_pass_ms_all"] = [round(t * 1e3, 4) for t in all_]
    for name, o in LEGS.items():
        best, all_, info = best_of(reps, lambda: acc.segment(**o), sync)
        res["legs"][name] = {"opts": o, "ms": round(best * 1e3, 4), "ms_all": [round(t * 1e3, 4) for t in all_],
                             "segmentation_alone_ms": round((best - base) * 1e3, 4), "ratio_to_time_img_pass": round(best / base, 3),
                             "foreground_pixels": int(info.foreground_pixels), "components_found": int(info.components_found),
                             "components": int(info.components)}
    acc.close()
    return res, sl, (nx, ny)


def host_path(sl, H, W, scale, flow):
    """bf::Segmenter's two paths, timed by tests/cpp/test_segment.cpp on one context"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_segment")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "better_flow_amd", "host"),
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_segment.cpp"),
                               "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"),
                               "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        ev = os.path.join(d, "events.txt")
        np.savetxt(ev, np.stack([sl["fr_x"], sl["fr_y"], sl["t"]], axis=1), fmt="%d")
        o = LEGS["thresholds_4ms"]
        out = subprocess.check_output([exe, ev, str(scale), str(H), str(W), repr(flow[0]), repr(flow[1]), repr(o["above_s"]), repr(o["below_s"]),
                                       str(o["min_count"]), str(o["connectivity"]), str(o["min_pixels"]), os.path.join(d, "out_")],
                                      timeout=600).decode().splitlines()
    assert "paths agree" in out, out
    t = [ln.split() for ln in out if ln.startswith("time_ms")][0]
    return {"opts": o, "device_path_ms": float(t[2]), "host_path_ms": float(t[4]),
            "note": "wall time of bf::Segmenter::run including its read-backs to host vectors; identical bytes (checked by the program)"}


def main():
    quick = "--quick" in sys.argv
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "segment_bench.json")
    out = {}
    a, sl, flow = shape(260, 346, 3, reps, quick)
    out["346x260_scale3"] = a
    out["1280x720_scale1"] = shape(720, 1280, 1, reps, quick)[0]
    if not quick:
        out["346x260_scale3"]["segmenter"] = host_path(sl, 260, 346, 3, flow)
    line = json.dumps({"segment": out})
    if not quick:
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
