"""bf_run_groups with "groups_wide" = 1 against the helper sequence it replaces: the refit step of one
alternation, warm, on a slice split into a small patch and the background.

  scene     tests/segment_scene.py's two-motion scene (90 x 120, ~15.6k events, scale 3): patch = group 0, background = group 1,
            both warm from their true models;
  large     a synthetic slice of --large-events events (default 1M) on 346 x 260: the events of a 30 x 30 sensor block are the
            patch, everything else the background, both warm from the slice's own velocity.

Timed per workload, host wall clock around synchronised calls, median of --reps after a warm-up:
  wide_ms     bf_run_groups with the option on (the slice uploaded and grouped before the clock starts);
  groups_ms   bf_run_groups with the option off (the background comes back BF_ERR_CAPACITY) ...
  helper_ms   ... and then what bf::MotionAssigner does with it: the background's events gathered on the host,
              bf_upload_events, bf_set_cloud, bf_set_model, bf_run and bf_writeout_events of (nx, ny) on a second context;
  today_ms    groups_ms + helper_ms, measured as one sequence.
  --quick   every device workload --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/groups_wide_bench.py --quick).
  --kernel-trace FILE  the kernel trace CSV of such a run: the median time per kernel name is merged into --out.

Prints one JSON line and writes it to profiles/groups_wide_bench.json."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

KERNELS = ("k_group_gather", "k_group_scatter_back", "k_group_optimizer", "k_prepare", "k_tile_scatter", "k_group_boxes")
HARD_CAP = 20000


def model_for(velocity):
    m = accel.Model()
    m.total_dx, m.total_dy = -velocity[0] * 1.27e-3, -velocity[1] * 1.27e-3
    return m


def scene_workload():
    import segment_scene as scene
    sc = scene.make()
    gid = np.where(sc["is_patch"], 0, 1).astype(np.int32)
    return dict(name="scene", sl=sc, gid=gid, res=(scene.H, scene.W), warm=[model_for(scene.V_PATCH), model_for(scene.V_BACKGROUND)])


def large_workload(n_events):
    H, W = 260, 346
    sl = synth.make_slice(n_events, H, W, 0.030, seed=1)
    x, y = sl["fr_x"], sl["fr_y"]
    gid = np.where((x >= 100) & (x < 130) & (y >= 150) & (y < 180), 0, 1).astype(np.int32)
    v = synth.default_velocity(H, W)
    return dict(name="large", sl=sl, gid=gid, res=(H, W), warm=[model_for(v), model_for(v)])


def median_ms(reps, fn, sync, prepare=None):
    times = []
    for rep in range(reps + 1):   # the first run warms up (buffers grown on first use, the inner context created)
        if prepare:
            prepare()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def run_workload(w, reps, quick):
    sl, gid, res, warm = w["sl"], w["gid"], w["res"], w["warm"]
    n = len(gid)
    S = 3
    cap = dict(device=0, max_events=n, max_rows=S * res[0] + S, max_cols=S * res[1] + S)
    a, helper = accel.Accel(**cap), accel.Accel(**cap)
    bg = np.flatnonzero(gid == 1)
    out = dict(events=n, background=int(len(bg)), patch=int((gid == 0).sum()))
    results = {}

    def stage():
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_groups(gid, 2)

    def groups(wide):
        a.set_option("groups_wide", wide)
        results["g%d" % wide] = a.run_groups(2, S, res, res, 100, warm=warm, hard_iter_cap=HARD_CAP)

    def helper_refit():   # bf::ObjectTasks' one-after-the-other path for the one large group (object_tasks.h)
        fx, fy, ft = sl["fr_x"][bg], sl["fr_y"][bg], sl["t"][bg]
        helper.upload_events(fx, fy, ft)
        helper.set_cloud(S, res[0], res[1])
        helper.set_model(warm[1])
        o = helper.default_opts()
        o.max_iter, o.min_events, o.res_x, o.res_y, o.hard_iter_cap = -1, 100, res[0], res[1], HARD_CAP
        m, info = accel.Model(), accel.RunInfo()
        helper.L.bf_run(helper.h, C.byref(o), C.byref(m), C.byref(info))
        nx, ny = np.empty(len(bg)), np.empty(len(bg))
        helper.L.bf_writeout_events(helper.h, None, None, nx.ctypes.data_as(C.c_void_p), ny.ctypes.data_as(C.c_void_p))
        full = np.zeros((2, n))
        full[0, bg], full[1, bg] = nx, ny   # (copied back event by event on the host, as the class does)
        results["helper"] = info

    def today():
        groups(0)
        helper_refit()

    sync = lambda: (a.synchronize(), helper.synchronize())
    if quick:
        for _ in range(quick):
            stage(); groups(1); stage(); today()
        sync()
    else:
        out["wide_ms"] = median_ms(reps, lambda: groups(1), sync, stage)
        out["groups_ms"] = median_ms(reps, lambda: groups(0), sync, stage)
        out["helper_ms"] = median_ms(reps, helper_refit, sync)
        out["today_ms"] = median_ms(reps, today, sync, stage)
    stage(); groups(1)
    out["wide_groups"] = a.get_stat("groups_wide")
    i1 = results["g1"][1]
    out["wide_rc"] = [int(x.rc) for x in i1]
    out["wide_iterations"] = [int(x.iterations) for x in i1]
    q = results["g1"][2][1]
    out["background_window"] = [int(q.rows), int(q.cols)]
    if "helper" in results:
        out["helper_iterations"] = int(results["helper"].iterations)
    # would the main context's own warm runs take the persistent form -- alone, and with the helper alive?
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    a.set_cloud(S, res[0], res[1])
    a.set_model(warm[1])
    out["persistent_with_helper_alive"] = int(a.get_stat("persistent"))
    helper.close()
    out["persistent_alone"] = int(a.get_stat("persistent"))
    a.close()
    return out


def kernel_medians(path):
    by = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    by.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(launches=len(v), median_us=float(np.median(v)), max_us=float(np.max(v))) for k, v in by.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large-events", type=int, default=1000000)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=3)
    ap.add_argument("--kernel-trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_wide_bench.json"))
    args = ap.parse_args()
    if args.kernel_trace:
        rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
        rec["kernel_trace_us"] = kernel_medians(args.kernel_trace)
        json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(rec, sort_keys=True))
        return
    rec = dict(reps=args.reps, timing="host wall clock around synchronised calls, median of reps after a warm-up")
    for w in (scene_workload(), large_workload(args.large_events)):
        rec[w["name"]] = run_workload(w, args.reps, args.quick_reps if args.quick else 0)
    if not args.quick:
        json.dump(rec, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
