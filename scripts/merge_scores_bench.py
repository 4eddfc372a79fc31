"""bf_merge_scores on the device: the config-4 slice (1M events, 346 x 260, scale 3), K = 2, 4 and 8 groups
under K translations, the ids a seeded uniform draw as in scripts/project_groups_bench.py, the events in upload order.

  timing    host wall clock around a synchronised call, median of --reps after a warm-up (`call_ms`).  Two yardsticks from the
            same run: bf_project_groups on the same grouping with its images left on the device (`project_call_ms`), and the
            bf_get_time_img pass without read-back (`time_img_pass_ms`).  The call does the work of K + 1 projections without
            label or colour: `over_k_plus_1_projections` = call_ms / ((K + 1) project_call_ms) is expected below 1.
  --quick   every K --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/merge_scores_bench.py --quick); the order of the calls is
            written to --labels.
  --kernel-trace FILE  a kernel trace CSV of such a run: a call begins at its k_project_vote; the times of its kernels, summed
            per kernel name, are matched to the labels and their medians per K are merged into --out.

Prints one JSON line and writes it to profiles/merge_scores_bench.json."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402
from project_groups_bench import models_for, median_ms  # noqa: E402

H, W, S = 260, 346, 3
KS = (2, 4, 8)
KERNELS = ("k_project_vote", "k_assign_box", "k_merge_total", "k_merge_vote", "k_merge_gain")


def merge(a, models, targets_per_pass=0):
    K = len(models)
    o = accel.MergeOpts(S, H, W, 0, targets_per_pass)
    ms = (accel.Model * K)(*models)
    gain = np.zeros((K, K), dtype=np.uint64)
    info = accel.MergeInfo()
    a._chk(a.L.bf_merge_scores(a.h, C.byref(o), ms, K, gain.ctypes.data_as(C.c_void_p), None, None, C.byref(info)))
    return gain, info


def project(a, models):
    K = len(models)
    o = accel.ProjectOpts(S, H, W, 0, 8)
    ms = (accel.Model * K)(*models)
    info = accel.ProjectInfo()
    a._chk(a.L.bf_project_groups(a.h, C.byref(o), ms, K, None, None, None, None, C.byref(info)))
    return info


def run(args):
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    n = len(sl["t"])
    a = accel.Accel(device=0, max_events=n, max_rows=S * H + S, max_cols=S * W + S)
    sync = lambda: a._chk(a.L.bf_synchronize(a.h))
    res = {"events": int(n), "sensor": [H, W], "scale": S, "window": [S * H, S * W], "workloads": []}
    labels = []
    if not args.quick:
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_cloud(S, H, W)
        res["time_img_pass_ms"], res["time_img_pass_ms_all"] = median_ms(
            args.reps, lambda: a.get_time_img(want_time=False, want_count=False), sync)
    for K in KS:
        ms = models_for(K, sl["velocity"])
        ids = np.random.default_rng(11).integers(0, K, n).astype(np.int32)
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_groups(ids, K)
        gain, info = merge(a, ms)   # (the buffers)
        labels.append("K%d warmup" % K)
        if args.quick:
            for _ in range(args.quick_reps):
                merge(a, ms)
                labels.append("K%d merge" % K)
            continue
        row = {"K": K, "passes": int(info.passes), "sum_sq": int(info.sum_sq)}
        assert project(a, ms).sum_sq == info.sum_sq   # one objective
        row["call_ms"], row["call_ms_all"] = median_ms(args.reps, lambda: merge(a, ms), sync)
        row["one_target_per_pass_call_ms"], _ = median_ms(args.reps, lambda: merge(a, ms, 1), sync)
        row["project_call_ms"], row["project_call_ms_all"] = median_ms(args.reps, lambda: project(a, ms), sync)
        row["over_k_plus_1_projections"] = round(row["call_ms"] / ((K + 1) * row["project_call_ms"]), 3)
        row["over_time_img_pass"] = round(row["call_ms"] / res["time_img_pass_ms"], 2)
        res["workloads"].append(row)
    a.close()
    if args.quick:
        with open(args.labels, "w") as f:
            json.dump(labels, f)
        print(json.dumps({"quick": True, "calls": len(labels)}))
        return
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def merge_trace(args):
    labels = json.load(open(args.labels))
    rows = []
    with open(args.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = next((k for k in KERNELS if k in r.get("Kernel_Name", "")), None)
            if name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    calls, cur = [], {}
    for s, e, name in rows:
        if name == "k_project_vote" and cur:
            calls.append(cur)
            cur = {}
        cur[name] = cur.get(name, 0.0) + (e - s) / 1e3
    if cur:
        calls.append(cur)
    if len(calls) != len(labels):
        raise SystemExit("the trace has %d calls, the labels %d" % (len(calls), len(labels)))
    per = {}
    for lab, c in zip(labels, calls):
        if "warmup" not in lab:
            per.setdefault(lab, []).append(c)
    out = {lab: {k: round(float(np.median([c.get(k, 0.0) for c in cs])), 2) for k in KERNELS} for lab, cs in per.items()}
    res = json.loads(open(args.out).read())
    res["kernel_us"] = out
    res["kernel_us_source"] = ("rocprofv3 --kernel-trace, a run of its own; per call the sum over its dispatches of one kernel, median "
                               "over %d calls per K" % args.quick_reps)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=3)
    ap.add_argument("--labels", default="merge_quick_labels.json")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_scores_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
