"""bf_project_groups on the device: the config-4 slice (1M events, 346 x 260, scale 3), K = 2 and 8 groups
under K translations, the ids a seeded uniform draw (every wave carries every id: the worst case for a kernel whose model differs
per event), with the events stored in upload order, sorted by tile (after bf_run_tiles) and sorted by group (after bf_run_groups).

  timing    host wall clock around a synchronised call, median of --reps after a warm-up, the three images left on the device
            (`call_ms`) and read back (`call_readback_ms`).  Two yardsticks from the same run: the bf_get_time_img pass without
            read-back (`time_img_pass_ms`), and bf_assign_groups with the same grouping as its prior at the same K
            (`assign_prior_call_ms`): its vote pass also does one scatter per event.
  --alt-lib a second build of the library (an experiment build: `make -C better_flow_amd/csrc alt ALTX=-D...`), timed alternating
            with the product in the same process: the keys ending in `_alt`.
  --quick   every workload --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace -d DIR -- python scripts/project_groups_bench.py --quick [--alt-lib ...]); the order of the
            calls is written to --labels.
  --kernel-trace FILE  a kernel trace CSV of such a run: the k_project_* / k_assign_* dispatches, in start order, are matched to
            the labels and their median times per workload are merged into --out.

Prints one JSON line and writes it to profiles/project_groups_bench.json."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

H, W, S = 260, 346, 3
KS = (2, 8)
STORAGE = ("upload_order", "sorted_by_tile", "sorted_by_group")


def models_for(K, velocity):
    """Model 0 compensates the slice's own velocity; the others translations spread around it (seeded)."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(K):
        v = (velocity[0], velocity[1]) if k == 0 else (velocity[0] + rng.uniform(-300, 300), velocity[1] + rng.uniform(-300, 300))
        m = accel.Model()
        m.total_dx, m.total_dy = -v[0] * 1.27e-3, -v[1] * 1.27e-3
        out.append(m)
    return out


class Bench:
    def __init__(self, sl, lib=None):
        self.sl = sl
        self.acc = accel.Accel(device=0, max_events=len(sl["t"]), max_rows=S * H + S, max_cols=S * W + S, lib=lib)

    def sync(self):
        self.acc._chk(self.acc.L.bf_synchronize(self.acc.h))

    def store(self, storage, ids, K):
        a = self.acc
        a.upload_events(self.sl["fr_x"], self.sl["fr_y"], self.sl["t"])
        a.set_groups(ids, K)
        if storage == "sorted_by_tile":   # the counting sort of the tile grid leaves the events stored by tile, with a permutation
            a.run_tiles(32, 32, S, (H, W), (H // 32, W // 32), min_events=256, hard_iter_cap=20000)
        elif storage == "sorted_by_group":   # ... and the grouped solve stored by group (one iteration: only the sort matters here)
            a.run_groups(K, S, (H, W), (H, W), 1, hard_iter_cap=1)

    def project(self, models, readback):
        a = self.acc
        if readback:
            return a.project_groups(models, S, (H, W))
        K = len(models)
        o = accel.ProjectOpts(S, H, W, 0, 8)
        ms = (accel.Model * K)(*models)
        scores = (accel.GroupScore * K)()
        info = accel.ProjectInfo()
        a._chk(a.L.bf_project_groups(a.h, C.byref(o), ms, K, None, None, None, scores, C.byref(info)))
        return scores, info

    def assign_prior(self, models):
        a = self.acc
        K = len(models)
        o = accel.AssignOpts(S, H, W, 0, 1, 1, 0, 0)   # use_prior, no install: the held grouping stays
        ms = (accel.Model * K)(*models)
        a._chk(a.L.bf_assign_groups(a.h, C.byref(o), ms, K, None, None, None, None))


def median_ms(reps, fn, sync):
    times = []
    for rep in range(reps + 1):   # the first run warms up (buffers grown on first use)
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep:
            times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 4), [round(t * 1e3, 4) for t in times]


def label(K, storage, what, lib):
    return "K%d %s %s %s" % (K, storage, what, lib)


def run(args):
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    n = len(sl["t"])
    libs = [("product", Bench(sl))]
    if args.alt_lib:
        libs.append(("alt", Bench(sl, lib=args.alt_lib)))
    res = {"events": int(n), "sensor": [H, W], "scale": S, "window": [S * H, S * W], "workloads": []}
    labels = []
    if not args.quick:
        b = libs[0][1]
        b.acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        b.acc.set_cloud(S, H, W)
        res["time_img_pass_ms"], res["time_img_pass_ms_all"] = median_ms(
            args.reps, lambda: b.acc.get_time_img(want_time=False, want_count=False), b.sync)
    for K in KS:
        ms = models_for(K, sl["velocity"])
        ids = np.random.default_rng(11).integers(0, K, n).astype(np.int32)
        for storage in STORAGE:
            row = {"K": K, "stored": storage}
            try:
                for name, b in libs:
                    b.store(storage, ids, K)
            except accel.BfError as e:   # (a storage order this slice cannot be brought into)
                row["skipped"] = str(e)
                res["workloads"].append(row)
                continue
            for name, b in libs:
                b.project(ms, False)   # (the buffers)
                labels.append(label(K, storage, "warmup", name))
                b.assign_prior(ms)
                labels.append(label(K, storage, "warmup", name))
            if args.quick:
                for _ in range(args.quick_reps):
                    for name, b in libs:
                        b.project(ms, False)
                        labels.append(label(K, storage, "project", name))
                    libs[0][1].assign_prior(ms)
                    labels.append(label(K, storage, "assign_prior", "product"))
                continue
            # alternating, so that both builds see the same neighbours on the machine
            t = {name: [] for name, _ in libs}
            for rep in range(args.reps + 1):
                for name, b in libs:
                    b.sync()
                    t0 = time.perf_counter()
                    out = b.project(ms, False)
                    b.sync()
                    if rep:
                        t[name].append(time.perf_counter() - t0)
                    row["sum_sq" + ("" if name == "product" else "_" + name)] = int(out[1].sum_sq)
            for name, _ in libs:
                sfx = "" if name == "product" else "_" + name
                row["call_ms" + sfx] = round(float(np.median(t[name])) * 1e3, 4)
                row["call_ms_all" + sfx] = [round(x * 1e3, 4) for x in t[name]]
            b = libs[0][1]
            row["call_readback_ms"], _ = median_ms(args.reps, lambda: b.project(ms, True), b.sync)
            row["assign_prior_call_ms"], row["assign_prior_call_ms_all"] = median_ms(args.reps, lambda: b.assign_prior(ms), b.sync)
            row["over_time_img_pass"] = round(row["call_ms"] / res["time_img_pass_ms"], 3)
            row["over_assign_prior"] = round(row["call_ms"] / row["assign_prior_call_ms"], 3)
            res["workloads"].append(row)
    for _, b in libs:
        b.acc.close()
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
    """The k_project_* / k_assign_* dispatches of a --quick run, in start order: a call begins at its vote kernel, and is that,
    a box sum and a compose (projection) or pick (assignment) kernel."""
    labels = json.load(open(args.labels))
    rows = []
    with open(args.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_project_" in name or "k_assign_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    kind = lambda n: next(k for k in ("vote", "box", "compose", "pick") if "_" + k in n)
    calls, cur = [], {}
    for s, e, n in rows:
        k = kind(n)
        if k == "vote" and cur:
            calls.append(cur)
            cur = {}
        cur[k] = (e - s) / 1e3
    if cur:
        calls.append(cur)
    if len(calls) != len(labels):
        raise SystemExit("the trace has %d calls, the labels %d" % (len(calls), len(labels)))
    per = {}
    for lab, c in zip(labels, calls):
        if " warmup " not in lab:
            per.setdefault(lab, []).append(c)
    out = {lab: {k: round(float(np.median([c[k] for c in cs if k in c])), 2) for k in ("vote", "box", "compose", "pick") if any(k in c for c in cs)}
           for lab, cs in per.items()}
    res = json.loads(open(args.out).read())
    res["kernel_us"] = out
    res["kernel_us_source"] = "rocprofv3 --kernel-trace, a run of its own; median over %d calls per workload" % args.quick_reps
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=3)
    ap.add_argument("--alt-lib", default="")
    ap.add_argument("--labels", default="project_quick_labels.json")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_groups_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
