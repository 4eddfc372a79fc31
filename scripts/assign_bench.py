"""bf_assign_groups on the device: the config-4 slice (1M events, 346 x 260, scale 3), K = 2 and 8 candidate
translations, a first round (no prior) and a round with the first round's result as its prior, with the events stored in
upload order and stored sorted by tile (after bf_run_tiles).

  timing    host wall clock around a synchronised call, median of --reps after a warm-up: the call as the C-ABI offers it
            without per-event read-back (ids and scores stay on the device; `call_ms`) and with it (`call_readback_ms`).
            Yardstick: the bf_get_time_img pass without read-back on the same slice (`time_img_pass_ms`) -- a first round does
            K warps and scatters, so K passes; a round with a prior does one scatter per event, so one pass plus K gathers.
  --alt-lib a second build of the library (an experiment build: `make -C better_flow_amd/csrc alt ALTX=-D...`), timed alternating
            with the product in the same process: the keys ending in `_alt`.
  --quick   every workload --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace -d DIR -- python scripts/assign_bench.py --quick [--alt-lib ...]); the order of the calls is
            written to --labels.
  --kernel-trace FILE  a kernel trace CSV of such a run: the k_assign_* dispatches, in start order, are matched to the labels
            and their median times per workload are merged into --out.

Prints one JSON line and writes it to profiles/assign_bench.json."""
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

    def store(self, sorted_):
        a = self.acc
        a.upload_events(self.sl["fr_x"], self.sl["fr_y"], self.sl["t"])
        if sorted_:   # the counting sort of the tile grid leaves the events stored by tile, with a permutation
            a.run_tiles(32, 32, S, (H, W), (H // 32, W // 32), min_events=256, hard_iter_cap=20000)

    def call(self, models, use_prior, readback):
        a = self.acc
        if readback:
            return a.assign_groups(models, S, (H, W), use_prior=use_prior, install=not use_prior)
        K = len(models)
        o = accel.AssignOpts(S, H, W, 0, 1, 1 if use_prior else 0, 0 if use_prior else 1, 0)
        ms = (accel.Model * K)(*models)
        counts = np.zeros(K + 1, dtype=np.int32)
        info = accel.AssignInfo()
        a._chk(a.L.bf_assign_groups(a.h, C.byref(o), ms, K, None, None, counts.ctypes.data_as(C.c_void_p), C.byref(info)))
        return counts, info


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


def workloads():
    for K in KS:
        for sorted_ in (False, True):
            yield K, sorted_


def label(K, sorted_, use_prior, lib):
    return "K%d %s %s %s" % (K, "sorted" if sorted_ else "upload_order", "prior" if use_prior else "first", lib)


def run(args):
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    libs = [("product", Bench(sl))]
    if args.alt_lib:
        libs.append(("alt", Bench(sl, lib=args.alt_lib)))
    res = {"events": int(len(sl["t"])), "sensor": [H, W], "scale": S, "window": [S * (H - 1) + S, S * (W - 1) + S], "workloads": []}
    labels = []
    if not args.quick:
        b = libs[0][1]
        b.store(False)
        b.acc.set_cloud(S, H, W)
        res["time_img_pass_ms"], res["time_img_pass_ms_all"] = median_ms(
            args.reps, lambda: b.acc.get_time_img(want_time=False, want_count=False), b.sync)
    for K, sorted_ in workloads():
        ms = models_for(K, sl["velocity"])
        row = {"K": K, "stored": "sorted" if sorted_ else "upload_order"}
        for name, b in libs:
            b.store(sorted_)
            b.call(ms, False, False)   # (the prior of the rounds below, and the buffers)
            labels.append("warmup")
        for use_prior in (False, True):
            key = "prior" if use_prior else "first"
            if args.quick:
                for _ in range(args.quick_reps):
                    for name, b in libs:
                        b.call(ms, use_prior, False)
                        labels.append(label(K, sorted_, use_prior, name))
                continue
            # alternating, so that both builds see the same neighbours on the machine
            t = {name: [] for name, _ in libs}
            for rep in range(args.reps + 1):
                for name, b in libs:
                    b.sync()
                    t0 = time.perf_counter()
                    out = b.call(ms, use_prior, False)
                    b.sync()
                    if rep:
                        t[name].append(time.perf_counter() - t0)
                    if name == "product":
                        row[key + "_counts"] = out[0].tolist()
                        row[key + "_changed"] = int(out[1].changed)
            for name, _ in libs:
                row["%s_call_ms%s" % (key, "" if name == "product" else "_" + name)] = round(float(np.median(t[name])) * 1e3, 4)
                row["%s_call_ms_all%s" % (key, "" if name == "product" else "_" + name)] = [round(x * 1e3, 4) for x in t[name]]
            b = libs[0][1]
            row[key + "_call_readback_ms"], _ = median_ms(args.reps, lambda: b.call(ms, use_prior, True), b.sync)
            yard = res["time_img_pass_ms"] * (K if not use_prior else 1)
            row[key + "_over_yardstick"] = round(row[key + "_call_ms"] / yard, 3)
        res["workloads"].append(row)
    for _, b in libs:
        b.acc.close()
    if args.quick:
        with open(args.labels, "w") as f:
            json.dump(labels, f)
        print(json.dumps({"quick": True, "calls": len(labels)}))
        return
    res["yardstick"] = "first round: K x time_img_pass_ms; round with a prior: 1 x time_img_pass_ms (plus K gathers, not priced)"
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def merge_trace(args):
    """The k_assign_* dispatches of a --quick run, in start order: one call is a vote, a box and a pick kernel."""
    labels = json.load(open(args.labels))
    rows = []
    with open(args.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_assign_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    kind = lambda n: "vote" if "k_assign_vote" in n else ("box" if "k_assign_box" in n else "pick")
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
        raise SystemExit("the trace has %d assignment calls, the labels %d" % (len(calls), len(labels)))
    out, per = {}, {}
    for lab, c in zip(labels, calls):
        if lab != "warmup":
            per.setdefault(lab, []).append(c)
    for lab, cs in per.items():
        out[lab] = {k: round(float(np.median([c[k] for c in cs if k in c])), 2) for k in ("vote", "box", "pick") if any(k in c for c in cs)}
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
    ap.add_argument("--labels", default="assign_quick_labels.json")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
