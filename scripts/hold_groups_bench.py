"""bf_hold_groups and bf_group_flow_medians on the device: the config-4 slice (1M events, 346 x 260), K = 2 and
8 groups under K translations, the ids a seeded uniform draw as in section 17 (every wave carries every id); and K = 2 under
four-parameter models (rotation and divergence about the sensor's centre), where no two events of a group share a flow.

  timing    host wall clock around a synchronised call, median of --reps after a warm-up:
              hold_groups_ms        bf_hold_groups;
              hold_best_ms          bf_global_hold_best in the same run, on the same slice and window (the yardstick: the same
                                    traffic per event, no warp arithmetic);
              medians_ms            bf_group_flow_medians on the flow bf_hold_groups left;
              host_group_flows_ms   the step it replaces, what bf::ObjectFinder::group_flows does per group: the group's events
                                    uploaded again, bf_set_cloud, bf_set_model, bf_writeout_events through the same C-ABI, then
                                    compute_uv and a sort per axis on the host (here numpy's hypot and sort).
            `medians_equal_host` says whether the two medians agree to the derived 4 * 2^-52 * max|u_i| (the device's own hypot).
  --quick   every device workload --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/hold_groups_bench.py --quick).
  --kernel-trace FILE  the kernel trace CSV of such a run: the median time per kernel name of this file's kernels and of
            k_global_hold_best is merged into --out.

Prints one JSON line and writes it to profiles/hold_groups_bench.json."""
import argparse
import csv
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
WORKLOADS = ((2, "translations"), (8, "translations"), (2, "four_parameter"))
KERNELS = ("k_hold_groups", "k_global_hold_best", "k_median_count", "k_median_pick")


def models_for(K, velocity, kind="translations"):
    """Model 0 compensates the slice's own velocity; the others translations spread around it (seeded).  four_parameter: every
    model also rotates and diverges about the sensor's centre, so that the flow differs from event to event."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(K):
        v = (velocity[0], velocity[1]) if k == 0 else (velocity[0] + rng.uniform(-300, 300), velocity[1] + rng.uniform(-300, 300))
        m = accel.Model()
        m.total_dx, m.total_dy = -v[0] * 1.27e-3, -v[1] * 1.27e-3
        if kind == "four_parameter":
            m.cx, m.cy = H / 2.0, W / 2.0
            m.total_rot, m.total_div = rng.uniform(-2e-3, 2e-3, 2)
        out.append(m)
    return out


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


def host_group_flows(acc, sl, ids, models):
    """bf::ObjectFinder::group_flows: K uploads, K write-outs, compute_uv and a sort per group and axis on the host."""
    um, vm = np.zeros(len(models)), np.zeros(len(models))
    for k, m in enumerate(models):
        sel = ids == k
        if not sel.any():
            continue
        acc.upload_events(sl["fr_x"][sel], sl["fr_y"][sel], sl["t"][sel])
        acc.set_cloud(S, H, W)
        acc.set_model(m)
        _, _, nx, ny = acc.writeout_events()
        ln = np.hypot(nx, ny)
        speed = ln / (127.0 / 100000.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = np.where(ln == 0, 0.0, speed * nx / ln)
            v = np.where(ln == 0, 0.0, speed * ny / ln)
        for out, a in ((um, u), (vm, v)):
            a = np.sort(a)
            c = len(a)
            out[k] = a[c // 2] if c % 2 else 0.5 * (a[c // 2 - 1] + a[c // 2])
    return um, vm


def run(args):
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n, max_rows=S * H + S, max_cols=S * W + S)
    sync = lambda: acc._chk(acc.L.bf_synchronize(acc.h))
    res = {"events": int(n), "sensor": [H, W], "workloads": []}
    for K, kind in WORKLOADS:
        ms = models_for(K, sl["velocity"], kind)
        ids = np.random.default_rng(11).integers(0, K, n).astype(np.int32)

        def stage():
            acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
            acc.global_set_window(1, 5)
            acc.set_groups(ids, K)

        stage()
        if args.quick:
            for _ in range(args.quick_reps + 1):
                acc.global_hold_best()
                acc.hold_groups(ms)
                acc.group_flow_medians()
            continue
        row = {"K": K, "models": kind}
        row["hold_best_ms"], row["hold_best_ms_all"] = median_ms(args.reps, acc.global_hold_best, sync)
        row["hold_groups_ms"], row["hold_groups_ms_all"] = median_ms(args.reps, lambda: acc.hold_groups(ms), sync)
        row["medians_ms"], row["medians_ms_all"] = median_ms(args.reps, acc.group_flow_medians, sync)
        um, vm, counts = acc.group_flow_medians()
        flow = acc.global_get_flow(keys=("u", "v"))
        row["counts"] = counts.tolist()
        row["host_group_flows_ms"], row["host_group_flows_ms_all"] = median_ms(args.reps, lambda: host_group_flows(acc, sl, ids, ms), sync)
        hu, hv = host_group_flows(acc, sl, ids, ms)
        bound = [4 * 2.0 ** -52 * max(np.abs(flow["u"][ids == k]).max(), np.abs(flow["v"][ids == k]).max()) for k in range(K)]
        row["medians_equal_host"] = bool(all(abs(um[k] - hu[k]) <= bound[k] and abs(vm[k] - hv[k]) <= bound[k] for k in range(K)))
        row["hold_groups_over_hold_best"] = round(row["hold_groups_ms"] / row["hold_best_ms"], 3)
        row["host_over_device_medians"] = round(row["host_group_flows_ms"] / row["medians_ms"], 2)
        res["workloads"].append(row)
    acc.close()
    if args.quick:
        print(json.dumps({"quick": True}))
        return
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def merge_trace(args):
    """Per kernel name its dispatches in start order, in as many equal parts as there are workloads (the same calls at each)."""
    per = {k: [] for k in KERNELS}
    with open(args.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k in KERNELS:
                if k in name:
                    per[k].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    res = json.loads(open(args.out).read())
    out = {}
    for k, v in per.items():
        v.sort()
        per_w = len(v) // len(WORKLOADS)
        for i, (K, kind) in enumerate(WORKLOADS):
            d = [x[1] for x in v[i * per_w:(i + 1) * per_w]]
            if d:
                out["K%d %s %s" % (K, kind, k)] = {"dispatches": len(d), "median": round(float(np.median(d)), 2), "min": round(min(d), 2),
                                          "max": round(max(d), 2), "sum_per_call": round(sum(d) / (args.quick_reps + 1), 2)}
    res["kernel_us"] = out
    res["kernel_us_source"] = "rocprofv3 --kernel-trace, a run of its own (--quick, %d calls per workload and K)" % (args.quick_reps + 1)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=3)
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hold_groups_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
