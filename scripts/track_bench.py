"""bf_track_keep and bf_track_overlap on the device: the config-4 slice (1M events, 346 x 260, scale 3), K = 2
and 8 groups under K translations, the ids a seeded uniform draw as in sections 17 and 19 (every wave carries every id), and the
same events stored by group, as a bf_run_groups sort leaves them (a wave then holds one id), and K = Kp = 64 (a wave of up to 64 distinct keys).

  timing    host wall clock around a synchronised call, median of --reps after a warm-up:
              keep_ms       bf_track_keep (no plane read back);
              project_ms    bf_project_groups with no output read back, in the same run on the same slice (the yardstick: the same
                            kernels);
              overlap_ms    bf_track_overlap against the plane just kept, dt = 30 ms;
              hold_ms       bf_hold_groups on the same slice and grouping (the yardstick: the same loads and warp per event).
  --quick   every device workload --quick-reps times, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/track_bench.py --quick).
  --kernel-trace FILE  the kernel trace CSV of such a run: the median time per kernel name is merged into --out.

Prints one JSON line and writes it to profiles/track_bench.json."""
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
WORKLOADS = ((2, False), (8, False), (2, True), (8, True), (64, False))   # (K, sorted by group first)
KERNELS = ("k_track_overlap", "k_hold_groups", "k_project_vote", "k_project_compose", "k_assign_box")
DT_NS = 30_000_000


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


def median_ms(reps, fn, sync):
    times = []
    for rep in range(reps + 1):   # the first run warms up (buffers grown on first use)
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    args = ap.parse_args()

    sl = synth.make_slice(args.events, H, W, 0.030, seed=4)
    n = len(sl["t"])
    a = accel.Accel(device=0, max_events=n, max_rows=S * H + S, max_cols=S * W + S)
    sync = lambda: a.L.bf_synchronize(a.h)
    result = dict(events=n, sensor=[H, W], scale=S, dt_ns=DT_NS, reps=args.reps, workloads=[])
    for K, sort_first in WORKLOADS:
        ids = np.random.default_rng(11).integers(0, K, n).astype(np.int32)
        ms = models_for(K, sl["velocity"])
        order = np.argsort(ids, kind="stable") if sort_first else np.arange(n)   # (stored by group: what a bf_run_groups sort leaves)
        ids = ids[order]
        a.upload_events(sl["fr_x"][order], sl["fr_y"][order], sl["t"][order])
        a.set_groups(ids, K)
        a.global_set_window(1, 5)
        calls = dict(keep_ms=lambda: a.track_keep(ms, S, (H, W), want_plane=False),
                     project_ms=lambda: a.project_groups(ms, S, (H, W), want=()),
                     overlap_ms=lambda: a.track_overlap(ms, DT_NS, S, (H, W)),
                     hold_ms=lambda: a.hold_groups(ms))
        rec = dict(K=K, sorted_by_group=sort_first)
        if args.quick:
            for _ in range(args.quick_reps):
                for fn in calls.values():
                    fn()
        else:
            for name, fn in calls.items():
                rec[name] = median_ms(args.reps, fn, sync)
            table, inside, info = a.track_overlap(ms, DT_NS, S, (H, W))
            rec.update(inside=int(inside.sum()), outside=int(info.outside), distinct_keys=int((table > 0).sum()))
        result["workloads"].append(rec)
    a.close()
    if args.kernel_trace:
        per = {}
        with open(args.kernel_trace) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for k in KERNELS:
                    if k in name:
                        per.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        result["kernel_us_median"] = {k: float(np.median(v)) for k, v in per.items()}
        result["kernel_calls"] = {k: len(v) for k, v in per.items()}
        if os.path.exists(args.out):   # merged into the timed run's record
            old = json.load(open(args.out))
            old["kernel_us_median"], old["kernel_calls"] = result["kernel_us_median"], result["kernel_calls"]
            result = old
    line = json.dumps(result)
    print(line)
    if not args.quick or args.kernel_trace:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
