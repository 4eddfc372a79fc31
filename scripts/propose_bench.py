"""bf_propose_models on the device: the config-4 slice (1M events, 346 x 260) after an exhaustive search over
the default 180 x 80 lattice (scale 1, a 5-pixel window), default options (radius 1, suppress 2, eight models).

  timing    host wall clock around a synchronised call that brings back the models, the proposals and the info (no planes),
            median of --reps after a warm-up (`call_ms`); the search that precedes it once (`search_ms`), and the share of a
            search plus a proposal that the proposal is.  Yardstick: the bf_get_time_img pass without read-back on the same slice
            in the same run (`time_img_pass_ms`), as in DESIGN section 15.
  --alt-lib a second build of the library (`make -C better_flow_amd/csrc alt ALTX=-DBF_PROPOSE_FOLD`), timed alternating with the
            product in the same process: the keys ending in `_alt`; with --fold-out the pair is also written there.
  --quick   the search, then the call --quick-reps times per build, untimed, for a profiler run of its own
            (rocprofv3 --kernel-trace -d DIR -- python scripts/propose_bench.py --quick [--alt-lib ...]).
  --kernel-trace FILE  the kernel trace CSV of such a run: the k_propose_* dispatches in start order, product and alt
            alternating, their median times merged into --out (and --fold-out).

Prints one JSON line and writes it to profiles/propose_bench.json."""
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
K = 8


class Bench:
    def __init__(self, sl, lib=None):
        self.acc = accel.Accel(device=0, max_events=len(sl["t"]), max_rows=S * H + S, max_cols=S * W + S, lib=lib)
        self.sl = sl
        self.lattice = accel.Accel.global_search_opts()
        self.opts = accel.AccelProposeOpts(1, 2, K, 1)
        self.models = (accel.Model * K)()
        self.props = (accel.Proposal * K)()
        self.info = accel.ProposeInfo()

    def sync(self):
        self.acc._chk(self.acc.L.bf_synchronize(self.acc.h))

    def search(self):
        a = self.acc
        a.upload_events(self.sl["fr_x"], self.sl["fr_y"], self.sl["t"])
        a.global_set_window(1, 5)
        self.sync()
        t0 = time.perf_counter()
        a.global_search(self.lattice, want_surface=False)
        self.sync()
        return (time.perf_counter() - t0) * 1e3

    def call(self):
        a = self.acc
        a._chk(a.L.bf_propose_models(a.h, C.byref(self.lattice), C.byref(self.opts), self.models, self.props, K, None, None, 0,
                                     C.byref(self.info)))


def run(args):
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    libs = [("product", Bench(sl))]
    if args.alt_lib:
        libs.append(("alt", Bench(sl, lib=args.alt_lib)))
    res = {"events": int(len(sl["t"])), "sensor": [H, W], "lattice": [180, 80], "search": "scale 1, window 5, default lattice",
           "options": {"radius": 1, "suppress": 2, "max_models": K, "min_votes": 1}}
    if not args.quick:
        b = libs[0][1]
        b.acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        b.acc.set_cloud(S, H, W)
        t = []
        for rep in range(args.reps + 1):
            b.sync()
            t0 = time.perf_counter()
            b.acc.get_time_img(want_time=False, want_count=False)
            b.sync()
            if rep:
                t.append(time.perf_counter() - t0)
        res["time_img_pass_ms"] = round(float(np.median(t)) * 1e3, 4)
    for name, b in libs:
        ms = b.search()
        b.call()   # (the buffers, grown on first use)
        if name == "product":
            res["search_ms"] = round(ms, 2)
            res["propose_form"] = int(b.acc.get_stat("propose_form"))
            res["info"] = {k: int(getattr(b.info, k)) for k in ("n_x", "n_y", "voted", "unscored", "off_lattice", "proposals")}
            res["proposals"] = [[round(p.u, 1), round(p.v, 1), int(p.votes), int(p.peak)] for p in list(b.props)[:b.info.proposals]]
            res["true_velocity"] = [float(v) for v in sl["velocity"]]
    if args.quick:
        for _ in range(args.quick_reps):
            for _, b in libs:
                b.call()
        for _, b in libs:
            b.acc.close()
        print(json.dumps({"quick": True, "calls_per_build": args.quick_reps + 1, "builds": [n for n, _ in libs]}))
        return
    t = {name: [] for name, _ in libs}
    for rep in range(args.reps + 1):   # alternating, so that both builds see the same neighbours on the machine
        for name, b in libs:
            b.sync()
            t0 = time.perf_counter()
            b.call()
            b.sync()
            if rep:
                t[name].append(time.perf_counter() - t0)
    for name, _ in libs:
        sfx = "" if name == "product" else "_" + name
        res["call_ms" + sfx] = round(float(np.median(t[name])) * 1e3, 4)
        res["call_ms_all" + sfx] = [round(x * 1e3, 4) for x in t[name]]
    res["call_over_time_img_pass"] = round(res["call_ms"] / res["time_img_pass_ms"], 2)
    res["share_of_search_plus_proposal"] = round(res["call_ms"] / (res["call_ms"] + res["search_ms"]), 6)
    for _, b in libs:
        b.acc.close()
    finish(args, res)


def finish(args, res):
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if args.fold_out and ("call_ms_alt" in res or "kernel_us_alt" in res):
        fold = {"what": "k_propose_vote, LDS form: plain (product) against the two-round fold of the wave's leading bins (alt, "
                        "-DBF_PROPOSE_FOLD), both builds alternating in one process",
                "events": res["events"], "info": res.get("info")}
        for k in ("call_ms", "call_ms_all", "call_ms_alt", "call_ms_all_alt", "kernel_us", "kernel_us_alt"):
            if k in res:
                fold[k] = res[k]
        with open(args.fold_out, "w") as f:
            f.write(json.dumps(fold) + "\n")


def merge_trace(args):
    """The k_propose_* dispatches of a --quick run in start order: a call is a vote, a box and a pick kernel; the first call of
    every build is its warm-up, the others alternate product, alt."""
    builds = ["product", "alt"] if args.alt_lib else ["product"]
    rows = []
    with open(args.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_propose_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    kind = lambda n: "vote" if "k_propose_vote" in n else ("box" if "k_propose_box" in n else "pick")
    calls, cur = [], {}
    for s, e, n in rows:
        k = kind(n)
        if k == "vote" and cur:
            calls.append(cur)
            cur = {}
        cur[k] = (e - s) / 1e3
    if cur:
        calls.append(cur)
    timed = calls[len(builds):]
    if len(timed) != args.quick_reps * len(builds):
        raise SystemExit("the trace has %d proposal calls, expected %d" % (len(calls), (args.quick_reps + 1) * len(builds)))
    res = json.loads(open(args.out).read())
    for i, name in enumerate(builds):
        mine = timed[i::len(builds)]
        res["kernel_us" + ("" if name == "product" else "_" + name)] = {
            k: round(float(np.median([c[k] for c in mine])), 2) for k in ("vote", "box", "pick")}
    res["kernel_us_source"] = "rocprofv3 --kernel-trace, a run of its own; median over %d calls per build" % args.quick_reps
    finish(args, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--quick-reps", type=int, default=5)
    ap.add_argument("--alt-lib", default="")
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propose_bench.json"))
    ap.add_argument("--fold-out", default="")
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
