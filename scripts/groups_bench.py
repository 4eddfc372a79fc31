"""bf_run_groups on the device, next to what it extends and what it replaces:

  (a) the config-4 slice (1M events, 346 x 260, 32 x 32 tiles, scale 3) with its tile ids as groups: bf_run_groups against
      bf_run_tiles of the same build.  Both run the same optimizer on the same runs of events; the difference is the keyed
      sort, the box pass and the host's sizing round trip.  The split comes from the context's profile (hipEvents around the
      sort + boxes and around the optimizer launch) in runs of their own.
  (b) the two-motion scene's four groups, and a 64-object variant (the scene's patch replicated on an 8 x 8 lattice of a
      346 x 260 sensor): bf_run_groups -- one upload, bf_set_groups, one call -- against what the C-ABI offered before, one
      context doing upload + bf_set_cloud + bf_set_model + bf_run per group, uploads included in both.

Timing: host wall clock around synchronised calls, median of --reps after a warm-up.  Prints one JSON line and writes it to
profiles/groups_bench.json.  --quick: every workload once, untimed (for a profiler run: rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import groups_ref as gr  # noqa: E402
import segment_scene as scene  # noqa: E402
from better_flow_amd import accel, synth  # noqa: E402

HARD_CAP = 20000


def median_of(reps, fn, sync):
    times = []
    for rep in range(reps + 1):                      # the first run warms up (buffers grown on first use)
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if rep:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(t * 1e3, 4) for t in times], out


def split(acc, fn):
    """(sort + boxes ms, optimizer ms) of one call from the context's profile."""
    acc.profile_enable(1)
    acc.profile_reset()
    fn()
    p = acc.profile_get()
    acc.profile_enable(0)
    return round(p.other_ms, 4), round(p.warp_scatter_ms, 4)


def against_the_tile_grid(reps, quick):
    H, W, S, G, ME = 260, 346, 3, 32, 256
    sl = synth.make_slice(1000000, H, W, 0.030, seed=1)
    n = len(sl["t"])
    tid = (np.minimum(sl["fr_x"].astype(np.int64) * G // H, G - 1) * G +
           np.minimum(sl["fr_y"].astype(np.int64) * G // W, G - 1)).astype(np.int32)
    guard = (H // G, W // G)
    acc = accel.Accel(device=0, max_events=n, max_rows=S * H + S, max_cols=S * W + S)
    sync = lambda: acc._chk(acc.L.bf_synchronize(acc.h))
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    acc.set_groups(tid, G * G)
    tiles = lambda: acc.run_tiles(G, G, S, (H, W), guard, min_events=ME, hard_iter_cap=HARD_CAP)
    groups = lambda: acc.run_groups(G * G, S, (H, W), guard, ME, hard_iter_cap=HARD_CAP)
    res = {"events": int(n), "sensor": [H, W], "grid": [G, G], "scale": S}
    if quick:
        tiles()
        groups()
    else:
        # alternating, so that both see the same neighbours on the machine
        t_t, t_g = [], []
        for rep in range(reps + 1):
            for fn, sink in ((tiles, t_t), (groups, t_g)):
                sync()
                t0 = time.perf_counter()
                out = fn()
                sync()
                if rep:
                    sink.append(time.perf_counter() - t0)
        res["run_tiles_ms"] = round(float(np.median(t_t)) * 1e3, 4)
        res["run_groups_ms"] = round(float(np.median(t_g)) * 1e3, 4)
        res["run_tiles_ms_all"] = [round(t * 1e3, 4) for t in t_t]
        res["run_groups_ms_all"] = [round(t * 1e3, 4) for t in t_g]
        res["groups_over_tiles"] = round(res["run_groups_ms"] / res["run_tiles_ms"], 4)
        res["run_tiles_split_ms"] = dict(zip(("sort", "optimizer"), split(acc, tiles)))
        res["run_groups_split_ms"] = dict(zip(("sort_and_boxes", "optimizer"), split(acc, groups)))
        res["iterations_max"] = int(max(i.iterations for i in out[1]))
    res["groups_lds_bytes"] = int(acc.get_stat("groups_lds"))
    res["groups_work_groups_per_cu"] = int(acc.get_stat("groups_per_cu"))
    acc.close()
    return res


def lattice_scene():
    """The scene's patch on an 8 x 8 lattice of a 346 x 260 sensor: 64 groups of 9600 events."""
    sc = scene.make()
    p = sc["is_patch"]
    x0, y0, t0 = sc["fr_x"][p], sc["fr_y"][p], sc["t"][p]
    xs, ys, ts, gs = [], [], [], []
    for r in range(8):
        for c in range(8):
            xs.append(x0 - x0.min() + 2 + r * 32)
            ys.append(y0 - y0.min() + 2 + c * 43)
            ts.append(t0)
            gs.append(np.full(len(t0), r * 8 + c, dtype=np.int32))
    order = np.argsort(np.concatenate(ts), kind="stable")
    cat = lambda a: np.concatenate(a)[order]
    return dict(fr_x=cat(xs).astype(np.int32), fr_y=cat(ys).astype(np.int32), t=cat(ts)), cat(gs), 64, (260, 346)


def against_one_context_per_group(name, sl, gid, K, res_hw, warm, reps, quick):
    H, W = res_hw
    S, GUARD, ME = 3, (90, 120), 100
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n, max_rows=S * H + S, max_cols=S * W + S)
    sync = lambda: acc._chk(acc.L.bf_synchronize(acc.h))
    wm = None
    if warm is not None:
        wm = accel.Model(**{k: getattr(warm, k) for k, _ in gr.oracle.Model._fields_})
    subsets = [np.flatnonzero(gid == g) for g in range(K)]
    cols = [tuple(np.ascontiguousarray(sl[k][idx]) for k in ("fr_x", "fr_y", "t")) for idx in subsets]
    o = acc.default_opts()
    o.res_x, o.res_y, o.min_events, o.hard_iter_cap = GUARD[0], GUARD[1], ME, HARD_CAP

    def grouped():
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        acc.set_groups(gid, K)
        return acc.run_groups(K, S, (H, W), GUARD, ME, warm=wm, hard_iter_cap=HARD_CAP)

    def one_by_one():
        its = []
        for x, y, t in cols:
            acc.upload_events(x, y, t)
            acc.set_cloud(S, H, W)
            if wm is not None:
                acc.set_model(wm)
            its.append(acc.run(o)[2].iterations)
        return its

    res = {"scene": name, "events": int(n), "groups": K, "sensor": [H, W], "scale": S, "warm": warm is not None}
    if quick:
        grouped()
        one_by_one()
    else:
        g_ms, g_all, out = median_of(reps, grouped, sync)
        s_ms, s_all, its = median_of(reps, one_by_one, sync)
        res.update(run_groups_ms=round(g_ms * 1e3, 4), one_by_one_ms=round(s_ms * 1e3, 4), run_groups_ms_all=g_all,
                   one_by_one_ms_all=s_all, one_by_one_over_groups=round(s_ms / g_ms, 3),
                   iterations_groups=[int(i.iterations) for i in out[1]][:8], iterations_one_by_one=[int(i) for i in its][:8],
                   rc_groups=sorted(set(int(i.rc) for i in out[1])))
    res["groups_lds_bytes"] = int(acc.get_stat("groups_lds"))
    res["groups_work_groups_per_cu"] = int(acc.get_stat("groups_per_cu"))
    acc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="every workload once, untimed (profiler runs)")
    ap.add_argument("--only", default="", choices=("", "a", "b4", "b64"), help="one workload only (a profiler run per workload)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_bench.json"))
    a = ap.parse_args()
    sc = scene.make()
    res = {"b_per_group": []}
    if a.only in ("", "a"):
        res["a_tile_grid"] = against_the_tile_grid(a.reps, a.quick)
    if a.only in ("", "b4"):
        res["b_per_group"].append(against_one_context_per_group("scene, 4 groups, cold", sc, gr.scene_groups(sc), 4, (scene.H, scene.W),
                                                                None, a.reps, a.quick))
        res["b_per_group"].append(against_one_context_per_group("scene, 4 groups, warm", sc, gr.scene_groups(sc), 4, (scene.H, scene.W),
                                                                gr.background_model(), a.reps, a.quick))
    if a.only in ("", "b64"):
        lat, gid, K, hw = lattice_scene()
        res["b_per_group"].append(against_one_context_per_group("patch x 64 on 346x260, cold", lat, gid, K, hw, None, a.reps, a.quick))
    line = json.dumps(res)
    print(line)
    if not a.quick and not a.only:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
