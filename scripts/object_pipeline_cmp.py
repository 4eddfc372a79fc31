#!/usr/bin/env python3
"""Two builds of bf_motion_compensator on the object pipeline's command line: do they write the same files?

    object_pipeline_cmp.py <parent binary> <new binary> <output directory> [--pairs 5] [--timeout 180]

Writes the three slices of tests/track_scene.py as one event file and runs both binaries on it under every flag set of FLAG_SETS,
`--pairs` times each, alternating parent and new.  Every run is a fresh child process under its own time limit; the first run that
exits non-zero, is signalled or runs out of time ends the script (exit 2) and nothing further is started.  Every pair's files are
compared by name and by bytes.  The table -- per flag set the file count, `same` or the first differing file, and the process wall
clock of both binaries (median, and the parent's min..max; library load included: a sanity figure, not a benchmark) -- goes to
standard output and to <output directory>/object_pipeline_cmp.txt.  Exit 1 when a flag set differs or wrote fewer than three
files (a comparison of nothing is a failure), else 0."""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLAG_SETS = [
    ["--objects=2"],
    ["--objects=2", "--objects-track"],
    ["--objects=2", "--objects-track", "--objects-wide"],
    ["--objects=4", "--objects-merge", "--objects-img", "--objects-flow"],
    ["--objects=4", "--objects-merge", "--objects-min-events=50", "--objects-track", "--objects-flow", "--objects-wide"],
    ["--objects=2", "--objects-track=1", "--objects-img"],
]


def run(exe, flags, scene, res, out, limit):
    """One run into the empty directory `out`; -> wall clock in s.  Ends the script on anything but a clean exit."""
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    cmd = [exe] + flags + ["--refresh-time=0.03", "--refresh-event-count=10000000", "--res-x=%d" % res[0], "--res-y=%d" % res[1],
                           "--quiet", "--img-prefix", out, scene]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, cwd=out, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("TIME LIMIT (%d s): %s" % (limit, " ".join(cmd)), flush=True)
        sys.exit(2)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        print("EXIT %d: %s\n%s" % (r.returncode, " ".join(cmd), r.stderr.decode(errors="replace")[-3000:]), flush=True)
        sys.exit(2)
    return dt


def first_difference(a, b):
    """-> (file count of a, None or what differs first)."""
    na, nb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if na != nb:
        return len(na), "names: %s" % sorted(set(na) ^ set(nb))[0]
    for name in na:
        with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
            if fa.read() != fb.read():
                return len(na), name
    return len(na), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=180)
    args = ap.parse_args()
    import numpy as np
    import track_scene
    from better_flow_amd import synth

    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    slices = track_scene.make()[0]
    scene = os.path.join(out, "scene.txt")
    synth.write_txt(scene, dict(fr_x=np.concatenate([s["fr_x"] for s in slices]), fr_y=np.concatenate([s["fr_y"] for s in slices]),
                                t=np.concatenate([s["t"] + s["t0_ns"] for s in slices])))
    res = (track_scene.H, track_scene.W)
    exes = {"parent": os.path.abspath(args.parent), "new": os.path.abspath(args.new)}
    rows, bad = [], False
    for flags in FLAG_SETS:
        times = {"parent": [], "new": []}
        files, differs = 0, None
        for _ in range(args.pairs):
            dirs = {}
            for who in ("parent", "new"):
                dirs[who] = os.path.join(out, who)
                times[who].append(run(exes[who], flags, scene, res, dirs[who], args.timeout))
            files, d = first_difference(dirs["parent"], dirs["new"])
            differs = differs or d
        verdict = differs or ("same" if files >= 3 else "FEWER THAN 3 FILES")
        bad = bad or verdict != "same"
        mp, mn = statistics.median(times["parent"]), statistics.median(times["new"])
        inside = "inside" if mn <= max(times["parent"]) else "ABOVE"
        rows.append("%-92s %5d  %-18s parent %.3f s (%.3f .. %.3f)  new %.3f s  %s" %
                    (" ".join(flags), files, verdict, mp, min(times["parent"]), max(times["parent"]), mn, inside))
        print(rows[-1], flush=True)
    head = "%-92s %5s  %-18s wall clock per process, median of %d (parent: min .. max); new median inside the parent's spread or below?" % (
        "flags", "files", "files", args.pairs)
    with open(os.path.join(out, "object_pipeline_cmp.txt"), "w") as f:
        f.write("\n".join([head] + rows) + "\n")
    for who in ("parent", "new"):
        shutil.rmtree(os.path.join(out, who), ignore_errors=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
