"""The per-event flow output at solve speed: the `with_flow_output` leg of the front-end record (5 M events, 346x260, rolling
30 ms slices of ~1 M events, binary input in the page cache) through the product command line, three ways:
  text       -o flow.txt                              (host walk over the kept history, StreamEngine::get_accumulated)
  bin        --outfile-bin=flow.bin                   (the table built on the device slice by slice, bf_emit_slice)
  text+bin   -o flow.txt --outfile-bin=flow.bin       (both files from the device table)
for the warm-start chain (one context) and for --stm-disable on four contexts.

    python scripts/flow_output_bench.py [--slices 5] [--reps 3] [--out DIR]

Prints one JSON line: per run the CLI's --timing record (stream_s: file open -> last model, with the emit step inside;
output_s: table -> files; output_bin_s: the binary file alone) and the process wall clock, best of --reps by stream_s."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from better_flow_amd import synth  # noqa: E402

CLI = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")


def one(path, d, extra, outputs, reps):
    args = [CLI, "--quiet", "--timing", "--res-x=260", "--res-y=346", "--max-events=1100000", "--span=0.03", "--refresh-time=0.03",
            "--refresh-event-count=1000000000"] + extra
    if "text" in outputs:
        args += ["-o", os.path.join(d, "flow.txt")]
    if "bin" in outputs:
        args += ["--outfile-bin=" + os.path.join(d, "flow.bin")]
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = subprocess.run(args + [path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr.decode()[-2000:])
        rec = json.loads([ln for ln in r.stderr.decode().splitlines() if ln.startswith("{")][-1])
        rec["process_wall_s"] = wall
        rec["stream_mevents_per_s"] = rec["events"] / rec["stream_s"] * 1e-6
        rec["stream_plus_output_mevents_per_s"] = rec["events"] / (rec["stream_s"] + rec["output_s"]) * 1e-6
        if best is None or rec["stream_s"] < best["stream_s"]:
            best = rec
    for f in ("flow.txt", "flow.bin"):
        p = os.path.join(d, f)
        if os.path.exists(p):
            best[f.replace(".", "_") + "_mb"] = os.path.getsize(p) / 1e6
            os.remove(p)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the input and output files (default: a temporary one)")
    a = ap.parse_args()
    d = a.out or tempfile.mkdtemp(prefix="bf_flowout_")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "stream.bin")
    n = synth.write_stream_bin(path, a.slices, 1000000, 260, 346)
    res = {"events": n, "host_cores": os.cpu_count(), "runs": {}}
    for chain, extra in (("warm_chain", []), ("stm_disable_4_contexts", ["--stm-disable", "--contexts=4"])):
        for outputs in (("text",), ("bin",), ("text", "bin")):
            res["runs"]["%s/%s" % (chain, "+".join(outputs))] = one(path, d, extra, outputs, a.reps)
    os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
