"""--flow-img throughput, on the two streams scripts/frame_output_bench.py uses (a 2M-event 240 x 180
stream and a 1M-event 346 x 260 stream, synth.write_stream_bin).

Per stream, three runs of the product command line into the same directory:
  plain        --engine=stream                      the stream engine without frames: what --flow-img is added to
  stream_flow  --engine=stream --flow-img           the flow frame composed on the device (bf_flow_frame_*), written by a thread
  ring_flow    --engine=ring --flow-img             DVS_flow: three synchronous tiles read back per slice, composed on the host
Reports frames/s (whole-process wall clock), the stream engine's stream-phase seconds and time spent waiting for frames
(--timing), and stream_flow's frames/s over ring_flow's.  One JSON record per line on stdout (and in --out).

    python scripts/flow_frame_bench.py [--work DIR] [--out FILE] [--quick]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from better_flow_amd import synth  # noqa: E402

CLI = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")


def run(args, out_dir, timeout):
    if os.path.exists(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    t0 = time.perf_counter()
    r = subprocess.run([CLI] + args, cwd=out_dir, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (args, r.stderr.decode()[-1000:]))
    timing = [json.loads(l) for l in r.stderr.decode().splitlines() if l.startswith("{")]
    sizes = {f: os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    return wall, sizes, (timing[-1] if timing else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/bf_flow_frame_bench")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a tenth of the events (a smoke run of the script)")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    div = 10 if a.quick else 1
    records = []
    for name, W, H, slices in (("240x180", 240, 180, 100 // div), ("346x260", 346, 260, 50 // div)):
        path = os.path.join(a.work, "stream_%s.bin" % name)
        n = synth.write_stream_bin(path, slices, 20000, H, W)
        out_dir = os.path.join(a.work, "out")
        fps = {}
        for run_name, engine, outs in (("plain", "stream", []), ("stream_flow", "stream", ["--flow-img"]), ("ring_flow", "ring", ["--flow-img"])):
            args = ["--engine=" + engine, "--res-x=%d" % H, "--res-y=%d" % W, "--quiet", "--img-prefix", out_dir] + outs
            if engine == "stream":
                args.append("--timing")
            wall, sizes, timing = run(args + [path], out_dir, 1800)
            frames = sum(f.endswith(".ppm") for f in sizes)
            rec = {"stream": name, "events": n, "run": run_name, "frames": frames, "bytes": sum(sizes.values()), "wall_s": round(wall, 3),
                   "frames_per_s": round(frames / wall, 2), "mevents_per_s": round(n / wall * 1e-6, 3)}
            if timing:
                rec.update({"slices": timing["slices"], "stream_s": timing["stream_s"], "frame_wait_s": timing["frame_wait_s"], "init_s": timing["init_s"]})
            fps[run_name] = rec["frames_per_s"]
            if run_name == "ring_flow" and fps["ring_flow"] > 0:
                rec["stream_over_ring"] = round(fps["stream_flow"] / fps["ring_flow"], 2)
            records.append(rec)
            print(json.dumps(rec), flush=True)
        shutil.rmtree(out_dir)
        os.remove(path)
    if a.out:
        with open(a.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
