"""--img / --video throughput of the two engines.

For each stream (a 2M-event 240 x 180 stream and a 1M-event 346 x 260 stream, synth.write_stream_bin) and each output set
(--img; --img --video), runs the product command line through --engine=ring and --engine=stream into the same directory and
reports frames/s and end-to-end Mevents/s (wall clock of the whole process).  The write ceiling is the time to write the
same bytes from memory: the same file count and sizes (frame_N.ppm, frame_N.txt, one AVI of the same size) into the same
directory.  One JSON record per line on stdout (and in --out).

    python scripts/frame_output_bench.py [--work DIR] [--out FILE] [--quick]
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
    files = sorted(os.listdir(out_dir))
    sizes = {f: os.path.getsize(os.path.join(out_dir, f)) for f in files}
    return wall, sizes, (timing[-1] if timing else None)


def write_ceiling(sizes, out_dir):
    """The same files, written from memory: what the disk and the page cache allow."""
    if os.path.exists(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    big = bytes(max(sizes.values()))
    avi = [f for f in sizes if f.endswith(".avi")]
    ppm = sorted((f for f in sizes if f.endswith(".ppm")), key=lambda f: int(f[6:-4]))
    t0 = time.perf_counter()
    va = open(os.path.join(out_dir, avi[0]), "wb") if avi else None
    frame = sizes[avi[0]] // max(1, len(ppm)) if avi else 0
    for f in ppm:
        with open(os.path.join(out_dir, f), "wb") as o:
            o.write(memoryview(big)[:sizes[f]])
        t = f[:-4] + ".txt"
        with open(os.path.join(out_dir, t), "w") as o:
            o.write("x" * sizes.get(t, 0))
        if va:
            va.write(memoryview(big)[:frame])
    if va:
        va.close()
    wall = time.perf_counter() - t0
    shutil.rmtree(out_dir)
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/bf_frame_bench")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a tenth of the events (a smoke run of the script)")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    div = 10 if a.quick else 1
    streams = [("240x180", 240, 180, 100 // div), ("346x260", 346, 260, 50 // div)]
    records = []
    for name, W, H, slices in streams:
        path = os.path.join(a.work, "stream_%s.bin" % name)
        n = synth.write_stream_bin(path, slices, 20000, H, W)
        out_dir = os.path.join(a.work, "out")
        for outs in (["--img"], ["--img", "--video"]):
            ceiling = None
            for engine in ("ring", "stream"):
                args = ["--engine=" + engine, "--res-x=%d" % H, "--res-y=%d" % W, "--quiet", "--img-prefix", out_dir] + outs
                if "--video" in outs:
                    args += ["--video-name", os.path.join(out_dir, "out.avi")]
                if engine == "stream":
                    args.append("--timing")
                wall, sizes, timing = run(args + [path], out_dir, 1800)
                frames = sum(f.endswith(".ppm") for f in sizes)
                if ceiling is None:
                    ceiling = write_ceiling(sizes, out_dir + "_ceiling")
                rec = {"stream": name, "events": n, "outputs": " ".join(outs), "engine": engine, "frames": frames,
                       "bytes": sum(sizes.values()), "wall_s": round(wall, 3), "frames_per_s": round(frames / wall, 2),
                       "mevents_per_s": round(n / wall * 1e-6, 3), "write_ceiling_s": round(ceiling, 3),
                       "ceiling_frames_per_s": round(frames / ceiling, 2), "over_ceiling": round(wall / ceiling, 2)}
                if timing:
                    rec.update({"stream_s": timing["stream_s"], "frame_wait_s": timing["frame_wait_s"], "init_s": timing["init_s"]})
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
