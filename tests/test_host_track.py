"""bf::ObjectTracker (host/better_flow/object_tracker.h) and bf_motion_compensator --objects-track.

CPU: match() from the stand-alone program tests/cpp/test_track_match.cpp, built with -fsanitize=address,undefined and run
directly, held to the Python restatement (tests/track_ref.py) on the cases of tests/test_track_cpu.py and on seeded tables.
GPU: tests/cpp/test_object_tracker.cpp linked against the product library runs the three slices of tests/track_scene.py through
next(); the command line runs them as one event file."""
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr
import track_scene
from test_track_cpu import MATCH_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "better_flow_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
H, W = track_scene.H, track_scene.W


# ---- CPU: match() ----

def test_match_on_the_host_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "test_track_match")
    subprocess.check_call(["g++", "-O1", "-std=c++14"] + SAN + ["-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                                                                os.path.join(ROOT, "tests", "cpp", "test_track_match.cpp"), "-o", exe])
    cases = [(np.array(t, dtype=np.int64), None if i is None else np.array(i), num, den) for _, t, i, num, den, _ in MATCH_CASES]
    rng = np.random.default_rng(17)
    for _ in range(40):   # seeded tables with many ties (small values), K and Kp from 1 .. 6 and 0 .. 6
        K, Kp = int(rng.integers(1, 7)), int(rng.integers(0, 7))
        cases.append((rng.integers(0, 4, (K, Kp + 1)) * int(rng.integers(1, 30)), None, int(rng.integers(0, 4)), int(rng.integers(1, 5))))
    cases.append((np.full((64, 65), 2 ** 31 - 1, dtype=np.int64), np.full(64, 2 ** 31 - 1), 1, 1))   # the largest table, the largest counts
    text, want = [], []
    for table, inside, num, den in cases:
        inside = np.minimum(table.sum(axis=1), 2 ** 31 - 1) if inside is None else inside
        text.append("%d %d %d %d %s %s" % (table.shape[0], table.shape[1] - 1, num, den, " ".join(map(str, table.ravel())),
                                           " ".join(map(str, inside))))
        want.append(tr.match(table, inside, num, den))
    r = subprocess.run([exe], input="\n".join(text).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = [[int(v) for v in ln.split()] for ln in r.stdout.decode().splitlines()]
    assert got == want
    assert [w for (_, _, _, _, _, w) in MATCH_CASES] == want[:len(MATCH_CASES)]


# ---- GPU: the tracker over the three slices ----

@pytest.fixture(scope="module")
def slices():
    return track_scene.make()[0]


def write_events(path, sl):
    with open(path, "w") as f:
        for x, y, t in zip(sl["fr_x"], sl["fr_y"], sl["t"]):
            f.write("%d %d %d\n" % (x, y, t))


def read_slice(A, prefix, n):
    i32 = lambda name: np.fromfile(prefix + name, dtype=np.int32)
    raw = open(prefix + "%d_models.bin" % n, "rb").read()
    K = len(raw) // 88
    lines = [ln.split() for ln in open(prefix + "%d.txt" % n).read().splitlines()]
    head = dict(zip(lines[0][::2], (int(v) for v in lines[0][1::2])))
    return dict(gid=i32("%d_gid.i32" % n), counts=i32("%d_counts.i32" % n), overlap=i32("%d_overlap.i32" % n), inside=i32("%d_inside.i32" % n),
                models=list((A.Model * K).from_buffer_copy(raw)) if K else [], raw_models=raw, head=head,
                groups=[[int(v) for v in ln] for ln in lines[1:-1]], ended=[int(v) for v in lines[-1][1:]])


@pytest.mark.gpu
def test_object_tracker_over_three_slices(accel_mod, slices, tmp_path):
    A = accel_mod
    exe = str(tmp_path / "test_object_tracker")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_object_tracker.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    files = []
    for n, sl in enumerate(slices):
        files.append(str(tmp_path / ("events_%d.txt" % n)))
        write_events(files[-1], sl)
    acc = A.Accel(device=0, max_events=max(len(s["t"]) for s in slices), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        for every in (0, 1):
            prefix = str(tmp_path / ("r%d_" % every))
            r = subprocess.run([exe, prefix, "2", str(every), str(track_scene.STEP_NS), str(H), str(W)] + files, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=120)
            assert r.returncode == 0, r.stderr.decode()[-3000:]
            out = [read_slice(A, prefix, n) for n in range(3)]
            print(open(prefix + "times.txt").read())   # (a figure, not a bar: the first call of a process also loads the kernels)
            for n, o in enumerate(out):
                print("research_every %d, slice %d: %s groups %s ended %s" % (every, n, o["head"], o["groups"], o["ended"]))
            # which path a slice took, and slice 0 is the finder's own result
            assert [o["head"]["searched"] for o in out] == ([1, 0, 0] if every == 0 else [1, 1, 1])
            assert [o["head"]["dt_ns"] for o in out] == [0, track_scene.STEP_NS, track_scene.STEP_NS]
            assert out[0]["gid"].tobytes() == np.fromfile(prefix + "find_gid.i32", dtype=np.int32).tobytes()
            assert out[0]["raw_models"] == open(prefix + "find_models.bin", "rb").read()
            assert out[0]["counts"].tobytes() == np.fromfile(prefix + "find_counts.i32", dtype=np.int32).tobytes()
            # patch and background keep one track id each
            owner = []
            for sl, o in zip(slices, out):
                assert len(o["groups"]) == 2 and o["ended"] == []
                patch_group = int(np.bincount(o["gid"][sl["is_patch"] & (o["gid"] >= 0)], minlength=2).argmax())
                track_of = {g[0]: g[1] for g in o["groups"]}
                owner.append((track_of[1 - patch_group], track_of[patch_group]))
            assert owner == [owner[0]] * 3 and sorted(owner[0]) == [0, 1], owner
            assert [[g[2] for g in o["groups"]] for o in out] == [[0, 0], [1, 1], [2, 2]]   # the ages
            # every table equals the binding's for the same ids and models
            for n in (1, 2):
                p, o = out[n - 1], out[n]
                acc.upload_events(slices[n - 1]["fr_x"], slices[n - 1]["fr_y"], slices[n - 1]["t"])
                acc.set_groups(p["gid"], 2)
                acc.track_keep(p["models"], 3, (H, W), want_plane=False)
                acc.upload_events(slices[n]["fr_x"], slices[n]["fr_y"], slices[n]["t"])
                acc.set_groups(o["gid"], 2)
                table, inside, _ = acc.track_overlap(o["models"], track_scene.STEP_NS, 3, (H, W))
                assert o["head"]["kept"] == 2 and o["overlap"].tobytes() == table.tobytes() and o["inside"].tobytes() == inside.tobytes()
                want = tr.match(table, inside)
                assert [g[4] for g in o["groups"]] == [int(table[k, want[k]]) for k in range(2)]
            assert out[0]["overlap"].size == 0 and out[0]["head"]["kept"] == 0
    finally:
        acc.close()


# ---- GPU: the command line ----

@pytest.mark.gpu
def test_cli_objects_track_on_the_three_slices(slices, tmp_path):
    """bf_motion_compensator --objects=2 --objects-track on the three slices as one text file: every tracks.txt carries the same
    two ids.  Without the flag only objects_N.txt appear, and slice 0's has the same bytes with the flag (the searched path is
    the finder's own)."""
    from better_flow_amd import synth
    exe = os.path.join(HOST, "bf_motion_compensator")
    whole = dict(fr_x=np.concatenate([s["fr_x"] for s in slices]), fr_y=np.concatenate([s["fr_y"] for s in slices]),
                 t=np.concatenate([s["t"] + s["t0_ns"] for s in slices]))
    txt = str(tmp_path / "scene.txt")
    synth.write_txt(txt, whole)

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([exe, "--objects=2"] + extra + ["--refresh-time=0.03", "--refresh-event-count=10000000", "--res-x=%d" % H,
                                                          "--res-y=%d" % W, "--quiet", "--img-prefix", str(out), txt],
                           cwd=str(out), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return out

    plain, tracked = run("plain", []), run("tracked", ["--objects-track"])
    names = sorted(os.listdir(str(plain)))
    n = len(names)
    assert n >= 3 and names == sorted("objects_%d.txt" % i for i in range(n))
    assert sorted(os.listdir(str(tracked))) == sorted(names + ["objects_%d.tracks.txt" % i for i in range(n)])
    assert open(str(tracked / "objects_0.txt"), "rb").read() == open(str(plain / "objects_0.txt"), "rb").read()
    origin = None
    for i in range(n):
        lines = [ln.split() for ln in open(str(tracked / ("objects_%d.tracks.txt" % i))).read().splitlines()]
        print(i, lines)
        assert lines[0][0] == "searched" and lines[0][2] == "dt_ns" and lines[-1] == ["ended"]
        # (the ring spans 0.2 s and the file 0.09 s: no event leaves it, every slice starts at the file's first event and holds
        # the slices before it, so the time origins do not move and dt is 0 -- overlapping slices, refresh < span)
        assert int(lines[0][1]) == (1 if i == 0 else 0) and int(lines[0][3]) == 0
        groups = [[int(v) for v in ln] for ln in lines[1:-1]]
        assert sorted(g[1] for g in groups) == [0, 1] and all(g[2] == i for g in groups)
        table = [ln.split() for ln in open(str(tracked / ("objects_%d.txt" % i))).read().splitlines()]
        assert [g[3] for g in groups] == [int(t[1]) for t in table[:2]]
        # the track of the group with the patch's flow (rows per second > 0) stays the same
        patch = [g[1] for g, t in zip(groups, table) if float(t[2]) > 100.0]
        assert len(patch) == 1
        origin = patch[0] if origin is None else origin
        assert patch[0] == origin
    r = subprocess.run([exe, "--objects-track", txt], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and b"--objects-track" in r.stderr   # it requires --objects
