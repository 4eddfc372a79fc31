"""The host classes with wide groups (bf::Refit::wide, held by bf::MotionAssigner, bf::ObjectMerger and bf::ObjectFinder and
given to bf::ObjectTasks::wide) and bf_motion_compensator --objects-wide, on the GPU.

tests/cpp/test_groups_wide.cpp linked against the product library runs MotionAssigner::alternate from the scene's two true models,
ObjectFinder::find, and the three slices of tests/track_scene.py through ObjectTracker::next, each two ways -- wide = true
with helper = nullptr, and wide = false with a helper context -- and compares ids, models, counts and records as bytes.
The command line writes objects_N.txt and objects_N.tracks.txt byte for byte as without the flag."""
import os
import subprocess

import numpy as np
import pytest

import groups_ref as gr
import segment_scene as scene
import track_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "better_flow_amd", "host")
H, W = track_scene.H, track_scene.W


@pytest.fixture(scope="module")
def slices():
    return track_scene.make()[0]


def test_host_classes_leave_the_helper_paths_bytes(accel_mod, slices, tmp_path):
    exe = str(tmp_path / "test_groups_wide")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_groups_wide.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    files = []
    for n, sl in enumerate(slices):
        files.append(str(tmp_path / ("events_%d.txt" % n)))
        with open(files[-1], "w") as f:
            for x, y, t in zip(sl["fr_x"], sl["fr_y"], sl["t"]):
                f.write("%d %d %d\n" % (x, y, t))
    models = str(tmp_path / "models.bin")
    with open(models, "wb") as f:   # the two true models: the patch's, the background's
        for vel in (scene.V_PATCH, scene.V_BACKGROUND):
            m = gr.warm_from_flow(*scene.flow_of(vel))
            f.write(bytes(accel_mod.Model(**{k: getattr(m, k) for k, _ in gr.oracle.Model._fields_})))
    prefix = str(tmp_path / "w_")
    r = subprocess.run([exe, prefix, models, "2", str(track_scene.STEP_NS), str(H), str(W)] + files, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    out = r.stdout.decode()
    print(out)
    print(open(prefix + "times.txt").read())   # (figures, not bars)
    assert r.returncode == 0, (out, r.stderr.decode()[-3000:])
    lines = out.splitlines()
    assert [ln.split()[:2] for ln in lines] == [["alternate", "same"], ["find", "same"], ["track", "same"]]
    assert all(int(ln.split()[2].lstrip("(")) > 1000 for ln in lines)   # (ids of ~15k events each: something was compared)


@pytest.mark.parametrize("track", [False, True])
def test_cli_objects_wide_keeps_every_files_bytes(slices, tmp_path, track):
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

    base = ["--objects-track"] if track else []
    plain, wide = run("plain", base), run("wide", base + ["--objects-wide"])
    names = sorted(os.listdir(str(plain)))
    assert len(names) >= (6 if track else 3) and sorted(os.listdir(str(wide))) == names
    assert any(n.endswith(".tracks.txt") for n in names) == track
    for n in names:
        assert open(str(wide / n), "rb").read() == open(str(plain / n), "rb").read(), n
    if not track:
        r = subprocess.run([exe, "--objects-wide", txt], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and b"--objects-wide" in r.stderr   # it requires --objects
