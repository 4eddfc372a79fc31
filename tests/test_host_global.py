"""OptimizerGlobal through the host class (better_flow/optimizer_global.h) on libbf_accel.so, against the numpy
restatement (tests/global_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import global_ref as G
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_optimizer_global_host_class(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    sl = synth.make_slice(8000, 180, 240, 0.05, seed=9)
    path = str(tmp_path / "ev.txt")
    synth.write_txt(path, sl)
    cloud = str(tmp_path / "cloud.txt")
    r = subprocess.run([exe, path, cloud], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    c = np.loadtxt(cloud, dtype=np.int64).reshape(-1, 3)
    ev = (c[:, 0], c[:, 1], c[:, 2])
    assert len(c) == len(sl["t"])

    ref = G.Global(*ev, scale=5, metric_wsize=21)
    img, _, s0 = ref.project_all(0.0, 0.0)
    w = np.arange(img.size) % 251 + 1
    m = re.search(r"default S0=(\d+) img=(\d+)x(\d+) checksum=(\d+)", out)
    assert m and int(m.group(1)) == s0 and (int(m.group(2)), int(m.group(3))) == img.shape
    assert int(m.group(4)) == int((img.ravel().astype(np.int64) * w).sum())
    xs, ys = G.sweep_values(-0.01, 0.0105, 0.001), G.sweep_values(-0.005, 0.0055, 0.001)
    surf, (bnx, bny, bs) = ref.search(xs, ys)
    m = re.search(r"default best nx=(\S+) ny=(\S+) S=(\d+) grid=(\d+)x(\d+)", out)
    assert (float(m.group(1)), float(m.group(2)), int(m.group(3))) == (bnx, bny, bs)
    assert (int(m.group(4)), int(m.group(5))) == (21, 11)
    u, v = ref.best_uv()
    lines = re.findall(r"default event (\d+) (\S+) (\S+) (\S+) (\S+) (\S+)", out)
    assert len(lines) == (len(c) + 96) // 97
    for k, ms, px, py, eu, evv in lines:
        k = int(k)
        assert (float(ms), float(px), float(py), float(eu), float(evv)) == \
            (ref.max_score[k], ref.best_pr_x[k], ref.best_pr_y[k], u[k], v[k]), k

    ga, gb = G.Global(*ev, scale=3, metric_wsize=5), G.Global(*ev, scale=7, metric_wsize=35)
    a1, b1 = ga.project_all(0.01, 0.0)[2], gb.project_all(-0.02, 0.01)[2]
    img_a, _, a2 = ga.project_all(-0.005, 0.002)
    m = re.search(r"pair a1=(\d+) b1=(\d+) a2=(\d+) img=(\d+)x(\d+) max_score_sum=(\S+)", out)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (a1, b1, a2)
    assert (int(m.group(4)), int(m.group(5))) == img_a.shape
    tot = 0.0
    for v in ga.max_score:
        tot += float(v)
    assert float(m.group(6)) == tot

    s3 = G.Global(*ev, scale=3).project_all(0.02, -0.01)[2]
    assert int(re.search(r"scale3 S=(\d+)", out).group(1)) == s3
    _, cur, s7 = G.Global(*ev, scale=7, metric_wsize=9).project_all(-0.03, 0.02, 127.0)
    m = re.search(r"scale7 S=(\d+) scores_sum=(\S+)", out)
    assert int(m.group(1)) == s7
    tot = 0.0
    for f in cur.ravel():
        tot += float(f)
    assert float(m.group(2)) == tot
