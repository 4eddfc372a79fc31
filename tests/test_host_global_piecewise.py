"""The piecewise projection through the host class (better_flow/optimizer_global.h: project_cells) on libbf_accel.so, against
the Python binding and the numpy restatement (tests/global_piecewise_ref.py) on the two-motion slice."""
import os
import re
import subprocess

import numpy as np
import pytest

import global_cells_ref as GC
import global_piecewise_ref as PW
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_optimizer_global_project_cells_host_class(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global_piecewise")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global_piecewise.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    fr_x, fr_y, t = GC.two_motion_slice()
    path = str(tmp_path / "ev.txt")
    synth.write_txt(path, {"fr_x": fr_x, "fr_y": fr_y, "t": t})
    cloud, imgf, scf = str(tmp_path / "cloud.txt"), str(tmp_path / "img.bin"), str(tmp_path / "scores.bin")
    r = subprocess.run([exe, path, cloud, imgf, scf], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    c = np.loadtxt(cloud, dtype=np.int64).reshape(-1, 3)
    assert len(c) == len(t) == 16000

    assert "no results threw=1" in out
    assert "state kept=1" in out
    assert "refused=6 sums kept=1" in out                      # grids that do not fit the cell grid
    acc = accel_mod.Accel(device=0, max_events=len(c))
    try:
        acc.upload_events(c[:, 0], c[:, 1], c[:, 2])
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        opts = acc.global_search_opts(x_low=-0.045, x_hi=0.056, x_step=0.005, y_low=-0.03, y_hi=0.036, y_step=0.005)
        res, cells, _ = acc.global_search_cells(opts)
        img, sc, S_pw, sums = acc.global_project_cells(cells["best_nx"], cells["best_ny"])
        S_all = acc.global_project_all(res.best_nx, res.best_ny, want_img=False, want_scores=False)[0]
    finally:
        acc.close()
    m = re.search(r"grid (\d+)x(\d+) slice nx=(\S+) ny=(\S+) S=(\d+) S_pw=(\d+) last=(\d+)", out)
    assert (int(m.group(1)), int(m.group(2))) == (2, 4)
    assert (float(m.group(3)), float(m.group(4)), int(m.group(5))) == (res.best_nx, res.best_ny, res.best_sum)
    assert int(m.group(6)) == int(m.group(7)) == S_pw > res.best_sum
    lines = re.findall(r"cell (\d+) (\d+) (\S+) (\S+) (\d+)", out)
    assert len(lines) == 8
    for cx, cy, nx, ny, s in lines:
        cx, cy = int(cx), int(cy)
        assert (float(nx), float(ny), int(s)) == (cells["best_nx"][cx, cy], cells["best_ny"][cx, cy], sums[cx, cy]), (cx, cy)
    assert "img %dx%d scores %d" % (img.shape[0], img.shape[1], sc.size) in out
    assert open(imgf, "rb").read() == img.tobytes() and img.any()
    assert open(scf, "rb").read() == sc.tobytes() and sc.any()
    m = re.search(r"uniform S=(\d+) cells=(\d+) project_all S=(\d+)", out)
    assert int(m.group(1)) == int(m.group(2)) == int(m.group(3)) == S_all == res.best_sum

    ref = GC.GlobalCells(c[:, 0], c[:, 1], c[:, 2], 64, 128, 32, 32, scale=3, metric_wsize=15)
    rimg, rsc, rS, rsums = PW.project_cells(ref, cells["best_nx"], cells["best_ny"])
    assert np.array_equal(img, rimg) and np.array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    assert rS == S_pw and np.array_equal(rsums, sums)
