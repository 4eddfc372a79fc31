"""The per-cell search through the host class (better_flow/optimizer_global.h: set_cells, compute_flow_cells,
write_cell_flo) on libbf_accel.so, against the numpy restatement (tests/global_cells_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import global_cells_ref as GC
import global_ref as G
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_optimizer_global_cells_host_class(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global_cells")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global_cells.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    sl = synth.make_slice(4000, 90, 120, 0.05, seed=9)
    path = str(tmp_path / "ev.txt")
    synth.write_txt(path, sl)
    cloud, flo = str(tmp_path / "cloud.txt"), str(tmp_path / "cells.flo")
    r = subprocess.run([exe, path, cloud, flo], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    c = np.loadtxt(cloud, dtype=np.int64).reshape(-1, 3)
    assert len(c) == len(sl["t"])

    assert "no cells threw=1" in out
    ref = GC.GlobalCells(c[:, 0], c[:, 1], c[:, 2], 128, 120, 32, 32, scale=3, metric_wsize=15)
    xs, ys = G.sweep_values(-0.003, 0.0035, 0.001), G.sweep_values(-0.002, 0.0025, 0.001)
    _, cells, (bnx, bny, bs) = ref.search_cells(xs, ys)
    m = re.search(r"grid (\d+)x(\d+) slice nx=(\S+) ny=(\S+) S=(\d+) sweep=(\d+)x(\d+)", out)
    assert (int(m.group(1)), int(m.group(2))) == (4, 4) == (ref.n_cell_x, ref.n_cell_y)
    assert (float(m.group(3)), float(m.group(4)), int(m.group(5))) == (bnx, bny, bs)
    assert (int(m.group(6)), int(m.group(7))) == (len(xs), len(ys)) == (7, 5)
    lines = re.findall(r"cell (\d+) (\d+) (\S+) (\S+) (\S+) (\S+) (\d+) (\d+) (\d+)", out)
    assert len(lines) == 16
    for cx, cy, nx, ny, u, v, s, k, n in lines:
        cx, cy = int(cx), int(cy)
        got = (float(nx), float(ny), float(u), float(v), int(s), int(k), int(n))
        assert got == tuple(cells[f][cx, cy] for f in GC.CELL_FIELDS), (cx, cy)
    assert not cells["events"][3].any() and cells["events"][:3].all()      # the last row of cells is empty, no other

    assert "flo written=1" in out
    raw = open(flo, "rb").read()
    assert np.frombuffer(raw[:4], "<f4")[0] == np.float32(202021.25)
    assert tuple(np.frombuffer(raw[4:12], "<i4")) == (4, 4)                # width = n_cell_y, height = n_cell_x
    pay = np.frombuffer(raw[12:], "<f4").reshape(4, 4, 2)
    has = cells["events"] > 0
    want_h = np.where(has, cells["best_v"].astype(np.float32), np.float32(1e9))     # horizontal = v (columns)
    want_v = np.where(has, cells["best_u"].astype(np.float32), np.float32(1e9))     # vertical = u (rows)
    assert np.array_equal(pay[..., 0], want_h) and np.array_equal(pay[..., 1], want_v)

    u, v = ref.best_uv()
    ev_lines = re.findall(r"event (\d+) (\S+) (\S+) (\S+) (\S+) (\S+)", out)
    assert len(ev_lines) == (len(c) + 96) // 97
    for k, ms, px, py, eu, evv in ev_lines:
        k = int(k)
        assert (float(ms), float(px), float(py), float(eu), float(evv)) == \
            (ref.max_score[k], ref.best_pr_x[k], ref.best_pr_y[k], u[k], v[k]), k
