"""The coarse-to-fine and seeded per-cell search through the host class (better_flow/optimizer_global.h:
compute_flow_cells_pyramid, compute_flow_cells_seeded, get_seeds / set_seeds, write_cell_flo) on libbf_accel.so, over two
slices, against the numpy restatement (tests/global_pyramid_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import global_cells_ref as GC
import global_pyramid_ref as P
import global_ref as G
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(out, tag):
    m = re.search(tag + r" grid (\d+)x(\d+) slice nx=(\S+) ny=(\S+) S=(\d+) lattice=(\d+)x(\d+) evaluated=(\d+) levels=(\d+) counts((?: \d+)*)", out)
    head = dict(grid=(int(m.group(1)), int(m.group(2))), slice=(float(m.group(3)), float(m.group(4)), int(m.group(5))),
                lattice=(int(m.group(6)), int(m.group(7))), evaluated=int(m.group(8)), levels=int(m.group(9)),
                counts=[int(v) for v in m.group(10).split()])
    cells = {}
    for cx, cy, nx, ny, u, v, s, k, n in re.findall(tag + r" cell (\d+) (\d+) (\S+) (\S+) (\S+) (\S+) (\d+) (\d+) (\d+)", out):
        cells[(int(cx), int(cy))] = (float(nx), float(ny), float(u), float(v), int(s), int(k), int(n))
    return head, cells


def _same(head, cells, want, levels):
    assert head["grid"] == (4, 3) and head["lattice"] == (23, 13) and head["levels"] == levels
    assert head["counts"] == want["level_count"] and head["evaluated"] == len(want["evaluated"])
    assert head["slice"] == want["slice"]
    assert len(cells) == 12
    for (cx, cy), got in cells.items():
        assert got == tuple(want["cells"][f][cx, cy] for f in GC.CELL_FIELDS), (cx, cy)


@pytest.mark.gpu
def test_optimizer_global_seeded_over_two_slices(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global_pyramid")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global_pyramid.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    paths = []
    for seed in (4, 7):                                       # the same motion, other events
        sl = synth.make_slice(3000, 40, 48, 0.05, seed=seed, velocity=(30.0, -20.0))
        paths.append(str(tmp_path / ("ev%d.txt" % seed)))
        synth.write_txt(paths[-1], sl)
    clouds, flo = [str(tmp_path / "cloud_a.txt"), str(tmp_path / "cloud_b.txt")], str(tmp_path / "cells.flo")
    r = subprocess.run([exe] + paths + clouds + [flo], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    ca, cb = (np.loadtxt(p, dtype=np.int64).reshape(-1, 3) for p in clouds)
    xs, ys = G.sweep_values(0.036, 0.0585, 0.001), G.sweep_values(-0.0375, -0.0250, 0.001)

    ra = GC.GlobalCells(ca[:, 0], ca[:, 1], ca[:, 2], 64, 48, 16, 16, scale=3, metric_wsize=15)
    wa = P.search_pyramid(ra, xs, ys, 3, 2, 2)
    _same(*_parse(out, "first"), wa, 3)
    seeds = np.where(wa["cells"]["events"] > 0, wa["cells"]["best_index"], -1)
    assert (seeds >= 0).any() and (seeds < 0).any()
    rb = GC.GlobalCells(cb[:, 0], cb[:, 1], cb[:, 2], 64, 48, 16, 16, scale=3, metric_wsize=15)
    wb = P.search_pyramid(rb, xs, ys, 1, 2, 2, seeds=seeds)
    head, cells = _parse(out, "second")
    _same(head, cells, wb, 1)
    assert head["evaluated"] < len(wa["evaluated"])

    assert "flo written=1" in out and "cleared seeds=0" in out
    raw = open(flo, "rb").read()
    assert np.frombuffer(raw[:4], "<f4")[0] == np.float32(202021.25)
    assert tuple(np.frombuffer(raw[4:12], "<i4")) == (3, 4)                # width = n_cell_y, height = n_cell_x
    pay = np.frombuffer(raw[12:], "<f4").reshape(4, 3, 2)
    has = wb["cells"]["events"] > 0
    assert np.array_equal(pay[..., 0], np.where(has, wb["cells"]["best_v"].astype(np.float32), np.float32(1e9)))
    assert np.array_equal(pay[..., 1], np.where(has, wb["cells"]["best_u"].astype(np.float32), np.float32(1e9)))

    u, v = P.best_uv(rb)
    ev_lines = re.findall(r"event (\d+) (\S+) (\S+) (\S+) (\S+) (\S+)", out)
    assert len(ev_lines) == (len(cb) + 96) // 97
    for k, ms, px, py, eu, evv in ev_lines:
        k = int(k)
        assert (float(ms), float(px), float(py), float(eu), float(evv)) == \
            (rb.max_score[k], rb.best_pr_x[k], rb.best_pr_y[k], u[k], v[k]), k
