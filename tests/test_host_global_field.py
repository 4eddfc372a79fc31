"""The interpolated field through the host class (better_flow/optimizer_global.h: project_field, get_event_field,
write_field_flo) on libbf_accel.so, against the Python binding and the numpy restatement (tests/global_field_ref.py) on the
shear slice.  The cell grid is laid over a 96 x 160 sensor, so that its last row and column of cells have no event and the
fill has work to do."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import global_cells_ref as GC
import global_field_ref as F
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (96, 160, 32, 32)


@pytest.mark.gpu
def test_optimizer_global_project_field_host_class(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global_field")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global_field.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    fr_x, fr_y, t = F.shear_slice()
    path = str(tmp_path / "ev.txt")
    synth.write_txt(path, {"fr_x": fr_x, "fr_y": fr_y, "t": t})
    cloud, imgf, scf, evf, flo = [str(tmp_path / n) for n in ("cloud.txt", "img.bin", "scores.bin", "events.bin", "field.flo")]
    r = subprocess.run([exe, path, cloud, imgf, scf, evf, flo], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    c = np.loadtxt(cloud, dtype=np.int64).reshape(-1, 3)
    n = len(c)
    assert n == len(t) == 16000

    assert "no results threw=1" in out
    assert "state kept=1" in out
    assert "flo written=1" in out
    assert "refused=7 results kept=1" in out                   # grids that do not fit the cell grid, and a NaN in an empty cell
    acc = accel_mod.Accel(device=0, max_events=n)
    try:
        acc.upload_events(c[:, 0], c[:, 1], c[:, 2])
        acc.global_set_window(3, 15)
        acc.global_set_cells(*GRID)
        opts = acc.global_search_opts(x_low=-0.06, x_hi=0.061, x_step=0.004, y_low=-0.03, y_hi=-0.019, y_step=0.002)
        res, cells, _ = acc.global_search_cells(opts)
        valid = F.cells_valid(cells)
        assert valid[:2, :4].all() and not valid[2, :].any() and not valid[:, 4].any()
        gx, gy = F.fill_cells(valid, cells["best_nx"], cells["best_ny"])
        img, sc, S_f, sums, ev = acc.global_project_field(gx, gy, want_events=True)
        S_m = acc.global_project_field(np.ascontiguousarray(gx[:, ::-1]), np.ascontiguousarray(gy[:, ::-1]), want_img=False,
                                       want_scores=False)[2]
        S_all = acc.global_project_all(res.best_nx, res.best_ny, want_img=False, want_scores=False)[0]
    finally:
        acc.close()
    m = re.search(r"grid (\d+)x(\d+) S_f=(\d+) last=(\d+)", out)
    assert (int(m.group(1)), int(m.group(2))) == (3, 5)
    assert int(m.group(3)) == int(m.group(4)) == S_f > res.best_sum
    lines = re.findall(r"cell (\d+) (\d+) (\S+) (\S+) (\S+) (\S+) (\d+) (\d+)", out)
    assert len(lines) == 15
    for cx, cy, nx, ny, fx, fy, events, s in lines:
        cx, cy = int(cx), int(cy)
        assert (float(nx), float(ny)) == (cells["best_nx"][cx, cy], cells["best_ny"][cx, cy]), (cx, cy)
        assert (float(fx), float(fy), int(events), int(s)) == (gx[cx, cy], gy[cx, cy], cells["events"][cx, cy], sums[cx, cy]), (cx, cy)
    assert "img %dx%d scores %d events %d" % (img.shape[0], img.shape[1], sc.size, n) in out
    assert open(imgf, "rb").read() == img.tobytes() and img.any()
    assert open(scf, "rb").read() == sc.tobytes() and sc.any()
    assert open(evf, "rb").read() == b"".join(ev[k].tobytes() for k in ("nx", "ny", "u", "v"))
    m = re.search(r"mirrored S=(\d+) cells=(\d+)", out)
    assert int(m.group(1)) == int(m.group(2)) == S_m < S_f
    m = re.search(r"uniform S=(\d+) cells=(\d+) project_all S=(\d+) best S=(\d+) events uniform=1", out)
    assert int(m.group(1)) == int(m.group(2)) == int(m.group(3)) == int(m.group(4)) == S_all == res.best_sum

    # the restatement: the projection, the per-event field, and the .flo at every sensor pixel
    ref = GC.GlobalCells(c[:, 0], c[:, 1], c[:, 2], *GRID, scale=3, metric_wsize=15)
    rimg, rsc, rS, rsums, rnx, rny = F.project_field(ref, 32, 32, gx, gy)
    assert np.array_equal(img, rimg) and np.array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    assert rS == S_f and np.array_equal(rsums, sums)
    ru, rv = F.event_uv(rnx, rny)
    for got, want in ((ev["nx"], rnx), (ev["ny"], rny), (ev["u"], ru), (ev["v"], rv)):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    X, Y = np.meshgrid(np.arange(GRID[0]), np.arange(GRID[1]), indexing="ij")
    pu, pv = F.event_uv(*F.field_at(X.ravel(), Y.ravel(), 32, 32, 3, 5, gx, gy))
    payload = np.stack([pv.astype(np.float32), pu.astype(np.float32)], axis=1)      # horizontal = v, vertical = u
    want = struct.pack("<fii", 202021.25, GRID[1], GRID[0]) + payload.astype("<f4").tobytes()
    assert open(flo, "rb").read() == want
