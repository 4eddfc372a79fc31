"""The held flow through the host class (better_flow/optimizer_global.h: hold_field, hold_best, get_flow, flow_field,
write_flow_flo, write_flow_ppm, emit_slice) on libbf_accel.so, against the Python binding on the same cloud: the shear slice on
its 64 x 128 sensor, 32 x 32 cells."""
import os
import re
import subprocess

import numpy as np
import pytest

import flowimg_ref as FI
import global_field_ref as F
import global_flow_ref as R
from better_flow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (64, 128)


@pytest.mark.gpu
def test_optimizer_global_held_flow_host_class(accel_mod, tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_global_flow")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_global_flow.cpp"),
                           "-L" + os.path.join(ROOT, "better_flow_amd"), "-lbf_accel",
                           "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    fr_x, fr_y, t = F.shear_slice()
    path, cloud = str(tmp_path / "ev.txt"), str(tmp_path / "cloud.txt")
    synth.write_txt(path, {"fr_x": fr_x, "fr_y": fr_y, "t": t})
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([exe, path, cloud, str(out_dir)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    c = np.loadtxt(cloud, dtype=np.int64).reshape(-1, 3)
    n = len(c)
    assert n == len(t) == 16000
    assert "no results threw=1" in out
    assert "no hold state errors=3" in out
    assert "state kept=1 best pr same=1" in out
    assert "refused=1 held kept=1" in out
    assert "after set_cells state errors=1" in out
    grid = np.array([[float(a), float(b)] for a, b in re.findall(r"cell \d+ (\S+) (\S+)", out)])
    assert grid.shape == (8, 2)

    def binding(hold):
        """What the binding gives for the same hold: the files' bytes by name."""
        hold()
        flow = acc.global_get_flow()
        owner, U, V = acc.global_flow_field(*RES)
        ppm, _, _ = acc.global_render_flow_frame(*RES, avi=False, flo=False)
        em = accel_mod.Emit(acc, 4 * n + 4, *RES, 2 * n + 2)
        try:
            ticket, rows = em.slice(n, 0, 1000, held=True)
        finally:
            em.close()
        assert ticket == 0 and flow["u"].any() and (owner >= 0).any()
        return {"flow": b"".join(flow[k].tobytes() for k in R.KEYS), "field": owner.tobytes() + U.tobytes() + V.tobytes(),
                "flo": FI.flo_file(owner, U, V), "ppm": b"P6\n%d %d\n255\n" % (3 * RES[1], RES[0]) + ppm.tobytes(),
                "rows": b"".join(rows[k].tobytes() for k in ("t", "row", "col", "u", "v"))}, len(rows["t"])

    acc = accel_mod.Accel(device=0, max_events=n, max_rows=3 * RES[0] + 3, max_cols=3 * RES[1] + 3)
    try:
        acc.upload_events(c[:, 0], c[:, 1], c[:, 2])
        acc.global_set_window(3, 15)
        acc.global_set_cells(*RES, 32, 32)
        opts = acc.global_search_opts(x_low=-0.06, x_hi=0.061, x_step=0.004, y_low=-0.03, y_hi=-0.019, y_step=0.002)
        _, cells, _ = acc.global_search_cells(opts)
        gx, gy = F.fill_cells(F.cells_valid(cells), cells["best_nx"], cells["best_ny"])
        assert np.array_equal(grid[:, 0], gx.reshape(-1)) and np.array_equal(grid[:, 1], gy.reshape(-1))
        holds = {"field": lambda: acc.global_hold_field(gx, gy, mode=R.FIELD), "cells": lambda: acc.global_hold_field(gx, gy, mode=R.CELLS),
                 "best": acc.global_hold_best}
        seen = set()
        for name in ("field", "cells", "best"):
            want, n_rows = binding(holds[name])
            assert "%s events=%d field=%dx%d flo=1 ppm=1 rows=%d" % (name, n, RES[0], RES[1], n_rows) in out
            for ext, data in want.items():
                assert open(str(out_dir / (name + "." + ext)), "rb").read() == data, (name, ext)
            seen.add(want["flow"])
        assert len(seen) == 3                                       # three different flows
    finally:
        acc.close()
