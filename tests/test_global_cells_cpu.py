"""The per-cell objective of the exhaustive search on the CPU: the numpy restatement (tests/global_cells_ref.py) against
Global.search, the two-motion slice it is meant for, and the ABI and symbols of the built library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import global_cells_ref as GC
import global_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


XS, YS = G.sweep_values(-0.002, 0.0025, 0.001), G.sweep_values(-0.003, 0.0035, 0.001)   # 5 x 7


@pytest.fixture(scope="module")
def golden_search():
    ev = _golden()
    ref = G.Global(*ev, scale=3, metric_wsize=15)
    surf, best = ref.search(XS, YS)
    return ev, ref, surf, best


def _same_state(a, b):
    for k in ("max_score", "best_nx", "best_ny", "best_nz", "best_pr_x", "best_pr_y"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_sum_over_cells_is_the_slice_surface(golden_search):
    ev, ref, surf, best = golden_search
    assert (len(XS), len(YS)) == (5, 7)
    gc = GC.GlobalCells(*ev, 90, 120, 16, 16, scale=3, metric_wsize=15)
    assert (gc.n_cell_x, gc.n_cell_y) == (6, 8)         # ragged: 90 = 5 * 16 + 10, 120 = 7 * 16 + 8
    csurf, cells, sbest = gc.search_cells(XS, YS)
    assert csurf.shape == (6, 8, 5, 7)
    assert np.array_equal(csurf.sum(axis=(0, 1)), surf)
    assert sbest == best
    assert cells["events"].sum() == len(ev[0])
    _same_state(gc, ref)
    # each cell's answer is its own first maximum
    flat = csurf.reshape(48, 35)
    assert np.array_equal(cells["best_index"].ravel(), flat.argmax(axis=1))
    assert np.array_equal(cells["best_sum"].ravel(), flat.max(axis=1))
    assert len(set(cells["best_index"].ravel().tolist())) > 1     # (the cells do not all agree: the test can tell them apart)


def test_one_cell_is_the_slice(golden_search):
    ev, ref, surf, (bnx, bny, bs) = golden_search
    gc = GC.GlobalCells(*ev, 90, 120, 90, 120, scale=3, metric_wsize=15)
    assert gc.n_cells == 1
    csurf, cells, sbest = gc.search_cells(XS, YS)
    assert np.array_equal(csurf[0, 0], surf)
    assert (cells["best_nx"][0, 0], cells["best_ny"][0, 0], cells["best_sum"][0, 0]) == (bnx, bny, bs) == sbest
    assert cells["events"][0, 0] == len(ev[0])
    assert (cells["best_u"][0, 0], cells["best_v"][0, 0]) == G.compute_uv(bnx, bny)


def test_two_motions_are_recovered_per_cell():
    """Every one of the eight 32 x 32 cells within 2 grid steps (1.575 px/s) of its half's motion, in both components: the
    winner is a grid point and the truth lies between grid points.  The slice-level best sees the left half only."""
    ev = GC.two_motion_slice()
    assert len(ev[0]) == 16000 and ev[0].max() < 64 and ev[1].max() < 128
    xs, ys = GC.two_motion_subgrid()
    assert (len(xs), len(ys)) == (39, 28)
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    assert (gc.n_cell_x, gc.n_cell_y) == (2, 4)
    _, cells, (bnx, bny, _) = gc.search_cells(xs, ys)
    assert cells["events"].min() >= 1000
    tol = 2 * GC.GRID_STEP
    assert abs(tol - 1.575) < 1e-3
    for cx in range(2):
        for cy in range(4):
            tu, tv = GC.TWO_MOTION_TRUTH["left" if cy < 2 else "right"]
            u, v = cells["best_u"][cx, cy], cells["best_v"][cx, cy]
            print("cell %d: (%.2f, %.2f) px/s, truth (%g, %g)" % (cx * 4 + cy, u, v, tu, tv))
            assert abs(u - tu) <= tol and abs(v - tv) <= tol, (cx, cy, u, v)
    su, sv = G.compute_uv(bnx, bny)
    assert abs(su - 40.0) <= tol and abs(sv + 20.0) <= tol      # one flow for the slice: the right half is invisible


def test_ragged_grid():
    rng = np.random.default_rng(7)
    n = 3000
    fr_x, fr_y = rng.integers(0, 67, n), rng.integers(0, 101, n)
    fr_x[:2], fr_y[:2] = (66, 0), (100, 0)                       # the last pixel of the sensor, and the first
    t = np.sort(rng.integers(0, 30000000, n))
    gc = GC.GlobalCells(fr_x, fr_y, t, 67, 101, 20, 30, scale=3, metric_wsize=5)
    assert (gc.n_cell_x, gc.n_cell_y) == (4, 4)                  # 67 = 3 * 20 + 7, 101 = 3 * 30 + 11
    assert gc.cell[0] == 15 and gc.cell[1] == 0
    want = np.zeros(16, dtype=np.int64)
    for x, y in zip(fr_x, fr_y):
        want[(x // 20) * 4 + y // 30] += 1
    assert np.array_equal(gc.events, want)
    xs, ys = [-0.001, 0.0, 0.001], [0.0, 0.002]
    csurf, cells, sbest = gc.search_cells(xs, ys)
    ref = G.Global(fr_x, fr_y, t, 3, 5)
    surf, best = ref.search(xs, ys)
    assert np.array_equal(csurf.sum(axis=(0, 1)), surf) and sbest == best
    _same_state(gc, ref)


def test_empty_cell_reports_candidate_zero():
    fr_x, fr_y, t = _golden()
    keep = ~((fr_x >= 32) & (fr_x < 48) & (fr_y >= 16) & (fr_y < 32))     # cell (2, 1) of the 16 x 16 grid loses its events
    ev = (fr_x[keep], fr_y[keep], t[keep])
    gc = GC.GlobalCells(*ev, 90, 120, 16, 16, scale=3, metric_wsize=15)
    csurf, cells, _ = gc.search_cells(XS, YS)
    assert cells["events"][2, 1] == 0 and cells["events"].sum() == keep.sum()
    assert not csurf[2, 1].any()
    assert (cells["best_index"][2, 1], cells["best_sum"][2, 1]) == (0, 0)
    assert (cells["best_nx"][2, 1], cells["best_ny"][2, 1]) == (XS[0], YS[0])
    # an empty cloud: every cell is empty
    e = GC.GlobalCells([], [], [], 20, 20, 8, 8, scale=3, metric_wsize=5)
    csurf, cells, sbest = e.search_cells(XS, YS)
    assert not csurf.any() and not cells["events"].any() and not cells["best_index"].any()
    assert sbest == (XS[0], YS[0], 0)


# ---- ABI ----

_PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "bf_accel.h"
#define F(S, M) printf(#S " " #M " %zu\n", offsetof(S, M))
int main(void) {
    printf("bf_global_cells size %zu\n", sizeof(bf_global_cells));
    printf("bf_global_cell_result size %zu\n", sizeof(bf_global_cell_result));
    F(bf_global_cells, n_cell_x); F(bf_global_cells, n_cell_y);
    F(bf_global_cell_result, best_nx); F(bf_global_cell_result, best_ny); F(bf_global_cell_result, best_u);
    F(bf_global_cell_result, best_v); F(bf_global_cell_result, best_sum); F(bf_global_cell_result, best_index);
    F(bf_global_cell_result, events);
    return 0;
}
'''


def test_struct_mirrors_match_the_header(tmp_path):
    from better_flow_amd import accel
    src = tmp_path / "probe.cpp"
    src.write_text(_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        s, m, v = line.split()
        got[(s, m)] = int(v)
    for cname, mirror in (("bf_global_cells", accel.GlobalCells), ("bf_global_cell_result", accel.GlobalCellResult)):
        assert got[(cname, "size")] == ctypes.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
        assert len(mirror._fields_) == sum(1 for (s, m) in got if s == cname and m != "size")
    assert tuple(np.dtype(accel.GlobalCellResult).names) == GC.CELL_FIELDS
    assert np.dtype(accel.GlobalCellResult).itemsize == got[("bf_global_cell_result", "size")]


def test_library_exports_the_cell_search():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    for name in ("bf_global_set_cells", "bf_global_search_cells"):
        assert hasattr(lib, name), name
        assert name in accel.EXPORTS
    # no context: an argument error, not a crash
    assert lib.bf_global_set_cells(None, 64, 64, 8, 8, None) == accel.BF_ERR_ARG
    assert lib.bf_global_search_cells(None, None, None, None, ctypes.c_int64(0), None, ctypes.c_int64(0)) == accel.BF_ERR_ARG
    assert callable(accel.Accel.global_set_cells) and callable(accel.Accel.global_search_cells)
