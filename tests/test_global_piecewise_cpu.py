"""The piecewise projection on the CPU: the numpy restatement (tests/global_piecewise_ref.py) against Global.project_all,
the two-motion slice it is meant for, and the symbol of the built library."""
import ctypes
import os

import numpy as np
import pytest

import global_cells_ref as GC
import global_piecewise_ref as PW
import global_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


@pytest.fixture(scope="module")
def two_motion():
    """The two-motion slice, its per-cell winners over two_motion_subgrid() and the slice's own best candidate."""
    ev = GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    _, cells, best = gc.search_cells(*GC.two_motion_subgrid())
    return gc, cells, best


# golden: the ragged 6 x 8 grid of the cell tests; two-motion: 2 x 4.  The candidates move events by pixels and push some out
@pytest.mark.parametrize("name,grid,cand", [("golden", (90, 120, 16, 16), (0.013, -0.007)),
                                            ("golden", (90, 120, 16, 16), (0.0, 0.0)),
                                            ("two_motion", (64, 128, 32, 32), (0.05, -0.026))])
def test_uniform_grid_is_project_all(name, grid, cand):
    ev = _golden() if name == "golden" else GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15)
    img0, cur0, S0 = G.Global(*ev, scale=3, metric_wsize=15).project_all(*cand)
    img, cur, S, sums = PW.project_cells(gc, np.full(gc.n_cells, cand[0]), np.full(gc.n_cells, cand[1]))
    assert S0 > 0 and img0.any()
    assert np.array_equal(img, img0) and img.dtype == np.uint8
    assert np.array_equal(cur, cur0) and cur.dtype == np.float32
    assert S == S0
    assert np.array_equal(sums.ravel(), GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15).project_all_cells(*cand))
    assert not gc.max_score.any()                                   # the restatement folds no per-event state


def test_sum_rule_and_empty_cells():
    fr_x, fr_y, t = _golden()
    keep = ~((fr_x >= 32) & (fr_x < 48) & (fr_y >= 16) & (fr_y < 32))     # cell (2, 1) of the 16 x 16 grid loses its events
    gc = GC.GlobalCells(fr_x[keep], fr_y[keep], t[keep], 90, 120, 16, 16, scale=3, metric_wsize=15)
    rng = np.random.default_rng(3)
    cx, cy = rng.uniform(-0.02, 0.02, (6, 8)), rng.uniform(-0.02, 0.02, (6, 8))
    cx[2, 1] = cy[2, 1] = np.nan                                          # never read
    img, cur, S, sums = PW.project_cells(gc, cx, cy)
    assert sums.shape == (6, 8) and sums.dtype == np.int64
    assert int(sums.sum()) == S and S > 0
    assert sums[2, 1] == 0 and (sums > 0).sum() > 8                       # (many cells take part in the sum)
    e = GC.GlobalCells([], [], [], 20, 20, 8, 8, scale=3, metric_wsize=5)
    img, cur, S, sums = PW.project_cells(e, np.full(9, np.nan), np.full(9, np.nan))
    assert S == 0 and not sums.any() and not img.any() and img.shape == (5, 5) and cur.shape == (0, 0)


def test_two_motions_are_recovered_piecewise(two_motion):
    """The eight winners of search_cells against the slice's one flow.  Floors: 1.1 for the slice and 1.3 for the right half
    (1.248 and 1.69 with the lattice points nearest the truths); the left half within 2 % of its one-flow value."""
    gc, cells, (bnx, bny, S_one) = two_motion
    img1, _, S1, one = PW.project_cells(gc, np.full(8, bnx), np.full(8, bny))
    assert S1 == S_one
    img, _, S_pw, sums = PW.project_cells(gc, cells["best_nx"], cells["best_ny"])
    acc1 = int(PW.accepted_per_cell(gc, np.full(8, bnx), np.full(8, bny)).sum())
    acc = int(PW.accepted_per_cell(gc, cells["best_nx"], cells["best_ny"]).sum())
    (l1, r1), (l, r) = PW.half_totals(one), PW.half_totals(sums)
    print("one flow (%.4f, %.4f): S = %d, %d events accepted" % (bnx, bny, S_one, acc1))
    print("piecewise: S_pw = %d (%.4f x), %d events accepted" % (S_pw, S_pw / S_one, acc))
    print("right half %.4f x, left half %.4f x" % (r / r1, l / l1))
    assert S_pw > S_one and S_pw >= 1.1 * S_one
    assert r >= 1.3 * r1
    assert abs(l / l1 - 1.0) <= 0.02
    assert not np.array_equal(img, img1)


def test_mutations_are_seen(two_motion):
    gc, cells, (bnx, bny, S_one) = two_motion
    cx, cy = cells["best_nx"], cells["best_ny"]
    _, _, S_pw, sums = PW.project_cells(gc, cx, cy)
    # the halves' candidates swapped: every event under the other motion's flow
    _, _, S_sw, _ = PW.project_cells(gc, np.roll(cx, 2, axis=1), np.roll(cy, 2, axis=1))
    print("swapped halves: %.4f x the one-flow S" % (S_sw / S_one))
    assert S_sw < S_one < S_pw
    # one cell's candidate changed: that cell's sum changes
    mx = cx.copy()
    mx[1, 2] += 0.02
    _, _, S_m, sums_m = PW.project_cells(gc, mx, cy)
    assert sums_m[1, 2] != sums[1, 2] and S_m != S_pw


def test_library_exports_the_piecewise_projection():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert hasattr(lib, "bf_global_project_cells")
    assert "bf_global_project_cells" in accel.EXPORTS
    lib.bf_global_project_cells.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    # no context: an argument error, not a crash
    assert lib.bf_global_project_cells(None, None, None, 0, 127.0, None, None, None, None, 0) == accel.BF_ERR_ARG
    assert callable(accel.Accel.global_project_cells)
