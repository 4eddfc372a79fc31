"""The interpolated cell flow field on the CPU: the numpy restatement (tests/global_field_ref.py) against a direct rational
evaluation of its weights, against Global.project_all and the piecewise projection where the three must agree, the fill, the
shear slice the smooth field is meant for, the two-motion slice it must not hurt, and the symbol of the built library."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import global_cells_ref as GC
import global_field_ref as F
import global_piecewise_ref as PW
import global_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


# 24 pixels: 3 cells of 8; 5 cells of 5 (odd: a centre pixel has w == 0; the last cell ragged); 24 of 1; 4 of 7 (ragged)
@pytest.mark.parametrize("size", [8, 5, 1, 7])
def test_weights_against_rational_position(size):
    res = 24
    n_cell = -(-res // size)
    x = np.arange(res)
    a0, a1, w = F.axis(x, size, n_cell)
    assert ((0 <= a0) & (a0 < n_cell) & (0 <= a1) & (a1 < n_cell)).all()
    assert ((0 <= w) & (w < 2 * size)).all()
    centre = [Fraction(2 * a + 1, 2) * size - Fraction(1, 2) for a in range(n_cell)]
    for xi in range(res):
        pos = min(max(Fraction(xi), centre[0]), centre[-1])          # clamped: constant beyond the outermost centres
        lo = max(a for a in range(n_cell) if centre[a] <= pos)
        frac = (pos - centre[lo]) / size                              # (centres are `size` apart)
        assert frac < 1
        assert (int(a0[xi]), Fraction(int(w[xi]), 2 * size)) == (lo, frac), xi
        assert int(a1[xi]) == min(lo + 1, n_cell - 1)
        if xi <= centre[0] or xi >= centre[-1]:
            assert w[xi] == 0                                         # both clamps
    if size % 2 == 1:
        assert (w[size // 2::size] == 0).all() and (a0[size // 2::size] == np.arange(len(x[size // 2::size]))).all()
    if size == 1:
        assert not w.any() and np.array_equal(a0, x)


# golden: the ragged 6 x 8 grid of the cell tests; two-motion: 2 x 4.  The candidates move events by pixels and push some out
@pytest.mark.parametrize("name,grid,cand", [("golden", (90, 120, 16, 16), (0.013, -0.007)),
                                            ("golden", (90, 120, 16, 16), (0.0, 0.0)),
                                            ("two_motion", (64, 128, 32, 32), (0.05, -0.026))])
def test_uniform_grid_is_project_all(name, grid, cand):
    ev = _golden() if name == "golden" else GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15)
    cx, cy = np.full(gc.n_cells, cand[0]), np.full(gc.n_cells, cand[1])
    nx_e, ny_e = F.field_at_events(gc, grid[2], grid[3], cx, cy)
    assert (nx_e == cand[0]).all() and (ny_e == cand[1]).all()      # exactly
    img0, cur0, S0 = G.Global(*ev, scale=3, metric_wsize=15).project_all(*cand)
    img, cur, S, sums, _, _ = F.project_field(gc, grid[2], grid[3], cx, cy)
    assert S0 > 0 and img0.any()
    assert np.array_equal(img, img0) and img.dtype == np.uint8
    assert np.array_equal(cur.view(np.uint32), cur0.view(np.uint32)) and cur.dtype == np.float32
    assert S == S0
    assert np.array_equal(sums.ravel(), GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15).project_all_cells(*cand))
    assert not gc.max_score.any()                                   # the restatement folds no per-event state


def _crop12():
    fr_x, fr_y, t = GC.tie_slice(False)
    keep = (fr_x < 12) & (fr_y < 12)
    return fr_x[keep], fr_y[keep], t[keep]


def test_per_pixel_cells_are_the_piecewise_projection():
    ev = _crop12()
    gc = GC.GlobalCells(*ev, 12, 12, 1, 1, scale=3, metric_wsize=15)
    rng = np.random.default_rng(5)
    cx, cy = rng.uniform(-0.2, 0.2, (12, 12)), rng.uniform(-0.2, 0.2, (12, 12))
    assert not F.axis(np.arange(12), 1, 12)[2].any()
    got = F.project_field(gc, 1, 1, cx, cy)
    want = PW.project_cells(gc, cx, cy)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2] == want[2] > 0 and np.array_equal(got[3], want[3])
    assert np.array_equal(got[4], cx[gc.fr_x, gc.fr_y]) and np.array_equal(got[5], cy[gc.fr_x, gc.fr_y])


def test_one_cell_is_project_all():
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, 24, 24, 24, 24, scale=3, metric_wsize=15)
    assert gc.n_cells == 1
    img0, cur0, S0 = G.Global(*ev, scale=3, metric_wsize=15).project_all(0.03, -0.02)
    img, cur, S, sums, nx_e, ny_e = F.project_field(gc, 24, 24, [0.03], [-0.02])
    assert np.array_equal(img, img0) and np.array_equal(cur.view(np.uint32), cur0.view(np.uint32)) and S == S0 > 0
    assert sums.shape == (1, 1) and (nx_e == 0.03).all() and (ny_e == -0.02).all()


def test_an_event_at_a_cell_centre_gets_its_cells_value():
    rng = np.random.default_rng(2)
    cx, cy = rng.uniform(-0.1, 0.1, (5, 5)), rng.uniform(-0.1, 0.1, (5, 5))
    c = np.arange(5) * 5 + 2                                         # the centre pixels of the 5-pixel cells
    X, Y = np.meshgrid(c, c, indexing="ij")
    nx, ny = F.field_at(X.ravel(), Y.ravel(), 5, 5, 5, 5, cx, cy)
    assert np.array_equal(nx, cx.ravel()) and np.array_equal(ny, cy.ravel())


def test_fill():
    rng = np.random.default_rng(9)
    cx, cy = rng.uniform(-1, 1, (3, 4)), rng.uniform(-1, 1, (3, 4))
    bx, by = np.where(F.FILL_MASK, cx, np.nan), np.where(F.FILL_MASK, cy, np.nan)       # invalid entries are not read
    fx, fy = F.fill_cells(F.FILL_MASK, bx, by)
    assert np.array_equal(fx, cx.ravel()[F.FILL_FROM]) and np.array_equal(fy, cy.ravel()[F.FILL_FROM])
    zx, zy = F.fill_cells(np.zeros((3, 4), dtype=bool), bx, by)
    assert not zx.any() and not zy.any() and zx.shape == (3, 4)
    ax, ay = F.fill_cells(np.ones((3, 4), dtype=bool), cx, cy)
    assert np.array_equal(ax, cx) and np.array_equal(ay, cy)
    for a in range(3):
        for b in range(4):                                           # a NaN anywhere in the grid is refused
            bad = cx.copy()
            bad[a, b] = np.nan
            with pytest.raises(AssertionError):
                F.field_at(np.array([0]), np.array([0]), 8, 8, 3, 4, bad, cy)
            with pytest.raises(AssertionError):
                F.field_at(np.array([0]), np.array([0]), 8, 8, 3, 4, cx, bad)


@pytest.fixture(scope="module")
def shear():
    """The shear slice on 32 x 32 cells, its per-cell winners over shear_subgrid() and the slice's own best candidate."""
    xs, ys = F.shear_subgrid()
    assert (len(xs), len(ys)) == (59, 5)
    ev, cells, best = F.shear_winners()
    assert len(ev[2]) == 16000
    return GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15), cells, best


def test_shear_is_recovered_better_by_the_smooth_field(shear):
    """Measured with this restatement (32 x 32 cells, scale 3, window 15, the eight winners of search_cells over 59 x 5
    candidates): S_pw = 1.1430 x the one-flow S, S_f = 1.2043 x it, S_f / S_pw = 1.0536; per cell S_f(cell) / S_pw(cell)
    between 1.0202 and 1.0888; the grid mirrored left <-> right gives 0.7880 x S_pw.  The floor is half the measured gain: the
    figure belongs to one synthetic slice, and the assertion is there to catch a broken interpolation."""
    gc, cells, (bnx, bny, S_one) = shear
    assert F.cells_valid(cells).all()
    cx, cy = cells["best_nx"], cells["best_ny"]
    _, _, S1, _ = PW.project_cells(gc, np.full(8, bnx), np.full(8, bny))
    assert S1 == S_one
    _, _, S_pw, pw = PW.project_cells(gc, cx, cy)
    _, _, S_f, fs, nx_e, _ = F.project_field(gc, 32, 32, cx, cy)
    _, _, S_m, _, _, _ = F.project_field(gc, 32, 32, cx[:, ::-1], cy[:, ::-1])
    ratio = fs / pw
    print("one flow (%.4f, %.4f): S = %d" % (bnx, bny, S_one))
    print("piecewise %.4f x, field %.4f x, field / piecewise %.4f" % (S_pw / S_one, S_f / S_one, S_f / S_pw))
    print("per cell field / piecewise: %.4f .. %.4f; mirrored grid %.4f x S_pw" % (ratio.min(), ratio.max(), S_m / S_pw))
    assert S_f > S_pw > S_one
    assert (fs >= pw).all()
    assert S_f >= (1 + F.SHEAR_GAIN / 2) * S_pw
    assert S_m < S_pw
    assert len(np.unique(nx_e)) > 8                                  # a field, not eight steps


def test_two_motions_lose_nothing():
    """The discontinuous flow the piecewise projection is for, with the eight winners of two_motion_subgrid(): measured
    S_f / S_pw = 1.0031 with this restatement; the floor is 0.98."""
    ev = GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    _, cells, _ = gc.search_cells(*GC.two_motion_subgrid())
    assert F.cells_valid(cells).all()
    _, _, S_pw, _ = PW.project_cells(gc, cells["best_nx"], cells["best_ny"])
    _, _, S_f, _, _, _ = F.project_field(gc, 32, 32, cells["best_nx"], cells["best_ny"])
    print("two motions: field / piecewise %.4f" % (S_f / S_pw))
    assert S_f >= 0.98 * S_pw


def test_library_exports_the_field_projection():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert hasattr(lib, "bf_global_project_field")
    assert "bf_global_project_field" in accel.EXPORTS
    lib.bf_global_project_field.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # no context: an argument error, not a crash
    assert lib.bf_global_project_field(None, None, None, 0, 127.0, None, None, None, None, 0, None, None, None,
                                       None) == accel.BF_ERR_ARG
    assert callable(accel.Accel.global_project_field)
