"""The piecewise projection on the GPU (bf_global_project_cells): bit for bit against the numpy restatement
(tests/global_piecewise_ref.py) and, with one candidate in every cell, against bf_global_project_all on the device itself.
Every value is an integer or one IEEE operation: no tolerances."""
import ctypes as C
import os

import numpy as np
import pytest

import global_cells_ref as GC
import global_piecewise_ref as PW
import global_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y", "best_u", "best_v")


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


def _accel(accel_mod, ev):
    acc = accel_mod.Accel(device=0, max_events=max(len(ev[2]), 1))
    acc.upload_events(*ev)
    return acc


def _opts(accel_mod, xlo=-0.002, xhi=0.0025, ylo=-0.003, yhi=0.0035, step=0.001):
    return accel_mod.Accel.global_search_opts(x_low=xlo, x_hi=xhi, x_step=step, y_low=ylo, y_hi=yhi, y_step=step)


def _same_state(a, b):
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), k


def _same(got, want):
    """(img, scores, S_pw, cell_sums) of the device against the restatement's"""
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float32 and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2] == want[2]
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    assert int(got[3].sum()) == got[2]


# t in [2e7, 3e7): (0.2, -0.15) moves an event by 3 to 5 pixels, so some leave the 24 x 24 image; (3.0, -2.0) removes all
UNIFORM = [(0.0, 0.0), (0.2, -0.15), (-0.03, 0.11), (3.0, -2.0)]


@pytest.mark.parametrize("scale,mw", [(1, 3), (3, 15), (5, 21), (7, 35)])
def test_uniform_grid_equals_project_all(accel_mod, scale, mw):
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=scale, metric_wsize=mw)
    assert gc.events[4] == 0 and (np.delete(gc.events, 4) > 0).all()
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(scale, mw)
        g = acc.global_set_cells(*GC.TIE_GRID)
        assert (g.n_cell_x, g.n_cell_y) == (3, 3)
        fresh = acc.global_get_events()
        for nx, ny in UNIFORM:
            cx, cy = np.full((3, 3), nx), np.full((3, 3), ny)
            cx[1, 1] = cy[1, 1] = np.nan                       # the empty middle cell: never read
            got = acc.global_project_cells(cx, cy)
            _same(got, PW.project_cells(gc, cx, cy))
            _same_state(acc.global_get_events(), fresh)        # nothing folded
            assert (got[2] == 0) == ((nx, ny) == UNIFORM[-1])
        for nx, ny in UNIFORM:                                 # ... and the device's own project_all
            cx, cy = np.full(9, nx), np.full(9, ny)
            img, cur, S_pw, sums = acc.global_project_cells(cx, cy)
            S, img0, cur0 = acc.global_project_all(nx, ny)
            assert np.array_equal(img, img0) and np.array_equal(cur.view(np.uint32), cur0.view(np.uint32)) and S_pw == S
    finally:
        acc.close()


def test_two_motion_slice(accel_mod):
    """32 x 32 cells of about 2 000 events: runs of 256, eight work-groups adding into one cell's word.  The cells' own
    winners of the default sweep; floors as in tests/test_global_piecewise_cpu.py."""
    ev = GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    assert gc.events.min() >= 1000
    small = _opts(accel_mod)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        r, cells, _ = acc.global_search_cells()
        before = acc.global_get_events()
        cx, cy = cells["best_nx"], cells["best_ny"]
        got = acc.global_project_cells(cx, cy)
        _same(got, PW.project_cells(gc, cx, cy))
        again = acc.global_project_cells(cx, cy)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
        one = acc.global_project_cells(np.full(8, r.best_nx), np.full(8, r.best_ny))
        _same_state(acc.global_get_events(), before)
        r2, cells2, surf2 = acc.global_search_cells(small, want_surface=True)
        after = acc.global_get_events()
        # the same calls without the piecewise projections in between
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        acc.global_search_cells()
        _same_state(acc.global_get_events(), before)
        r3, cells3, surf3 = acc.global_search_cells(small, want_surface=True)
        _same_state(acc.global_get_events(), after)
    finally:
        acc.close()
    assert np.array_equal(cells2, cells3) and np.array_equal(surf2, surf3)
    assert (r2.best_nx, r2.best_ny, r2.best_sum) == (r3.best_nx, r3.best_ny, r3.best_sum)
    S_one, S_pw = one[2], got[2]
    assert S_one == r.best_sum
    (l1, r1), (l, rr) = PW.half_totals(one[3]), PW.half_totals(got[3])
    print("S_pw / S = %.4f, right half %.4f x, left half %.4f x" % (S_pw / S_one, rr / r1, l / l1))
    assert S_pw > S_one and S_pw >= 1.1 * S_one
    assert rr >= 1.3 * r1
    assert abs(l / l1 - 1.0) <= 0.02


def test_pyramid_and_seeded_search_after_it(accel_mod):
    """The cells' running bests and the scratch of the pyramid are as the call found them: a pyramid search, then a seeded
    one on the same window (it continues from the cells' bests and the per-event state), give the same bits with the
    piecewise projections in between as without them."""
    ev = _golden()
    o = _opts(accel_mod, -0.006, 0.0065, -0.004, 0.0045)

    def sequence(acc, piecewise):
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        r1, cells1, ev1, _, _ = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1)
        seeds = np.where(cells1["events"] > 0, cells1["best_index"], -1)
        if piecewise:
            acc.global_project_cells(cells1["best_nx"], cells1["best_ny"])
            acc.global_project_cells(cells1["best_ny"], cells1["best_nx"], want_img=False, want_scores=False)
        r2, cells2, ev2, surf2, info2 = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1, seeds=seeds,
                                                                       want_surface=True)
        if piecewise:
            acc.global_project_cells(cells2["best_nx"], cells2["best_ny"])
        r3, cells3, ev3, surf3, _ = acc.global_search_cells_pyramid(o, levels=3, factor=2, radius=1, want_surface=True)
        return ((r1.best_nx, r1.best_ny, r1.best_sum), cells1, ev1, (r2.best_nx, r2.best_ny, r2.best_sum), cells2, ev2, surf2,
                list(info2.level_count), (r3.best_nx, r3.best_ny, r3.best_sum), cells3, ev3, surf3, acc.global_get_events())

    acc = _accel(accel_mod, ev)
    try:
        a = sequence(acc, True)
        b = sequence(acc, False)
    finally:
        acc.close()
    assert len(a[5]) > 0 and a[4]["best_sum"].any()
    for x, y in zip(a[:-1], b[:-1]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    _same_state(a[-1], b[-1])


def _tie_plus_corner():
    """tie_slice plus 150 events in the corner cell (0, 0): 450 events over 8 occupied cells (runs of 64), one of them split"""
    fr_x, fr_y, t = GC.tie_slice(False)
    rng = np.random.default_rng(23)
    ax, ay, at = rng.integers(0, 8, 150), rng.integers(0, 8, 150), rng.integers(20000000, 30000000, 150)
    fr_x, fr_y, t = np.concatenate([fr_x, ax]), np.concatenate([fr_y, ay]), np.concatenate([t, at])
    o = np.argsort(t, kind="stable")
    return fr_x[o].astype(np.int64), fr_y[o].astype(np.int64), t[o].astype(np.int64)


def _ragged():
    """the slice and grid of tests/test_global_cells_cpu.py::test_ragged_grid: 3 000 events, 4 x 4 cells of 20 x 30 on 67 x 101"""
    rng = np.random.default_rng(7)
    n = 3000
    fr_x, fr_y = rng.integers(0, 67, n), rng.integers(0, 101, n)
    fr_x[:2], fr_y[:2] = (66, 0), (100, 0)
    t = np.sort(rng.integers(0, 30000000, n))
    return fr_x.astype(np.int64), fr_y.astype(np.int64), t.astype(np.int64)


def _crop12():
    fr_x, fr_y, t = GC.tie_slice(False)
    keep = (fr_x < 12) & (fr_y < 12)
    return fr_x[keep], fr_y[keep], t[keep]


# name: (events, sensor and cells, scale, window, run length the grid must choose, events of the largest cell at least)
SHAPES = {"split64": (_tie_plus_corner, GC.TIE_GRID, 3, 15, 64, 65),
          "ragged": (_ragged, (67, 101, 20, 30), 3, 5, 64, 65),
          "one_cell": (_ragged, (67, 101, 67, 101), 3, 5, 256, 3000),
          "per_pixel": (_crop12, (12, 12, 1, 1), 3, 15, 64, 1)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_run_shapes(accel_mod, name):
    make, grid, scale, mw, run_len, biggest = SHAPES[name]
    ev = make()
    gc = GC.GlobalCells(*ev, *grid, scale=scale, metric_wsize=mw)
    occupied = int((gc.events > 0).sum())
    assert (256 if len(ev[0]) >= 256 * occupied else 64) == run_len and gc.events.max() >= biggest   # (bf_global_set_cells' rule)
    rng = np.random.default_rng(5)
    shape = (gc.n_cell_x, gc.n_cell_y)
    cx, cy = rng.uniform(-0.2, 0.2, shape), rng.uniform(-0.2, 0.2, shape)      # a different flow in every cell
    cx[gc.events.reshape(shape) == 0] = np.nan
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(scale, mw)
        acc.global_set_cells(*grid)
        got = acc.global_project_cells(cx, cy)
        want = PW.project_cells(gc, cx, cy)
        _same(got, want)
        assert got[2] > 0
        img, sc, S, none = acc.global_project_cells(cx, cy, want_img=False, want_scores=False, want_cell_sums=False)
        assert img is None and sc is None and none is None and S == want[2]
    finally:
        acc.close()


def test_mixed_candidates_reject_per_cell(accel_mod):
    """A different candidate in every cell; those of the TIE_ZERO range carry every event of their cell out of the image
    (by 78 pixels or more), the others keep theirs: the acceptance test bites cell by cell."""
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=3, metric_wsize=15)
    zx, zy = G.sweep_values(GC.TIE_ZERO[0], GC.TIE_ZERO[1], 0.001), G.sweep_values(GC.TIE_ZERO[2], GC.TIE_ZERO[3], 0.001)
    cx = np.array([[0.01, zx[1], -0.02], [zx[3], np.nan, 0.0], [0.015, 0.03, zx[6]]])
    cy = np.array([[-0.01, zy[0], 0.02], [zy[2], np.nan, 0.005], [0.0, -0.025, zy[4]]])
    far = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=bool)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(*GC.TIE_GRID)
        got = acc.global_project_cells(cx, cy)
        _same(got, PW.project_cells(gc, cx, cy))
        accepted = PW.accepted_per_cell(gc, cx, cy)
        assert not accepted[far].any() and not got[3][far].any()
        near = ~far & (gc.events.reshape(3, 3) > 0)
        assert (accepted[near] > 0).all() and (got[3][near] > 0).all()
    finally:
        acc.close()


def test_two_calls_give_identical_bytes(accel_mod):
    ev = _golden()
    rng = np.random.default_rng(11)
    cx, cy = rng.uniform(-0.05, 0.05, (6, 8)), rng.uniform(-0.05, 0.05, (6, 8))
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        a = acc.global_project_cells(cx, cy)
        b = acc.global_project_cells(cx, cy)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] > 0
        assert a[3].tobytes() == b[3].tobytes()
        _same(a, PW.project_cells(GC.GlobalCells(*ev, 90, 120, 16, 16, scale=3, metric_wsize=15), cx, cy))
    finally:
        acc.close()


def test_refusals_and_edge_cases(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_STATE, BfError

    def raises(code, call):
        with pytest.raises(BfError) as e:
            call()
        assert e.value.code == code

    ev = GC.tie_slice(False)
    zeros = np.zeros((3, 3))
    acc = _accel(accel_mod, ev)
    try:
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, zeros))                  # no window
        acc.global_set_window(3, 15)
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, zeros))                  # no cells
        acc.global_set_cells(*GC.TIE_GRID)
        acc.global_search_cells(_opts(accel_mod))                                           # (a state that is not the fresh one)
        before = acc.global_get_events()
        assert before["max_score"].any()
        good = acc.global_project_cells(zeros, zeros)
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(np.zeros(8), np.zeros(8)))      # short grids
        short, S = np.full(8, -1, dtype=np.int64), C.c_int64(-1)                            # short sums: the C-ABI itself
        assert acc.L.bf_global_project_cells(acc.h, zeros.ctypes.data, zeros.ctypes.data, 9, 127.0, None, None, C.byref(S),
                                             short.ctypes.data, 8) == BF_ERR_ARG
        assert S.value == -1 and (short == -1).all()
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, zeros, nz=0.0))
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, zeros, nz=-127.0))
        for bad in (np.inf, -np.inf, np.nan, 1e39, -1e39):                                  # (1e39: infinite as a float)
            cx = zeros.copy()
            cx[2, 0] = bad                                                                  # an occupied cell
            raises(BF_ERR_ARG, lambda: acc.global_project_cells(cx, zeros))
            raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, cx))
        cx = zeros.copy()
        cx[1, 1] = np.inf                                                                   # the empty cell: not read
        assert all(np.array_equal(a, b) for a, b in zip(acc.global_project_cells(cx, cx), good))
        _same_state(acc.global_get_events(), before)
        assert all(np.array_equal(a, b) for a, b in zip(acc.global_project_cells(zeros, zeros), good))
        acc.upload_events(*ev)                                                              # an upload in between
        raises(BF_ERR_STATE, lambda: acc.global_project_cells(zeros, zeros))
        acc.global_set_window(3, 15)                                                        # the window clears the cells
        raises(BF_ERR_ARG, lambda: acc.global_project_cells(zeros, zeros))
        acc.global_set_cells(*GC.TIE_GRID)
        assert all(np.array_equal(a, b) for a, b in zip(acc.global_project_cells(zeros, zeros), good))
    finally:
        acc.close()


def test_empty_cloud(accel_mod):
    acc = accel_mod.Accel(device=0, max_events=16)
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        acc.global_set_window(3, 5)
        g = acc.global_set_cells(20, 30, 8, 8)
        assert (g.n_cell_x, g.n_cell_y) == (3, 4)
        img, sc, S, sums = acc.global_project_cells(np.full((3, 4), np.nan), np.full((3, 4), np.nan))
        assert S == 0 and sums.shape == (3, 4) and not sums.any()
        assert img.shape == (5, 5) and not img.any() and sc.shape == (0, 0)
    finally:
        acc.close()
