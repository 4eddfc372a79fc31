"""The per-cell objective of the exhaustive search on the GPU (bf_global_set_cells / bf_global_search_cells): bit for bit
against the numpy restatement (tests/global_cells_ref.py) and against bf_global_search.  Every value is an integer or one
IEEE operation: no tolerances."""
import os

import numpy as np
import pytest

import global_cells_ref as GC
import global_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS, YS = G.sweep_values(-0.002, 0.0025, 0.001), G.sweep_values(-0.003, 0.0035, 0.001)   # 5 x 7: batches of 32 and 3
STATE_KEYS = ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y")


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


def _accel(accel_mod, ev):
    acc = accel_mod.Accel(device=0, max_events=max(len(ev[2]), 1))
    acc.upload_events(*ev)
    return acc


def _opts(accel_mod, xlo=-0.002, xhi=0.0025, ylo=-0.003, yhi=0.0035, step=0.001):
    return accel_mod.Accel.global_search_opts(x_low=xlo, x_hi=xhi, x_step=step, y_low=ylo, y_hi=yhi, y_step=step)


def _check(acc, r, cells, surf, ref, rsurf, rcells, rbest):
    """cell results, surface, slice result and the full per-event state against the restatement"""
    assert (r.n_x, r.n_y) == rsurf.shape[2:]
    assert cells.shape == rsurf.shape[:2]
    assert np.array_equal(surf, rsurf)
    for k in GC.CELL_FIELDS:
        assert np.array_equal(cells[k], rcells[k]), k
    assert (r.best_nx, r.best_ny, r.best_sum) == rbest
    got = acc.global_get_events()
    for k in STATE_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), k
    u, v = ref.best_uv()
    assert np.array_equal(got["best_u"], u) and np.array_equal(got["best_v"], v)


# 16 x 16: ragged against 90 x 120, runs of 64; 90 x 120: one cell, 24 work-groups of 256 adding into one word;
# 1 x 120: one cell per sensor row; 1 x 1: a cell per pixel, most of them empty or with one event
GRIDS = [(16, 16), (90, 120), (1, 120), (1, 1)]


@pytest.mark.parametrize("scale,mw", [(3, 15), (1, 5)])
def test_golden_bit_identical(accel_mod, scale, mw):
    ev = _golden()
    assert len(ev[0]) % 256 != 0
    acc = _accel(accel_mod, ev)
    try:
        for rows, cols in GRIDS:
            ref = GC.GlobalCells(*ev, 90, 120, rows, cols, scale=scale, metric_wsize=mw)
            rsurf, rcells, rbest = ref.search_cells(XS, YS)
            acc.global_set_window(scale, mw)
            g = acc.global_set_cells(90, 120, rows, cols)
            assert (g.n_cell_x, g.n_cell_y) == (ref.n_cell_x, ref.n_cell_y), (rows, cols)
            r, cells, surf = acc.global_search_cells(_opts(accel_mod), want_surface=True)
            _check(acc, r, cells, surf, ref, rsurf, rcells, rbest)
            if (rows, cols) == (1, 1):
                assert (cells["events"] == 0).sum() > 5000 and (cells["events"] == 1).sum() > 500
            # without a surface buffer: the same answers from the batch block alone
            acc.global_set_window(scale, mw)
            acc.global_set_cells(90, 120, rows, cols)
            r2, cells2, none = acc.global_search_cells(_opts(accel_mod))
            assert none is None and np.array_equal(cells2, cells)
            assert (r2.best_nx, r2.best_ny, r2.best_sum) == (r.best_nx, r.best_ny, r.best_sum)
    finally:
        acc.close()


def _crowded(n_a, n_b, n_rest, seed):
    """n_a events inside the 8 x 8 cell at (8, 8), n_b inside the one at (24, 16), n_rest anywhere on a 40 x 40 sensor"""
    rng = np.random.default_rng(seed)
    fr_x = np.concatenate([rng.integers(8, 16, n_a), rng.integers(24, 32, n_b), rng.integers(0, 40, n_rest)])
    fr_y = np.concatenate([rng.integers(8, 16, n_a), rng.integers(16, 24, n_b), rng.integers(0, 40, n_rest)])
    fr_x[-2:], fr_y[-2:] = (0, 39), (0, 39)                 # the bounding box is the sensor
    o = rng.permutation(len(fr_x))
    t = np.sort(rng.integers(0, 30000000, len(fr_x)))
    return fr_x[o].astype(np.int64), fr_y[o].astype(np.int64), t.astype(np.int64)


# 700 + 300 scattered: runs of 64, eleven work-groups add into one cell's words;
# 700 + 600 + 2: two crowded cells, runs of 256, three work-groups each (the last one partly filled)
@pytest.mark.parametrize("n_a,n_b,n_rest", [(700, 0, 300), (700, 600, 2)])
def test_one_cell_split_over_several_work_groups(accel_mod, n_a, n_b, n_rest):
    ev = _crowded(n_a, n_b, n_rest, seed=n_rest)
    assert len(ev[0]) % 256 != 0
    ref = GC.GlobalCells(*ev, 40, 40, 8, 8, scale=3, metric_wsize=15)
    assert ref.events[1 * 5 + 1] >= n_a
    rsurf, rcells, rbest = ref.search_cells(XS, YS)
    assert rsurf[1, 1].any()
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(40, 40, 8, 8)
        r, cells, surf = acc.global_search_cells(_opts(accel_mod), want_surface=True)
        _check(acc, r, cells, surf, ref, rsurf, rcells, rbest)
    finally:
        acc.close()


@pytest.mark.parametrize("equal", [True, False])
def test_ties_keep_the_lowest_candidate(accel_mod, equal):
    """GC.tie_slice: S(k, cell) equal and non-zero for all 35 k of two batches, and all zero.  Every cell, the empty one
    included, and the slice answer candidate 0; the events are counted either way."""
    ev = GC.tie_slice(equal)
    lat = GC.TIE_EQUAL if equal else GC.TIE_ZERO
    xs, ys = G.sweep_values(lat[0], lat[1], 0.001), G.sweep_values(lat[2], lat[3], 0.001)
    assert (len(xs), len(ys)) == (7, 5)
    ref = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=3, metric_wsize=15)
    rsurf, rcells, rbest = ref.search_cells(xs, ys)
    assert (rsurf == rsurf[:, :, :1, :1]).all() and rsurf[:, :, 0, 0].astype(bool).sum() == (8 if equal else 0)
    assert ref.events[4] == 0 and (np.delete(ref.events, 4) > 0).all() and not rcells["best_index"].any()
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        g = acc.global_set_cells(*GC.TIE_GRID)
        assert (g.n_cell_x, g.n_cell_y) == (3, 3)
        r, cells, surf = acc.global_search_cells(_opts(accel_mod, lat[0], lat[1], lat[2], lat[3]), want_surface=True)
        _check(acc, r, cells, surf, ref, rsurf, rcells, rbest)
        assert not cells["best_index"].any() and (r.best_nx, r.best_ny) == (xs[0], ys[0])
    finally:
        acc.close()


def test_equivalence_with_global_search(accel_mod):
    ev = _golden()
    step = 2.0 ** -9                                  # exact in binary: the half grids hold the union's values
    whole = _opts(accel_mod, -0.0078125, 0.0078125, -0.00390625, 0.00390625, step)      # 8 x 4
    lo = _opts(accel_mod, -0.0078125, 0.0, -0.00390625, 0.00390625, step)
    hi = _opts(accel_mod, 0.0, 0.0078125, -0.00390625, 0.00390625, step)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        r0, s0 = acc.global_search(whole)
        st0 = acc.global_get_events()
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        r1, cells, s1 = acc.global_search_cells(whole, want_surface=True)
        st1 = acc.global_get_events()
        assert np.array_equal(s1.sum(axis=(0, 1)), s0)
        assert (r1.best_nx, r1.best_ny, r1.best_sum, r1.n_x, r1.n_y) == (r0.best_nx, r0.best_ny, r0.best_sum, r0.n_x, r0.n_y)
        for k in st0:
            assert np.array_equal(st1[k], st0[k]), k
        assert st0["max_score"].max() > 0
        # two half ranges in sequence leave the state of the union; the cells stay set across searches
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        _, ca, sa = acc.global_search_cells(lo, want_surface=True)
        _, cb, sb = acc.global_search_cells(hi, want_surface=True)
        st2 = acc.global_get_events()
        assert np.array_equal(np.concatenate([sa, sb], axis=2), s1)
        for k in st0:
            assert np.array_equal(st2[k], st0[k]), k
        # ... and mixing the two entry points does too
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        acc.global_search(lo)
        acc.global_search_cells(hi)
        st3 = acc.global_get_events()
        for k in st0:
            assert np.array_equal(st3[k], st0[k]), k
    finally:
        acc.close()


def test_two_motions_default_sweep(accel_mod):
    """The slice of two motions, full default sweep (14 400 candidates): every 32 x 32 cell within 2 grid steps
    (1.575 px/s: the winner is a grid point, the truth lies between grid points) of its half's motion in both components;
    the slice's best equals bf_global_search's."""
    ev = GC.two_motion_slice()
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        r, cells, _ = acc.global_search_cells()
        st = acc.global_get_events()
        acc.global_set_window(3, 15)
        r0, _ = acc.global_search(want_surface=False)
        st0 = acc.global_get_events()
    finally:
        acc.close()
    assert cells.shape == (2, 4) and (r.n_x, r.n_y) == (180, 80)
    tol = 2 * GC.GRID_STEP
    for cx in range(2):
        for cy in range(4):
            tu, tv = GC.TWO_MOTION_TRUTH["left" if cy < 2 else "right"]
            u, v = cells["best_u"][cx, cy], cells["best_v"][cx, cy]
            print("cell %d: (%.2f, %.2f) px/s, truth (%g, %g), %d events" % (cx * 4 + cy, u, v, tu, tv, cells["events"][cx, cy]))
            assert abs(u - tu) <= tol and abs(v - tv) <= tol, (cx, cy, u, v)
    assert (r.best_nx, r.best_ny, r.best_sum) == (r0.best_nx, r0.best_ny, r0.best_sum)
    for k in st0:
        assert np.array_equal(st[k], st0[k]), k
    xs, ys = G.default_grid()
    bi = cells["best_index"]
    assert np.array_equal(cells["best_nx"], np.array(xs)[bi // 80]) and np.array_equal(cells["best_ny"], np.array(ys)[bi % 80])


def test_error_paths(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_CAPACITY, BF_ERR_STATE, BfError

    def raises(code, call):
        with pytest.raises(BfError) as e:
            call()
        assert e.value.code == code

    ev = _golden()
    small = _opts(accel_mod)
    acc = _accel(accel_mod, ev)
    try:
        raises(BF_ERR_ARG, lambda: acc.global_set_cells(90, 120, 16, 16))       # no window
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(small))
        acc.global_set_window(3, 15)
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(small))              # no cells
        for bad in ((0, 120, 16, 16), (90, -1, 16, 16), (90, 120, 0, 16), (90, 120, 16, -3)):
            raises(BF_ERR_ARG, lambda: acc.global_set_cells(*bad))
        raises(BF_ERR_ARG, lambda: acc.global_set_cells(int(ev[0].max()), 120, 16, 16))    # an event outside the sensor
        raises(BF_ERR_ARG, lambda: acc.global_set_cells(90, int(ev[1].max()), 16, 16))
        raises(BF_ERR_ARG, lambda: acc.global_set_cells(257, 256, 1, 1))        # 65 792 cells
        assert acc.global_set_cells(256, 256, 1, 1).n_cell_x == 256             # 65 536: the most
        acc.global_set_cells(90, 120, 16, 16)
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(small, cells_cap=47))                            # short buffers
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(small, want_surface=True, surface_cap=48 * 35 - 1))
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(accel_mod.Accel.global_search_opts(x_step=0.0)))
        acc.global_set_cells(90, 120, 1, 1)
        raises(BF_ERR_CAPACITY, lambda: acc.global_search_cells(want_surface=True))     # 10 800 cells x 14 400 > 2^27
        r, cells, _ = acc.global_search_cells(small)                                    # ... and fine without a surface
        assert cells.shape == (90, 120) and cells["events"].sum() == len(ev[0])
        acc.global_set_window(3, 15)                                                    # the window clears the cells
        raises(BF_ERR_ARG, lambda: acc.global_search_cells(small))
        acc.global_set_cells(90, 120, 16, 16)
        acc.upload_events(*ev)                                                          # an upload in between
        raises(BF_ERR_STATE, lambda: acc.global_search_cells(small))
        raises(BF_ERR_STATE, lambda: acc.global_set_cells(90, 120, 16, 16))
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        assert acc.global_search_cells(small)[1]["events"].sum() == len(ev[0])
    finally:
        acc.close()


def test_empty_cloud(accel_mod):
    acc = accel_mod.Accel(device=0, max_events=16)
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        acc.global_set_window(3, 5)
        g = acc.global_set_cells(20, 30, 8, 8)
        assert (g.n_cell_x, g.n_cell_y) == (3, 4)
        r, cells, surf = acc.global_search_cells(_opts(accel_mod), want_surface=True)
        assert surf.shape == (3, 4, 5, 7) and not surf.any()
        assert (r.best_nx, r.best_ny, r.best_sum) == (XS[0], YS[0], 0)
        assert not cells["events"].any() and not cells["best_index"].any() and not cells["best_sum"].any()
        assert (cells["best_nx"] == XS[0]).all() and (cells["best_ny"] == YS[0]).all()
        assert np.array_equal(cells["best_u"], np.full((3, 4), G.compute_uv(XS[0], YS[0])[0]))
    finally:
        acc.close()
