"""The coarse-to-fine / seeded per-cell search on the GPU (bf_global_search_cells_pyramid): bit for bit against
bf_global_search_cells where the two must agree, and against the numpy restatement (tests/global_pyramid_ref.py).  Every
value is an integer or one IEEE operation: no tolerances."""
import os

import numpy as np
import pytest

import global_cells_ref as GC
import global_pyramid_ref as P
import global_ref as G
import test_global_pyramid_cpu as CPU
from better_flow_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y")
XS, YS = G.sweep_values(-0.002, 0.0025, 0.001), G.sweep_values(-0.003, 0.0035, 0.001)   # 5 x 7: batches of 32 and 3


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


def _moving(n=3000, seed=4, t0_ns=0):
    """(30, -20) px/s on a 40 x 48 patch of a sensor declared 64 x 48: the last rows of cells are empty"""
    sl = synth.make_slice(n, 40, 48, 0.05, seed=seed, velocity=(30.0, -20.0), t0_ns=t0_ns)
    return sl["fr_x"].astype(np.int64), sl["fr_y"].astype(np.int64), sl["t"].astype(np.int64)


def _accel(accel_mod, ev):
    acc = accel_mod.Accel(device=0, max_events=max(len(ev[2]), 1))
    acc.upload_events(*ev)
    return acc


def _opts(accel_mod, xlo, xhi, ylo, yhi, step=0.001):
    return accel_mod.Accel.global_search_opts(x_low=xlo, x_hi=xhi, x_step=step, y_low=ylo, y_hi=yhi, y_step=step)


def _state_equal(acc, ref):
    got = acc.global_get_events()
    for k in STATE_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), k
    u, v = P.best_uv(ref)
    assert np.array_equal(got["best_u"], u) and np.array_equal(got["best_v"], v)


def _check(acc, got, ref, want, n_xy):
    """evaluated list, per-level counts, cells, slice, sparse surface and the per-event state against the restatement"""
    r, cells, ev, surf, info = got
    assert (info.n_x, info.n_y) == (r.n_x, r.n_y) == n_xy
    assert list(ev) == want["evaluated"] and info.evaluated == len(want["evaluated"])
    assert info.levels_run == len(want["level_count"])
    assert list(info.level_count) == want["level_count"] + [0] * (8 - info.levels_run)
    for k in GC.CELL_FIELDS:
        assert np.array_equal(cells[k], want["cells"][k]), k
    assert (r.best_nx, r.best_ny, r.best_sum) == want["slice"]
    if surf is not None:
        assert np.array_equal(surf.reshape(-1, len(ev)), want["surface"])
    _state_equal(acc, ref)


# 16 x 16: ragged against 90 x 120, below 256 events per cell (work-groups of 64); 90 x 120: one cell (work-groups of 256);
# 1 x 120: one cell per sensor row
@pytest.mark.parametrize("rows,cols", [(16, 16), (90, 120), (1, 120)])
def test_one_level_is_the_exhaustive_search(accel_mod, rows, cols):
    ev = _golden()
    o = _opts(accel_mod, -0.002, 0.0025, -0.003, 0.0035)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, rows, cols)
        r0, cells0, surf0 = acc.global_search_cells(o, want_surface=True)
        st0 = acc.global_get_events()
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, rows, cols)
        r, cells, evl, surf, info = acc.global_search_cells_pyramid(o, levels=1, want_surface=True)
        st = acc.global_get_events()
        assert list(evl) == list(range(35)) and info.evaluated == 35 and list(info.level_count)[:2] == [35, 0]
        assert np.array_equal(cells, cells0) and cells["best_sum"].any()
        assert (r.best_nx, r.best_ny, r.best_sum, r.n_x, r.n_y) == (r0.best_nx, r0.best_ny, r0.best_sum, 5, 7)
        assert np.array_equal(surf, surf0.reshape(surf.shape))
        for k in st0:
            assert np.array_equal(st[k], st0[k]), k
        # without the optional outputs: the same answers
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, rows, cols)
        _, cells2, _, none, _ = acc.global_search_cells_pyramid(o)
        assert none is None and np.array_equal(cells2, cells0)
    finally:
        acc.close()


# GC.tie_slice on 7 x 5 candidates and 3 x 3 cells: S(k, cell) equal and non-zero for every k (one level: batches of 32 and
# 3; two levels: 12 strided candidates, then the 3 new ones around candidate 0), and all zero (no cell has a centre: the
# second level is empty).  Every cell and the slice answer candidate 0.
@pytest.mark.parametrize("equal,levels,count", [(True, 1, [35]), (True, 2, [12, 3]), (False, 1, [35]), (False, 2, [12, 0])])
def test_ties_keep_the_lowest_candidate(accel_mod, equal, levels, count):
    ev = GC.tie_slice(equal)
    lat = GC.TIE_EQUAL if equal else GC.TIE_ZERO
    xs, ys = G.sweep_values(lat[0], lat[1], 0.001), G.sweep_values(lat[2], lat[3], 0.001)
    ref = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=3, metric_wsize=15)
    want = P.search_pyramid(ref, xs, ys, levels, 2, 1)
    assert want["level_count"] == count and not want["cells"]["best_index"].any()
    assert (want["surface"] == want["surface"][:, :1]).all() and want["surface"][:, 0].astype(bool).sum() == (8 if equal else 0)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(*GC.TIE_GRID)
        got = acc.global_search_cells_pyramid(_opts(accel_mod, *lat), levels=levels, factor=2, radius=1, want_surface=True)
        _check(acc, got, ref, want, (7, 5))
        assert not got[1]["best_index"].any() and (got[0].best_nx, got[0].best_ny) == (xs[0], ys[0])
    finally:
        acc.close()


# The lattice holds the motion's candidate (0.0381, -0.0254) two steps from its low-x edge and at its high-y edge, so the
# refinement windows are clipped; 23 x 13 is no multiple of any stride (2, 4, 16).
LAT = (0.036, 0.0585, -0.0375, -0.0250)


@pytest.mark.parametrize("levels,factor,radius", [(2, 2, 1), (3, 2, 3), (2, 4, 3), (3, 4, 1)])
def test_device_equals_restatement(accel_mod, levels, factor, radius):
    ev = _moving()
    xs, ys = G.sweep_values(LAT[0], LAT[1], 0.001), G.sweep_values(LAT[2], LAT[3], 0.001)
    assert (len(xs), len(ys)) == (23, 13)
    ref = GC.GlobalCells(*ev, 64, 48, 16, 16, scale=3, metric_wsize=15)
    assert (ref.events.reshape(4, 3)[3] == 0).all() and ref.events.reshape(4, 3)[:2].all()
    want = P.search_pyramid(ref, xs, ys, levels, factor, radius)
    assert len(want["evaluated"]) < 23 * 13 and want["level_count"][-1] > 0
    bi = want["cells"]["best_index"][:2]
    assert (bi // 13 < radius).any() or (bi % 13 > 12 - radius).any()             # a final window reaches past an edge
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        got = acc.global_search_cells_pyramid(_opts(accel_mod, *LAT), levels=levels, factor=factor, radius=radius,
                                              want_surface=True)
        _check(acc, got, ref, want, (23, 13))
    finally:
        acc.close()


def test_sparse_surface_is_a_subset_of_the_exhaustive_surface(accel_mod):
    ev = _moving()
    o = _opts(accel_mod, *LAT)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        _, _, full = acc.global_search_cells(o, want_surface=True)
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        _, cells, evl, surf, info = acc.global_search_cells_pyramid(o, levels=3, factor=2, radius=2, want_surface=True)
    finally:
        acc.close()
    flat = full.reshape(12, -1)
    assert 0 < info.evaluated < flat.shape[1] and len(set(evl)) == len(evl)
    assert np.array_equal(surf.reshape(12, -1), flat[:, evl])
    order = np.sort(evl)
    sub = flat[:, order]
    assert np.array_equal(cells["best_index"].ravel(), order[np.argmax(sub, axis=1)])      # the first largest of the subset
    assert np.array_equal(cells["best_sum"].ravel(), sub.max(axis=1))


def test_seeded_from_the_previous_slice(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BfError
    ev_a, ev_b = _moving(seed=4), _moving(seed=7)          # the same motion, other events
    xs, ys = G.sweep_values(LAT[0], LAT[1], 0.001), G.sweep_values(LAT[2], LAT[3], 0.001)
    o = _opts(accel_mod, *LAT)
    acc = _accel(accel_mod, ev_a)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        _, cells_a, _, _, _ = acc.global_search_cells_pyramid(o, levels=3, factor=2, radius=2)
        seeds = cells_a["best_index"].copy()
        seeds[cells_a["events"] == 0] = -1
        seeds[0, 0] = -1                                                            # a cell with events and no seed
        acc.upload_events(*ev_b)
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        got = acc.global_search_cells_pyramid(o, levels=1, radius=2, seeds=seeds, want_surface=True)
        ref = GC.GlobalCells(*ev_b, 64, 48, 16, 16, scale=3, metric_wsize=15)
        want = P.search_pyramid(ref, xs, ys, 1, 2, 2, seeds=seeds)
        assert len(want["evaluated"]) <= 25 * 5
        _check(acc, got, ref, want, (23, 13))
        # two levels around the seeds: strides 2 and 1
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        got = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1, seeds=seeds, want_surface=True)
        ref = GC.GlobalCells(*ev_b, 64, 48, 16, 16, scale=3, metric_wsize=15)
        _check(acc, got, ref, P.search_pyramid(ref, xs, ys, 2, 2, 1, seeds=seeds), (23, 13))
        # nothing to evaluate: every seed -1, or seeds on empty cells only
        before = acc.global_get_events()
        for bad in (np.full((4, 3), -1), np.where(cells_a["events"] == 0, 5, -1)):
            with pytest.raises(BfError) as e:
                acc.global_search_cells_pyramid(o, levels=1, seeds=bad)
            assert e.value.code == BF_ERR_ARG
        after = acc.global_get_events()
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        acc.close()


def test_mixed_with_global_search_on_one_window(accel_mod):
    ev = _moving()
    xs, ys = G.sweep_values(LAT[0], LAT[1], 0.001), G.sweep_values(LAT[2], LAT[3], 0.001)
    xs2, ys2 = G.sweep_values(0.030, 0.0355, 0.001), G.sweep_values(-0.030, -0.0255, 0.001)     # 6 x 5, beside the lattice
    ref = GC.GlobalCells(*ev, 64, 48, 16, 16, scale=3, metric_wsize=15)
    want = P.search_pyramid(ref, xs, ys, 2, 4, 1)
    rsurf, rbest = ref.search(xs2, ys2)                                                 # folds on into the same state
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        got = acc.global_search_cells_pyramid(_opts(accel_mod, *LAT), levels=2, factor=4, radius=1)
        assert list(got[2]) == want["evaluated"]
        r, surf = acc.global_search(_opts(accel_mod, 0.030, 0.0355, -0.030, -0.0255))
        assert np.array_equal(surf, rsurf) and (r.best_nx, r.best_ny, r.best_sum) == rbest
        _state_equal(acc, ref)
    finally:
        acc.close()


def test_two_motions_recovered(accel_mod):
    """The committed setting of tests/test_global_pyramid_cpu.py on the two-motion slice, default lattice: the device's
    eight winners are the restatement's (which that file holds to 2 grid steps of the truth), from a fraction of the lattice."""
    ev, xs, ys, grid, (scale, mw) = CPU.recovery_case()
    ref, want = CPU.recovery_reference()
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(scale, mw)
        acc.global_set_cells(*grid)
        r, cells, evl, _, info = acc.global_search_cells_pyramid(**CPU.RECOVERY_SETTING)
    finally:
        acc.close()
    assert (info.n_x, info.n_y) == (180, 80) and info.evaluated < 180 * 80
    print("evaluated %d of 14400, per level %s" % (info.evaluated, list(info.level_count)[:info.levels_run]))
    assert list(evl) == want["evaluated"]
    for k in GC.CELL_FIELDS:
        assert np.array_equal(cells[k], want["cells"][k]), k
    assert (r.best_nx, r.best_ny, r.best_sum) == want["slice"]
    CPU.check_recovery(cells)


def test_empty_cloud(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BfError
    acc = accel_mod.Accel(device=0, max_events=16)
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        acc.global_set_window(3, 5)
        acc.global_set_cells(20, 30, 8, 8)
        o = _opts(accel_mod, -0.002, 0.0025, -0.003, 0.0035)
        r, cells, evl, surf, info = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1, want_surface=True)
        assert list(evl) == P.strided_level(5, 7, 2) and list(info.level_count)[:3] == [12, 0, 0] and info.levels_run == 2
        assert surf.shape == (3, 4, 12) and not surf.any()
        assert (r.best_nx, r.best_ny, r.best_sum) == (XS[0], YS[0], 0)
        assert not cells["events"].any() and not cells["best_index"].any() and not cells["best_sum"].any()
        assert (cells["best_nx"] == XS[0]).all() and (cells["best_ny"] == YS[0]).all()
        with pytest.raises(BfError) as e:                                  # seeds on a slice without events: nothing to do
            acc.global_search_cells_pyramid(o, levels=1, seeds=np.zeros((3, 4), np.int64))
        assert e.value.code == BF_ERR_ARG
    finally:
        acc.close()


def test_error_paths_leave_the_state(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_STATE, BfError

    def raises(code, call):
        with pytest.raises(BfError) as e:
            call()
        assert e.value.code == code

    ev = _moving()
    o = _opts(accel_mod, *LAT)
    acc = _accel(accel_mod, ev)
    try:
        raises(BF_ERR_ARG, lambda: acc.global_search_cells_pyramid(o, levels=2))            # no window
        acc.global_set_window(3, 15)
        raises(BF_ERR_ARG, lambda: acc.global_search_cells_pyramid(o, levels=2))            # no cells
        acc.global_set_cells(64, 48, 16, 16)
        _, _, _, _, info = acc.global_search_cells_pyramid(o, levels=2, factor=4, radius=1)   # a state to keep
        before = acc.global_get_events()
        assert before["max_score"].max() > 0
        p = acc.global_search_cells_pyramid
        for bad in (dict(levels=0), dict(levels=9), dict(levels=2, factor=1), dict(levels=2, radius=0), dict(levels=2, radius=65),
                    dict(levels=3, factor=5),                       # stride 25 on a 23 x 13 lattice
                    dict(levels=1, evaluated_cap=23 * 13 - 1),      # short at level 0
                    dict(levels=2, factor=2, radius=3, evaluated_cap=12 * 7 + 1),            # short at level 1: the state is put back
                    dict(levels=2, cells_cap=11),
                    dict(levels=2, factor=2, want_surface=True, surface_cap=12 * (12 * 7 + 1)),
                    dict(levels=1, seeds=np.full((4, 3), 23 * 13)), dict(levels=1, seeds=np.full((4, 3), -2))):
            raises(BF_ERR_ARG, lambda: p(o, **bad))
        raises(BF_ERR_ARG, lambda: p(accel_mod.Accel.global_search_opts(x_step=0.0), levels=2))
        after = acc.global_get_events()
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        acc.upload_events(*ev)                                                              # an upload since the window
        raises(BF_ERR_STATE, lambda: p(o, levels=2))
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 48, 16, 16)
        assert p(o, levels=2, factor=4, radius=1)[4].evaluated == info.evaluated
    finally:
        acc.close()
