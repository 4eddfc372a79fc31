"""The interpolated cell flow field on the GPU (bf_global_project_field): bit for bit against the numpy restatement
(tests/global_field_ref.py) -- image, scores, S_f, the per-cell sums and the per-event nx / ny / u / v -- and, where the
definition says so, against the device's own bf_global_project_all and bf_global_project_cells.  Every value is an integer or
one IEEE operation: no tolerances."""
import ctypes as C
import os

import numpy as np
import pytest

import global_cells_ref as GC
import global_field_ref as F
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want):
    """(img, scores, S_f, cell_sums, events) of the device against the restatement's (img, scores, S_f, cell_sums, nx_e, ny_e)"""
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float32 and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert got[2] == want[2]
    assert got[3].dtype == np.int64 and np.array_equal(got[3], want[3])
    assert int(got[3].sum()) == got[2]
    ev = got[4]
    assert np.array_equal(_bits(ev["nx"]), _bits(want[4])) and np.array_equal(_bits(ev["ny"]), _bits(want[5]))
    u, v = F.event_uv(want[4], want[5])
    assert np.array_equal(_bits(ev["u"]), _bits(u)) and np.array_equal(_bits(ev["v"]), _bits(v))


def _same_bits(a, b):
    """two results of the device, with or without the events"""
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[3].tobytes() == b[3].tobytes()
    if len(a) > 4 and len(b) > 4:
        assert all(a[4][k].tobytes() == b[4][k].tobytes() for k in ("nx", "ny", "u", "v"))


# t in [2e7, 3e7): (0.2, -0.15) moves an event by 3 to 5 pixels, so some leave the 24 x 24 image; (3.0, -2.0) removes all
UNIFORM = [(0.0, 0.0), (0.2, -0.15), (-0.03, 0.11), (3.0, -2.0)]


@pytest.mark.parametrize("scale,mw", [(1, 3), (3, 15), (5, 21), (7, 35)])
def test_tie_slice_random_and_uniform_grids(accel_mod, scale, mw):
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=scale, metric_wsize=mw)
    assert gc.events[4] == 0 and (np.delete(gc.events, 4) > 0).all()
    rng = np.random.default_rng(41)
    cx, cy = rng.uniform(-0.2, 0.2, (3, 3)), rng.uniform(-0.2, 0.2, (3, 3))
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(scale, mw)
        g = acc.global_set_cells(*GC.TIE_GRID)
        assert (g.n_cell_x, g.n_cell_y) == (3, 3)
        fresh = acc.global_get_events()
        got = acc.global_project_field(cx, cy, want_events=True)
        _same(got, F.project_field(gc, 8, 8, cx, cy))
        assert got[2] > 0 and len(np.unique(got[4]["nx"])) > 9
        _same_state(acc.global_get_events(), fresh)            # nothing folded
        mx = cx.copy()
        mx[1, 1] += 0.1                                         # the middle cell has no event, and is a corner all the same
        moved = acc.global_project_field(mx, cy, want_events=True)
        _same(moved, F.project_field(gc, 8, 8, mx, cy))
        assert not np.array_equal(moved[4]["nx"], got[4]["nx"]) and np.array_equal(moved[4]["ny"], got[4]["ny"])
        for nx, ny in UNIFORM:                                  # the device's own project_all, and the restatement
            ux, uy = np.full((3, 3), nx), np.full((3, 3), ny)
            res = acc.global_project_field(ux, uy, want_events=True)
            S, img0, cur0 = acc.global_project_all(nx, ny)
            assert np.array_equal(res[0], img0) and np.array_equal(_bits(res[1]), _bits(cur0)) and res[2] == S
            assert (res[4]["nx"] == nx).all() and (res[4]["ny"] == ny).all()
            assert (res[2] == 0) == ((nx, ny) == UNIFORM[-1])   # (3.0, -2.0) carries every event out of the image
            _same(res, F.project_field(gc, 8, 8, ux, uy))
    finally:
        acc.close()


# name: sensor and cells, the grid they give, the run length the grid must choose
TIE_SHAPES = {"odd_5x5": ((24, 24, 5, 5), (5, 5), 64),
              "per_pixel": ((24, 24, 1, 1), (24, 24), 64),
              "one_cell": ((24, 24, 24, 24), (1, 1), 256),
              "one_row": ((24, 24, 24, 8), (1, 3), 64)}


@pytest.mark.parametrize("name", sorted(TIE_SHAPES))
def test_tie_slice_grid_shapes(accel_mod, name):
    grid, shape, run_len = TIE_SHAPES[name]
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15)
    assert (gc.n_cell_x, gc.n_cell_y) == shape
    assert (256 if len(ev[0]) >= 256 * int((gc.events > 0).sum()) else 64) == run_len      # (bf_global_set_cells' rule)
    rng = np.random.default_rng(43)
    cx, cy = rng.uniform(-0.2, 0.2, shape), rng.uniform(-0.2, 0.2, shape)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(*grid)
        got = acc.global_project_field(cx, cy, want_events=True)
        _same(got, F.project_field(gc, grid[2], grid[3], cx, cy))
        assert got[2] > 0
        if name == "per_pixel":                                 # w == 0 everywhere: the piecewise projection
            _same_bits(got, acc.global_project_cells(cx, cy))
            assert np.array_equal(got[4]["nx"], cx[gc.fr_x, gc.fr_y])
        if name == "one_cell":
            S, img0, cur0 = acc.global_project_all(cx[0, 0], cy[0, 0])
            assert np.array_equal(got[0], img0) and np.array_equal(_bits(got[1]), _bits(cur0)) and got[2] == S
    finally:
        acc.close()


def test_golden_slice_ragged_grid(accel_mod):
    """6 000 events, 16 x 16 cells on 90 x 120: a ragged 6 x 8 grid, runs of 64.  With the per-event outputs not asked for, the
    other outputs are the same bits; two calls give identical bytes."""
    ev = _golden()
    gc = GC.GlobalCells(*ev, 90, 120, 16, 16, scale=3, metric_wsize=15)
    assert len(ev[0]) < 256 * int((gc.events > 0).sum())
    rng = np.random.default_rng(11)
    cx, cy = rng.uniform(-0.05, 0.05, (6, 8)), rng.uniform(-0.05, 0.05, (6, 8))
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        a = acc.global_project_field(cx, cy, want_events=True)
        _same(a, F.project_field(gc, 16, 16, cx, cy))
        assert a[2] > 0
        b = acc.global_project_field(cx, cy)
        assert len(b) == 4
        _same_bits(a, b)
        _same_bits(a, acc.global_project_field(cx, cy, want_events=True))
        img, sc, S, none = acc.global_project_field(cx, cy, want_img=False, want_scores=False, want_cell_sums=False)
        assert img is None and sc is None and none is None and S == a[2]
        # one per-event output alone, through the C-ABI itself
        u = np.full(len(ev[0]), -1.0)
        S1 = C.c_int64(-1)
        assert acc.L.bf_global_project_field(acc.h, cx.ctypes.data, cy.ctypes.data, 48, 127.0, None, None, C.byref(S1), None, 0,
                                             None, None, u.ctypes.data, None) == 0
        assert S1.value == a[2] and np.array_equal(_bits(u), _bits(a[4]["u"]))
    finally:
        acc.close()


def test_two_motion_slice(accel_mod):
    """32 x 32 cells of about 2 000 events: runs of 256, eight work-groups adding into one cell's word.  The cells' own
    winners of the default sweep.  The flow is discontinuous, what the piecewise projection is for: the smooth field must
    cost next to nothing (floor 0.98; 1.0031 measured on the CPU with two_motion_subgrid()'s winners)."""
    ev = GC.two_motion_slice()
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    assert gc.events.min() >= 1000
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        r, cells, _ = acc.global_search_cells()
        assert F.cells_valid(cells).all()
        cx, cy = cells["best_nx"], cells["best_ny"]
        got = acc.global_project_field(cx, cy, want_events=True)
        _same(got, F.project_field(gc, 32, 32, cx, cy))
        S_pw = acc.global_project_cells(cx, cy, want_img=False, want_scores=False)[2]
    finally:
        acc.close()
    print("two motions: field / piecewise %.4f" % (got[2] / S_pw))
    assert got[2] >= 0.98 * S_pw


def test_shear_slice_recovery(accel_mod):
    """The shear slice under the eight winners of the restatement's search (global_field_ref.shear_winners), on the device:
    bit for bit the restatement, and the recovery assertions of tests/test_global_field_cpu.py on the device's values
    (measured there: piecewise 1.1430 x the one-flow S, field 1.2043 x, field / piecewise 1.0536; per cell 1.0202 .. 1.0888;
    mirrored grid 0.7880 x S_pw)."""
    ev, cells, (bnx, bny, S_one) = F.shear_winners()
    gc = GC.GlobalCells(*ev, 64, 128, 32, 32, scale=3, metric_wsize=15)
    cx, cy = cells["best_nx"], cells["best_ny"]
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(64, 128, 32, 32)
        got = acc.global_project_field(cx, cy, want_events=True)
        _same(got, F.project_field(gc, 32, 32, cx, cy))
        pw = acc.global_project_cells(cx, cy, want_img=False, want_scores=False)
        one = acc.global_project_all(bnx, bny, want_img=False, want_scores=False)[0]
        mirrored = acc.global_project_field(np.ascontiguousarray(cx[:, ::-1]), np.ascontiguousarray(cy[:, ::-1]), want_img=False,
                                            want_scores=False)[2]
    finally:
        acc.close()
    S_f, S_pw = got[2], pw[2]
    ratio = got[3] / pw[3]
    print("piecewise %.4f x, field %.4f x, field / piecewise %.4f" % (S_pw / one, S_f / one, S_f / S_pw))
    print("per cell field / piecewise: %.4f .. %.4f; mirrored grid %.4f x S_pw" % (ratio.min(), ratio.max(), mirrored / S_pw))
    assert one == S_one
    assert S_f > S_pw > one
    assert (got[3] >= pw[3]).all()
    assert S_f >= (1 + F.SHEAR_GAIN / 2) * S_pw
    assert mirrored < S_pw


def test_calls_share_their_scratch_without_leftovers(accel_mod):
    """bf_global_project_cells, bf_global_project_field and bf_global_project_all run through the same device buffers (point
    and window planes, image, scores, per-cell sums): each call of a mixed sequence, with grids of its own, is bit for bit its
    restatement, whatever the call before left there.  Once with runs of 64 (3 x 3 cells) and once with runs of 256 (one
    cell), on one context."""
    ev = GC.tie_slice(False)
    rng = np.random.default_rng(53)
    acc = _accel(accel_mod, ev)
    try:
        for grid, shape in ((GC.TIE_GRID, (3, 3)), ((24, 24, 24, 24), (1, 1))):
            gc = GC.GlobalCells(*ev, *grid, scale=3, metric_wsize=15)
            ax, ay, bx, by, cx, cy = rng.uniform(-0.2, 0.2, (6,) + shape)
            nx, ny = rng.uniform(-0.2, 0.2, 2)

            def window_and_cells():
                acc.global_set_window(3, 15)
                g = acc.global_set_cells(*grid)
                assert (g.n_cell_x, g.n_cell_y) == shape

            window_and_cells()
            want_pw = PW.project_cells(gc, ax, ay)
            first = acc.global_project_cells(ax, ay)
            _same_bits(first, want_pw)
            assert first[2] > 0
            _same(acc.global_project_field(bx, by, want_events=True), F.project_field(gc, grid[2], grid[3], bx, by))
            S, img, cur = acc.global_project_all(nx, ny)
            img0, cur0, S0 = G.Global(*ev, scale=3, metric_wsize=15).project_all(nx, ny)
            assert S == S0 > 0 and np.array_equal(img, img0) and np.array_equal(_bits(cur), _bits(cur0))
            none, sc, S_f, sums = acc.global_project_field(cx, cy, want_img=False)
            want_f = F.project_field(gc, grid[2], grid[3], cx, cy)
            assert none is None and np.array_equal(_bits(sc), _bits(want_f[1])) and S_f == want_f[2] > 0
            assert np.array_equal(sums, want_f[3])
            last = acc.global_project_cells(ax, ay)
            _same_bits(last, want_pw)
            _same_bits(last, first)
            after = acc.global_get_events()
            window_and_cells()                                      # (resets the per-event state)
            assert acc.global_project_all(nx, ny)[0] == S
            _same_state(after, acc.global_get_events())             # what project_all alone leaves
            assert after["max_score"].any()
    finally:
        acc.close()


def test_empty_cloud(accel_mod):
    acc = accel_mod.Accel(device=0, max_events=16)
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        acc.global_set_window(3, 5)
        g = acc.global_set_cells(20, 30, 8, 8)
        assert (g.n_cell_x, g.n_cell_y) == (3, 4)
        img, sc, S, sums, ev = acc.global_project_field(np.zeros((3, 4)), np.zeros((3, 4)), want_events=True)
        assert S == 0 and sums.shape == (3, 4) and not sums.any()
        assert img.shape == (5, 5) and not img.any() and sc.shape == (0, 0)
        assert all(len(ev[k]) == 0 for k in ("nx", "ny", "u", "v"))
        # nothing is written to the per-event outputs: the C-ABI itself with sentinel buffers
        z, keep, S1 = np.zeros(12), np.full(4, -7.0), C.c_int64(-1)
        assert acc.L.bf_global_project_field(acc.h, z.ctypes.data, z.ctypes.data, 12, 127.0, None, None, C.byref(S1), None, 0,
                                             keep.ctypes.data, keep.ctypes.data, keep.ctypes.data, keep.ctypes.data) == 0
        assert S1.value == 0 and (keep == -7.0).all()
        with pytest.raises(accel_mod.BfError):                  # the grid is checked all the same
            acc.global_project_field(np.full((3, 4), np.nan), np.zeros((3, 4)))
    finally:
        acc.close()


def test_refusals(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_STATE, BfError

    def raises(code, call):
        with pytest.raises(BfError) as e:
            call()
        assert e.value.code == code

    ev = GC.tie_slice(False)
    zeros = np.zeros((3, 3))
    rng = np.random.default_rng(47)
    gx, gy = rng.uniform(-0.05, 0.05, (3, 3)), rng.uniform(-0.05, 0.05, (3, 3))
    acc = _accel(accel_mod, ev)
    try:
        raises(BF_ERR_ARG, lambda: acc.global_project_field(zeros, zeros))                  # no window
        acc.global_set_window(3, 15)
        raises(BF_ERR_ARG, lambda: acc.global_project_field(zeros, zeros))                  # no cells
        acc.global_set_cells(*GC.TIE_GRID)
        acc.global_search_cells(_opts(accel_mod))                                           # (a state that is not the fresh one)
        before = acc.global_get_events()
        assert before["max_score"].any()
        good = acc.global_project_field(gx, gy, want_events=True)
        assert good[2] > 0

        def still_good():
            _same_bits(acc.global_project_field(gx, gy, want_events=True), good)
            _same_state(acc.global_get_events(), before)

        raises(BF_ERR_ARG, lambda: acc.global_project_field(np.zeros(8), np.zeros(8)))      # short grids
        still_good()
        short, S = np.full(8, -1, dtype=np.int64), C.c_int64(-1)                            # short sums: the C-ABI itself
        evb = np.full(len(ev[0]), -7.0)
        assert acc.L.bf_global_project_field(acc.h, gx.ctypes.data, gy.ctypes.data, 9, 127.0, None, None, C.byref(S),
                                             short.ctypes.data, 8, evb.ctypes.data, None, None, None) == BF_ERR_ARG
        assert S.value == -1 and (short == -1).all() and (evb == -7.0).all()
        still_good()
        raises(BF_ERR_ARG, lambda: acc.global_project_field(gx, gy, nz=0.0))
        raises(BF_ERR_ARG, lambda: acc.global_project_field(gx, gy, nz=-127.0))
        still_good()
        pw_good = acc.global_project_cells(gx, gy)
        for bad in (np.inf, -np.inf, np.nan, 1e39, -1e39):                                  # (1e39: infinite as a float)
            cx = gx.copy()
            cx[1, 1] = bad                                                                  # the EMPTY cell: a corner here
            raises(BF_ERR_ARG, lambda: acc.global_project_field(cx, gy))
            raises(BF_ERR_ARG, lambda: acc.global_project_field(gx, cx))
            assert all(np.array_equal(a, b) for a, b in zip(acc.global_project_cells(cx, gy), pw_good))   # ... not read there
            still_good()
        cx = gx.copy()
        cx[2, 0] = np.nan                                                                   # an occupied cell
        raises(BF_ERR_ARG, lambda: acc.global_project_field(cx, gy))
        still_good()
        acc.upload_events(*ev)                                                              # an upload in between
        raises(BF_ERR_STATE, lambda: acc.global_project_field(gx, gy))
        acc.global_set_window(3, 15)                                                        # the window clears the cells
        raises(BF_ERR_ARG, lambda: acc.global_project_field(gx, gy))
        acc.global_set_cells(*GC.TIE_GRID)
        _same_bits(acc.global_project_field(gx, gy, want_events=True), good)
    finally:
        acc.close()


def test_state_is_left_alone(accel_mod):
    """bf_global_get_events, a following bf_global_search_cells and a following seeded and unseeded
    bf_global_search_cells_pyramid give the same bits with bf_global_project_field calls in between as without them."""
    ev = _golden()
    o = _opts(accel_mod, -0.006, 0.0065, -0.004, 0.0045)
    small = _opts(accel_mod)

    def sequence(acc, field):
        def project(cells, **kw):
            if field:
                nx, ny = F.fill_cells(F.cells_valid(cells), cells["best_nx"], cells["best_ny"])
                acc.global_project_field(nx, ny, **kw)

        acc.global_set_window(3, 15)
        acc.global_set_cells(90, 120, 16, 16)
        r1, cells1, ev1, _, _ = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1)
        s1 = acc.global_get_events()
        seeds = np.where(cells1["events"] > 0, cells1["best_index"], -1)
        project(cells1, want_events=True)
        project(cells1, want_img=False, want_scores=False)
        s1b = acc.global_get_events()
        r2, cells2, ev2, surf2, info2 = acc.global_search_cells_pyramid(o, levels=2, factor=2, radius=1, seeds=seeds,
                                                                       want_surface=True)
        project(cells2, want_events=True)
        r3, cells3, ev3, surf3, _ = acc.global_search_cells_pyramid(o, levels=3, factor=2, radius=1, want_surface=True)
        project(cells3)
        r4, cells4, surf4 = acc.global_search_cells(small, want_surface=True)
        return ((r1.best_nx, r1.best_ny, r1.best_sum), cells1, ev1, (r2.best_nx, r2.best_ny, r2.best_sum), cells2, ev2, surf2,
                list(info2.level_count), (r3.best_nx, r3.best_ny, r3.best_sum), cells3, ev3, surf3,
                (r4.best_nx, r4.best_ny, r4.best_sum), cells4, surf4, s1, s1b, acc.global_get_events())

    acc = _accel(accel_mod, ev)
    try:
        a = sequence(acc, True)
        b = sequence(acc, False)
    finally:
        acc.close()
    assert len(a[5]) > 0 and a[4]["best_sum"].any()
    for x, y in zip(a[:-3], b[:-3]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    for x, y in zip(a[-3:], b[-3:]):
        _same_state(x, y)
    _same_state(a[-3], a[-2])
