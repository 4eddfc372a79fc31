"""The held flow of the exhaustive search on the GPU (bf_global_hold_field, bf_global_hold_best) and everything that reads it
(bf_global_get_flow, the flow field, its colour coding, the flow frame and its ticket form, bf_global_emit_slice), against the
numpy restatement (tests/global_flow_ref.py), on the inputs of tests/test_gpu_global_field.py.

Bit for bit: (nx, ny), the positions, the owner planes, the field against the device's own held (u, v), the colour coding of
the device's own field, every frame payload.  Bounded: the held (u, v) against the host's compute_uv (global_flow_ref.UV_REL,
derived there; the largest difference seen is printed: pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import flowimg_ref as FI
import global_cells_ref as GC
import global_field_ref as F
import global_flow_ref as R
import global_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = (FI.LAST_UPLOADED, FI.FIRST_UPLOADED)
MODES = (R.CELLS, R.FIELD)
STATE_KEYS = ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y", "best_u", "best_v")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _accel(accel_mod, ev, res):
    acc = accel_mod.Accel(device=0, max_events=max(len(ev[2]), 1), max_rows=3 * res[0] + 3, max_cols=3 * res[1] + 3)
    acc.upload_events(*ev)
    return acc


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


def check_get_flow(acc, want, what):
    """bf_global_get_flow against the restatement; returns the restatement with the device's own (u, v) in place of the host's."""
    got = acc.global_get_flow()
    for k in ("nx", "ny", "pr_x", "pr_y"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
    for k in ("u", "v"):
        rel, zeros = R.uv_bound(got[k], want[k])
        print("%s: largest relative difference of %s against the host %.3g (%.2f x 2^-52)" % (what, k, rel, rel * 2.0 ** 52))
        assert zeros and rel <= R.UV_REL, (what, k, rel)
    # any subset of the outputs gives the same values
    part = acc.global_get_flow(keys=("u", "pr_y"))
    assert np.array_equal(_bits(part["u"]), _bits(got["u"])) and np.array_equal(_bits(part["pr_y"]), _bits(got["pr_y"]))
    return dict(want, u=got["u"], v=got["v"])


def check_renders(acc, dev, ev, res, what, moving=True):
    """Flow field, colour coding and flow frame of the held flow under both rules; dev: check_get_flow's result."""
    left, right = R.frame_tiles(dev, ev[0], ev[1], *res)
    out = []
    for rule in RULES:
        owner, U, V = acc.global_flow_field(*res, rule)
        ro, rU, rV = R.flow_field(dev, *res, rule)
        assert np.array_equal(owner, ro), (what, rule, int((owner != ro).sum()))
        assert np.array_equal(_bits(U), _bits(rU)) and np.array_equal(_bits(V), _bits(rV)), (what, rule)   # the held (u, v) of the owner
        bgr, hs = acc.global_color_flow_img(*res, rule, want_hs=True)
        live = (owner >= 0) & ((U != 0) | (V != 0))
        near = live & FI.at_risk(U, V)
        assert near.sum() == 0, (what, rule, int(near.sum()))       # the inputs keep clear of the byte boundaries
        assert (live.sum() > 0) == moving, (what, rule)
        rb, rhs = FI.color_flow(owner, U, V)
        assert np.array_equal(hs, rhs) and np.array_equal(bgr, rb), (what, rule)
        assert (bgr[owner < 0] == 255).all()
        p, a, f = acc.global_render_flow_frame(*res, rule)
        assert np.array_equal(f.view(np.uint32), FI.flo_payload(owner, U, V).view(np.uint32)), (what, rule)
        fr = FI.flow_frame(left, bgr, right)
        assert np.array_equal(p, FI.ppm_payload(fr)) and np.array_equal(a, FI.avi_payload(fr)), (what, rule)
        out.append((owner, U, V, bgr, p, a, f))
    return out


def check_case(accel_mod, ev, res, grid, cx, cy, what, scale=3, mw=15, run_len=None, moving=True):
    gc = GC.GlobalCells(*ev, *res, *grid, scale=scale, metric_wsize=mw)
    assert np.shape(cx) == (gc.n_cell_x, gc.n_cell_y)
    if run_len is not None:
        assert (256 if len(ev[0]) >= 256 * int((gc.events > 0).sum()) else 64) == run_len      # (bf_global_set_cells' rule)
    acc = _accel(accel_mod, ev, res)
    try:
        acc.global_set_window(scale, mw)
        acc.global_set_cells(*res, *grid)
        for mode in MODES:
            acc.global_hold_field(cx, cy, mode=mode)
            dev = check_get_flow(acc, R.hold_field(gc, grid[0], grid[1], cx, cy, mode), "%s mode %d" % (what, mode))
            check_renders(acc, dev, ev, res, "%s mode %d" % (what, mode), moving)
    finally:
        acc.close()


# name: cells of the 24 x 24 sensor, the grid they give, the run length the grid must choose
TIE_SHAPES = {"3x3": ((8, 8), (3, 3), 64), "odd_5x5": ((5, 5), (5, 5), 64), "per_pixel": ((1, 1), (24, 24), 64),
              "one_cell": ((24, 24), (1, 1), 256), "one_row": ((24, 8), (1, 3), 64)}


@pytest.mark.parametrize("name", sorted(TIE_SHAPES))
def test_tie_slice_grid_shapes(accel_mod, name):
    grid, shape, run_len = TIE_SHAPES[name]
    rng = np.random.default_rng(61)
    cx, cy = rng.uniform(-0.2, 0.2, shape), rng.uniform(-0.2, 0.2, shape)
    check_case(accel_mod, GC.tie_slice(False), (24, 24), grid, cx, cy, name, run_len=run_len)


def test_golden_slice_ragged_grid(accel_mod):
    """6 000 events, 16 x 16 cells on 90 x 120: a ragged 6 x 8 grid, runs of 64."""
    rng = np.random.default_rng(11)
    cx, cy = rng.uniform(-0.05, 0.05, (6, 8)), rng.uniform(-0.05, 0.05, (6, 8))
    check_case(accel_mod, _golden(), (90, 120), (16, 16), cx, cy, "golden", run_len=64)


def test_shear_slice_runs_of_256(accel_mod):
    """16 000 events in 2 x 4 cells of 32 x 32: runs of 256, every cell split over several work-groups."""
    rng = np.random.default_rng(13)
    cx, cy = rng.uniform(-0.05, 0.05, (2, 4)), rng.uniform(-0.05, 0.05, (2, 4))
    check_case(accel_mod, F.shear_slice(), (64, 128), (32, 32), cx, cy, "shear", run_len=256)


def test_a_cell_carried_off_the_sensor(accel_mod):
    """(3.0, -2.0) moves an event by 470 pixels and more: the corner cell's events own no pixel in the piecewise mode, and the
    restatement still holds; nothing is written out of the planes."""
    ev = GC.tie_slice(False)
    rng = np.random.default_rng(67)
    cx, cy = rng.uniform(-0.1, 0.1, (3, 3)), rng.uniform(-0.1, 0.1, (3, 3))
    cx[0, 0], cy[0, 0] = 3.0, -2.0
    check_case(accel_mod, ev, (24, 24), (8, 8), cx, cy, "off sensor")
    gc = GC.GlobalCells(*ev, 24, 24, 8, 8, scale=3, metric_wsize=15)
    owner = R.flow_field(R.hold_field(gc, 8, 8, cx, cy, R.CELLS), 24, 24, FI.LAST_UPLOADED)[0]
    gone = np.nonzero(gc.cell == 0)[0]
    assert len(gone) > 0 and not np.isin(owner, gone).any()


def test_one_event(accel_mod):
    ev = tuple(a[:1] for a in GC.tie_slice(False))
    check_case(accel_mod, ev, (24, 24), (8, 8), np.full((3, 3), 0.05), np.full((3, 3), -0.02), "one event")


def test_empty_cloud(accel_mod):
    """BF_OK everywhere, nothing written, the images of no event, no ticket from the emit."""
    acc = accel_mod.Accel(device=0, max_events=16, max_rows=64, max_cols=96)
    em = None
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        acc.global_set_window(3, 5)
        acc.global_set_cells(20, 30, 8, 8)
        em = accel_mod.Emit(acc, 64, 20, 30, 64)
        for hold in (lambda: acc.global_hold_field(np.zeros((3, 4)), np.zeros((3, 4)), mode=R.CELLS),
                     lambda: acc.global_hold_field(np.zeros((3, 4)), np.zeros((3, 4)), mode=R.FIELD), acc.global_hold_best):
            hold()
            keep = np.full(4, -7.0)
            assert acc.L.bf_global_get_flow(acc.h, *[keep.ctypes.data_as(C.c_void_p)] * 6) == 0 and (keep == -7.0).all()
            owner, U, V = acc.global_flow_field(20, 30)
            assert (owner == -1).all() and not U.any() and not V.any()
            assert (acc.global_color_flow_img(20, 30) == 255).all()
            p, a, f = acc.global_render_flow_frame(20, 30)
            assert (p[:, 30:60] == 255).all() and not p[:, :30].any() and not p[:, 60:].any() and (f == np.float32(1e9)).all()
            assert em.slice(0, 0, 0, held=True) == (-1, None)
        with pytest.raises(accel_mod.BfError):                      # the grid is checked all the same
            acc.global_hold_field(np.full((3, 4), np.nan), np.zeros((3, 4)))
    finally:
        if em:
            em.close()
        acc.close()


def test_ticket_form_equals_the_synchronous_form(accel_mod):
    ev = GC.tie_slice(False)
    rng = np.random.default_rng(71)
    cx, cy = rng.uniform(-0.2, 0.2, (3, 3)), rng.uniform(-0.2, 0.2, (3, 3))
    acc = _accel(accel_mod, ev, (24, 24))
    L = acc.L
    fr = C.c_void_p()
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(*GC.TIE_GRID)
        acc.global_hold_field(cx, cy)
        want = acc.global_render_flow_frame(24, 24, FI.FIRST_UPLOADED)
        layouts = accel_mod.BF_FRAME_PPM | accel_mod.BF_FRAME_AVI | accel_mod.BF_FLOW_FRAME_FLO
        assert L.bf_flow_frame_create(acc.h, 24, 24, 2, layouts, C.byref(fr)) == 0
        tickets = []
        for _ in range(2):
            t = C.c_int64(-2)
            assert L.bf_global_flow_frame_render(acc.h, fr, FI.FIRST_UPLOADED, C.byref(t)) == 0
            tickets.append(t.value)
        assert tickets == [0, 1]
        t = C.c_int64(-2)
        assert L.bf_global_flow_frame_render(acc.h, fr, FI.FIRST_UPLOADED, C.byref(t)) == accel_mod.BF_ERR_CAPACITY and t.value == -1
        for tk in tickets:
            ppm, avi, flo = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_float)()
            assert L.bf_flow_frame_wait(acc.h, fr, tk, C.byref(ppm), C.byref(avi), C.byref(flo)) == 0
            assert np.array_equal(np.ctypeslib.as_array(ppm, shape=want[0].shape), want[0])
            assert np.array_equal(np.ctypeslib.as_array(avi, shape=want[1].shape), want[1])
            assert np.array_equal(np.ctypeslib.as_array(flo, shape=want[2].shape).view(np.uint32), want[2].view(np.uint32))
            assert L.bf_flow_frame_release(fr, tk) == 0
        # the rolling family renders into the same frame object, from its own state
        t = C.c_int64(-2)
        assert L.bf_flow_frame_render(acc.h, fr, FI.FIRST_UPLOADED, C.byref(t)) == 0 and t.value == 2
        assert L.bf_flow_frame_release(fr, 2) == 0
    finally:
        if fr:
            L.bf_flow_frame_destroy(fr)
        acc.close()


def test_uniform_grid_and_best_state_are_one_flow(accel_mod):
    """(0.005, 0.005) moves every event of the tie slice (t in [2e7, 3e7)) down by 0.08 to 0.12 pixels: inside the scaled
    window's acceptance test for all of them, so one project_all leaves that candidate as every event's best.  hold_best then,
    and hold_field with the uniform grid in either mode, are the same flow: same arrays, same field, same frames."""
    ev = GC.tie_slice(False)
    nx = ny = 0.005
    acc = _accel(accel_mod, ev, (24, 24))
    try:
        acc.global_set_window(3, 15)
        acc.global_set_cells(*GC.TIE_GRID)
        acc.global_project_all(nx, ny)
        assert (acc.global_get_events()["max_score"] > 0).all()     # every event accepted
        results = []
        for hold in (acc.global_hold_best, lambda: acc.global_hold_field(np.full((3, 3), nx), np.full((3, 3), ny), mode=R.CELLS),
                     lambda: acc.global_hold_field(np.full((3, 3), nx), np.full((3, 3), ny), mode=R.FIELD)):
            hold()
            flow = acc.global_get_flow()
            results.append([flow[k] for k in R.KEYS] + list(acc.global_flow_field(24, 24)) +
                           list(acc.global_render_flow_frame(24, 24)))
        assert (results[0][0] == nx).all() and results[0][2].all()
        for other in results[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0], other))
    finally:
        acc.close()


def test_best_state_snapshot(accel_mod):
    """hold_best after a search: the restatement's snapshot bit for bit (pr is best_pr), and a later search does not move it."""
    ev = GC.tie_slice(False)
    g = G.Global(*ev, scale=3, metric_wsize=15)
    xs, ys = G.sweep_values(-0.002, -0.0005, 0.001), G.sweep_values(-0.003, 0.0035, 0.001)     # nx < 0: rows only move up
    g.search(xs, ys)
    acc = _accel(accel_mod, ev, (24, 24))
    try:
        acc.global_set_window(3, 15)
        acc.global_search(accel_mod.Accel.global_search_opts(x_low=-0.002, x_hi=-0.0005, x_step=0.001, y_low=-0.003, y_hi=0.0035,
                                                             y_step=0.001))
        st = acc.global_get_events()
        acc.global_hold_best()                                      # (no cells: none needed)
        dev = check_get_flow(acc, R.hold_best(g), "best")
        assert np.array_equal(_bits(dev["pr_x"]), _bits(st["best_pr_x"])) and np.array_equal(_bits(dev["pr_y"]), _bits(st["best_pr_y"]))
        never = st["max_score"] == 0                               # (the events of the last row: no candidate brings them inside)
        assert never.any() and not dev["u"][never].any() and np.array_equal(dev["pr_x"][never], ev[0][never].astype(np.float64))
        first = check_renders(acc, dev, ev, (24, 24), "best")
        acc.global_set_cells(*GC.TIE_GRID)                          # the cells do not concern this mode
        acc.global_search_cells(accel_mod.Accel.global_search_opts(x_low=0.01, x_hi=0.0125, x_step=0.001, y_low=0.01, y_hi=0.0125,
                                                                   y_step=0.001))
        assert not np.array_equal(acc.global_get_events()["best_nx"], st["best_nx"])
        again = check_renders(acc, dev, ev, (24, 24), "best, after another search")
        assert all(a.tobytes() == b.tobytes() for x, y in zip(first, again) for a, b in zip(x, y))
    finally:
        acc.close()


def test_emit_rows_carry_the_held_flow(accel_mod):
    """Three overlapping slices of one stream on 64 x 128 (a lead, same-instant twins, same-pixel pairs 99 999 and 100 000 ns
    apart, a t == -1 mark), each held with another grid and mode: the rows are emit_ref's, element for element, with the
    device's own held (u, v)."""
    ts, row, col = R.emit_stream()
    slices = R.emit_slices(ts)
    H, W = R.EMIT_SENSOR
    cap = 2 * len(ts)
    rng = np.random.default_rng(73)
    holds = [((32, 32), R.CELLS), ((16, 16), R.FIELD), ((64, 128), None)]      # None: hold_best after one project_all
    acc = accel_mod.Accel(device=0, max_events=len(ts), max_rows=3 * H + 3, max_cols=3 * W + 3)
    em = accel_mod.Emit(acc, cap, H, W, 2 * len(ts))
    try:
        for k, ((first, n, start, lead), (grid, mode)) in enumerate(zip(slices, holds)):
            sl = slice(first, first + n)
            t_loc = ts[sl].astype(np.int64) - start
            assert t_loc.min() >= -1
            acc.upload_events(row[sl].astype(np.int32), col[sl].astype(np.int32), t_loc.astype(np.int32))
            acc.global_set_window(3, 15)
            g = acc.global_set_cells(H, W, *grid)
            if mode is None:
                acc.global_project_all(0.004, -0.003)
                acc.global_hold_best()
            else:
                shape = (g.n_cell_x, g.n_cell_y)
                acc.global_hold_field(rng.uniform(-0.05, 0.05, shape), rng.uniform(-0.05, 0.05, shape), mode=mode)
            flow = acc.global_get_flow(keys=("u", "v"))
            assert flow["u"].any()
            ld = (int(ts[first - 1]), int(row[first - 1]), int(col[first - 1])) if lead else None
            ticket, rows = em.slice(n, first, start, lead=ld, held=True)
            assert ticket == k
            want = R.emit_rows(ts, row, col, slices, k, (flow["u"], flow["v"]), cap)
            assert len(want["t"]) > 0
            for key in ("t", "row", "col"):
                assert np.array_equal(rows[key], want[key]), (k, key)
            for key in ("u", "v"):
                assert np.array_equal(_bits(rows[key]), _bits(want[key])), (k, key)
    finally:
        em.close()
        acc.close()


def _consumers(accel_mod, acc, em, fr, n):
    """Every consumer of the held flow as a call that returns its code."""
    L, h = acc.L, acc.h
    buf = np.zeros(max(n, 1))
    img = np.zeros((24, 72, 3), dtype=np.uint8)
    t = C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return {"get_flow": lambda: L.bf_global_get_flow(h, p(buf), None, None, None, None, None),
            "flow_field": lambda: L.bf_global_flow_field(h, 24, 24, 0, None, p(np.zeros((24, 24))), None),
            "color_flow_img": lambda: L.bf_global_color_flow_img(h, 24, 24, 0, p(img), None),
            "render_flow_frame": lambda: L.bf_global_render_flow_frame(h, 24, 24, 0, p(img), None, None),
            "flow_frame_render": lambda: L.bf_global_flow_frame_render(h, fr, 0, C.byref(t)),
            "emit_slice": lambda: L.bf_global_emit_slice(h, em.h, n, 0, 0, 0, 0, 0, 0, C.byref(t))}


def test_state_errors(accel_mod):
    """BF_ERR_STATE from every consumer before a hold, after an upload, after bf_global_set_window and -- for the grid modes --
    after bf_global_set_cells; the hold's own refusals are those of the projections, and leave a held flow as it was."""
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_STATE, BfError
    ev = GC.tie_slice(False)
    n = len(ev[0])
    rng = np.random.default_rng(47)
    gx, gy = rng.uniform(-0.05, 0.05, (3, 3)), rng.uniform(-0.05, 0.05, (3, 3))
    acc = _accel(accel_mod, ev, (24, 24))
    em = accel_mod.Emit(acc, 4 * n, 24, 24, 4 * n)
    fr = C.c_void_p()
    assert acc.L.bf_flow_frame_create(acc.h, 24, 24, 1, accel_mod.BF_FRAME_PPM, C.byref(fr)) == 0

    def all_refuse(what):
        for name, call in _consumers(accel_mod, acc, em, fr, n).items():
            assert call() == BF_ERR_STATE, (what, name)

    def raises(code, call):
        with pytest.raises(BfError) as e:
            call()
        assert e.value.code == code

    try:
        all_refuse("no window")
        raises(BF_ERR_ARG, acc.global_hold_best)                                            # no window
        raises(BF_ERR_ARG, lambda: acc.global_hold_field(gx, gy))
        acc.global_set_window(3, 15)
        all_refuse("window, no hold")
        raises(BF_ERR_ARG, lambda: acc.global_hold_field(gx, gy))                           # no cells
        acc.global_set_cells(*GC.TIE_GRID)
        all_refuse("cells, no hold")
        for mode in MODES:
            acc.global_hold_field(gx, gy, mode=mode)
            good = acc.global_get_flow()
            # the hold's own refusals: nothing ran, the held flow is as before
            raises(BF_ERR_ARG, lambda: acc.global_hold_field(gx, gy, mode=7))
            raises(BF_ERR_ARG, lambda: acc.global_hold_field(np.zeros(8), np.zeros(8), mode=mode))
            raises(BF_ERR_ARG, lambda: acc.global_hold_field(gx, gy, nz=0.0, mode=mode))
            raises(BF_ERR_ARG, lambda: acc.global_hold_field(gx, gy, nz=-127.0, mode=mode))
            for bad in (np.inf, np.nan, 1e39):
                cx = gx.copy()
                cx[1, 1] = bad                                                              # the EMPTY cell
                if mode == R.FIELD:
                    raises(BF_ERR_ARG, lambda: acc.global_hold_field(cx, gy, mode=mode))    # a corner there
                else:
                    acc.global_hold_field(cx, gy, mode=mode)                                # not read here
                cx = gx.copy()
                cx[2, 0] = bad                                                              # an occupied cell
                raises(BF_ERR_ARG, lambda: acc.global_hold_field(cx, gy, mode=mode))
            flow = acc.global_get_flow()
            assert all(flow[k].tobytes() == good[k].tobytes() for k in R.KEYS)
            acc.global_set_cells(*GC.TIE_GRID)                                              # the cells the hold lives in are gone
            all_refuse("set_cells, mode %d" % mode)
            acc.global_hold_field(gx, gy, mode=mode)
            acc.global_set_window(3, 15)
            all_refuse("set_window, mode %d" % mode)
            acc.global_set_cells(*GC.TIE_GRID)
            acc.global_hold_field(gx, gy, mode=mode)
            acc.upload_events(*ev)
            all_refuse("upload, mode %d" % mode)
            acc.global_set_window(3, 15)
            acc.global_set_cells(*GC.TIE_GRID)
        acc.global_hold_best()
        acc.global_set_cells(24, 24, 5, 5)                                                  # not this mode's concern
        assert acc.L.bf_global_get_flow(acc.h, None, None, None, None, None, None) == 0
        t = C.c_int64()
        assert acc.L.bf_global_emit_slice(acc.h, em.h, n - 1, 0, 0, 0, 0, 0, 0, C.byref(t)) == BF_ERR_STATE   # not its slice
        acc.global_set_window(3, 15)
        all_refuse("set_window, best")
        acc.global_hold_best()
        acc.upload_events(*ev)
        all_refuse("upload, best")
    finally:
        acc.L.bf_flow_frame_destroy(fr)
        em.close()
        acc.close()


def test_state_is_left_alone(accel_mod):
    """The per-event best state, a following bf_global_search_cells, a following bf_global_project_field and the rolling
    bf_flow_field give the same bits with the holds and every consumer in between as without them."""
    ev = _golden()
    n = len(ev[0])
    res = (90, 120)
    o = accel_mod.Accel.global_search_opts(x_low=-0.004, x_hi=0.0045, x_step=0.001, y_low=-0.003, y_hi=0.0035, y_step=0.001)
    rng = np.random.default_rng(79)
    gx, gy = rng.uniform(-0.05, 0.05, (6, 8)), rng.uniform(-0.05, 0.05, (6, 8))

    def sequence(acc, em, with_flow):
        def flow(hold):
            if not with_flow:
                return
            hold()
            acc.global_get_flow()
            acc.global_flow_field(*res)
            acc.global_color_flow_img(*res)
            acc.global_render_flow_frame(*res)
            em.slice(n, 0, 0, held=True)

        acc.upload_events(*ev)
        acc.set_cloud(3, *res)
        acc.project_4param_reinit(-0.013, 0.021, res[0] / 2.0, res[1] / 2.0, 0.00011, 0.00007)
        rolling = acc.flow_field(*res)
        acc.global_set_window(3, 15)
        acc.global_set_cells(*res, 16, 16)
        r1, cells1, _ = acc.global_search_cells(o)
        s1 = acc.global_get_events()
        flow(acc.global_hold_best)
        flow(lambda: acc.global_hold_field(gx, gy, mode=R.CELLS))
        flow(lambda: acc.global_hold_field(gx, gy, mode=R.FIELD))
        s2 = acc.global_get_events()
        field = acc.global_project_field(gx, gy, want_events=True)
        r2, cells2, surf2 = acc.global_search_cells(o, want_surface=True)
        s3 = acc.global_get_events()
        rolling2 = acc.flow_field(*res)
        frame = acc.render_flow_frame(*res)
        flat = [r1.best_nx, r1.best_ny, r1.best_sum, cells1, r2.best_nx, r2.best_ny, r2.best_sum, cells2, surf2]
        flat += list(rolling) + list(rolling2) + list(frame) + list(field[:4]) + [field[4][k] for k in ("nx", "ny", "u", "v")]
        for s in (s1, s2, s3):
            flat += [s[k] for k in STATE_KEYS]
        return flat

    acc = accel_mod.Accel(device=0, max_events=n, max_rows=3 * res[0] + 3, max_cols=3 * res[1] + 3)
    em = accel_mod.Emit(acc, 4 * n, *res, 4 * n)
    try:
        a = sequence(acc, em, True)
        b = sequence(acc, em, False)
    finally:
        em.close()
        acc.close()
    assert len(a) == len(b) and a[3]["best_sum"].any()
    for x, y in zip(a, b):
        assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
