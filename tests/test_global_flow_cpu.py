"""The numpy restatement of the held flow (tests/global_flow_ref.py) against the restatements it stands on: the per-event
values of global_field_ref and global_piecewise_ref, flowimg_ref's field, the search's best state, the oracle's projection
image and emit_ref's table.  No GPU."""
import numpy as np
import pytest

import emit_ref
import flowimg_ref as FI
import global_cells_ref as GC
import global_field_ref as F
import global_flow_ref as R
import global_piecewise_ref as PW
import global_ref as G


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, keys=R.KEYS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.fixture(scope="module")
def tie():
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, *GC.TIE_GRID, scale=3, metric_wsize=15)
    rng = np.random.default_rng(41)
    return ev, gc, rng.uniform(-0.2, 0.2, (3, 3)), rng.uniform(-0.2, 0.2, (3, 3))


def test_field_mode_is_the_field_refs_per_event_values(tie):
    ev, gc, cx, cy = tie
    h = R.hold_field(gc, 8, 8, cx, cy, R.FIELD)
    nx, ny = F.field_at_events(gc, 8, 8, cx, cy)
    u, v = F.event_uv(nx, ny)
    pr_x, pr_y = PW.project_per_event(gc.fr_x, gc.fr_y, gc.t, nx, ny)
    _same(h, dict(nx=nx, ny=ny, u=u, v=v, pr_x=pr_x, pr_y=pr_y))
    assert len(np.unique(h["nx"])) > 9 and (h["pr_x"] != gc.fr_x).any()
    # another nz: the positions and the flow scale with it, (nx, ny) do not
    h2 = R.hold_field(gc, 8, 8, cx, cy, R.FIELD, nz=64.0)
    _same(h, h2, ("nx", "ny"))
    u2, v2 = F.event_uv(nx, ny, 64.0)
    _same(h2, dict(u=u2, v=v2), ("u", "v"))
    assert not np.array_equal(h2["u"], h["u"])


def test_cells_mode_is_the_piecewise_refs_per_event_values(tie):
    ev, gc, cx, cy = tie
    bad = cx.copy()
    bad[1, 1] = np.nan                                              # the empty cell is not read
    h = R.hold_field(gc, 8, 8, bad, cy, R.CELLS)
    nx, ny = cx.reshape(-1)[gc.cell], cy.reshape(-1)[gc.cell]
    pr_x, pr_y = PW.project_per_event(gc.fr_x, gc.fr_y, gc.t, nx, ny)
    u, v = F.event_uv(nx, ny)
    _same(h, dict(nx=nx, ny=ny, u=u, v=v, pr_x=pr_x, pr_y=pr_y))
    with pytest.raises(AssertionError):
        R.hold_field(gc, 8, 8, bad, cy, R.FIELD)                    # ... and is a corner of the smooth form


@pytest.mark.parametrize("rule", [FI.LAST_UPLOADED, FI.FIRST_UPLOADED])
def test_flow_field_is_flowimg_ref_fed_the_held_values(tie, rule):
    ev, gc, cx, cy = tie
    h = R.hold_field(gc, 8, 8, cx, cy, R.FIELD)
    owner, U, V = R.flow_field(h, 24, 24, rule)
    ro, rU, rV = FI.flow_field(h["pr_x"], h["pr_y"], h["u"], h["v"], None, 24, 24, rule)
    assert np.array_equal(owner, ro) and np.array_equal(_bits(U), _bits(rU)) and np.array_equal(_bits(V), _bits(rV))
    has = owner >= 0
    assert 0 < has.sum() < len(ev[0])                               # some events share a pixel or leave the sensor
    assert np.array_equal(_bits(U[has]), _bits(h["u"][owner[has]]))
    x, y = FI.trunc_x86(h["pr_x"]), FI.trunc_x86(h["pr_y"])
    inside = (x >= 0) & (x < 24) & (y >= 0) & (y < 24)
    assert not inside.all()
    k = owner[has][0]
    assert inside[k] and owner[x[k], y[k]] == k


def test_per_pixel_cells_make_the_two_modes_one():
    ev = GC.tie_slice(False)
    gc = GC.GlobalCells(*ev, 24, 24, 1, 1, scale=3, metric_wsize=15)
    rng = np.random.default_rng(43)
    cx, cy = rng.uniform(-0.2, 0.2, (24, 24)), rng.uniform(-0.2, 0.2, (24, 24))
    _same(R.hold_field(gc, 1, 1, cx, cy, R.FIELD), R.hold_field(gc, 1, 1, cx, cy, R.CELLS))


@pytest.mark.parametrize("mode", [R.CELLS, R.FIELD])
def test_uniform_grid_gives_every_event_the_same_flow(tie, mode):
    ev, gc, _, _ = tie
    h = R.hold_field(gc, 8, 8, np.full((3, 3), 0.2), np.full((3, 3), -0.15), mode)
    assert (h["nx"] == 0.2).all() and (h["ny"] == -0.15).all()
    assert len(np.unique(h["u"])) == 1 and len(np.unique(h["v"])) == 1
    pr_x, pr_y = G.project(gc.fr_x, gc.fr_y, gc.t, 0.2, -0.15)
    _same(h, dict(pr_x=pr_x, pr_y=pr_y), ("pr_x", "pr_y"))
    zero = R.hold_field(gc, 8, 8, np.zeros((3, 3)), np.zeros((3, 3)), mode)
    assert not zero["u"].any() and not zero["v"].any() and np.array_equal(zero["pr_x"], gc.fr_x.astype(np.float64))


def test_best_mode_reproduces_best_pr_bit_for_bit():
    """A small search: the position derived from the snapshot's (best_nx, best_ny, best_nz) is the best_pr the fold kept, for
    every event -- the accepted ones (two values of nz among them) and the never accepted ones (pr = fr, zero flow)."""
    fr_x, fr_y, t = GC.tie_slice(False)
    fr_x, fr_y = fr_x.copy(), fr_y.copy()
    g = G.Global(fr_x, fr_y, t, scale=3, metric_wsize=15)
    xs, ys = G.sweep_values(-0.002, 0.0025, 0.001), G.sweep_values(-0.003, 0.0035, 0.001)
    g.search(xs[:2], ys, nz=64.0)
    g.search(xs[2:], ys)
    g.project_all(3.0, -2.0)                                         # accepts no event
    h = R.hold_best(g)
    assert len(np.unique(g.best_nz)) == 2 and (g.max_score > 0).any()
    assert np.array_equal(_bits(h["pr_x"]), _bits(g.best_pr_x)) and np.array_equal(_bits(h["pr_y"]), _bits(g.best_pr_y))
    u, v = g.best_uv()
    _same(h, dict(u=u, v=v), ("u", "v"))
    never = G.Global(fr_x, fr_y, t, scale=3, metric_wsize=15)
    never.project_all(3.0, -2.0)
    h0 = R.hold_best(never)
    assert not never.max_score.any() and not h0["u"].any() and not h0["nx"].any()
    assert np.array_equal(h0["pr_x"], fr_x.astype(np.float64)) and np.array_equal(h0["pr_y"], fr_y.astype(np.float64))


def test_projection_tile_equals_the_oracle(oracle_lib, tie):
    """projection_img1 against EventFile::projection_img at scale 1 of the oracle, on the held and on the raw positions."""
    ev, gc, cx, cy = tie
    h = R.hold_field(gc, 8, 8, cx, cy, R.FIELD)
    c = oracle_lib.Cloud(*ev)
    c.pr_x[:], c.pr_y[:] = h["pr_x"], h["pr_y"]
    left, right = R.frame_tiles(h, ev[0], ev[1], 24, 24)
    assert np.array_equal(left, c.projection_img(1, 24, 24, show_final=False))
    assert np.array_equal(right, c.projection_img(1, 24, 24, show_final=True))
    assert left.any() and not np.array_equal(left, right)
    assert not R.projection_img1(np.zeros(0), np.zeros(0), 24, 24).any()


def test_uv_bound_arithmetic():
    assert R.UV_REL == 2.0 ** -50
    host = np.array([0.0, 1.0, -3.0])
    assert R.uv_bound(host, host) == (0.0, True)
    rel, zeros = R.uv_bound(np.array([1e-300, 1.0 + 2.0 ** -52, -3.0]), host)
    assert rel == 2.0 ** -52 and not zeros


def test_emit_rows_split_the_refs_table_by_slice():
    ts, row, col = R.emit_stream()
    assert (np.diff(ts.astype(np.int64)) >= 0).all()
    pix = row * R.EMIT_SENSOR[1] + col
    d = np.diff(ts.astype(np.int64))
    same_pix = pix[1:] == pix[:-1]
    assert (same_pix & (d == 0)).any()                                # twins, adjacent after the stable sort
    sl = R.emit_slices(ts)
    assert sl[0][3] == 1 and sl[1][0] < sl[0][0] + sl[0][1] and sl[2][0] < sl[1][0] + sl[1][1]       # a lead; overlapping
    cap = 2 * len(ts)
    rng = np.random.default_rng(1)
    got, total = [], 0
    for k, (first, n, start, lead) in enumerate(sl):
        uv = (rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
        rows = R.emit_rows(ts, row, col, sl, k, uv, cap)
        total += len(rows["t"])
        got.append(rows)
        g_in = np.nonzero(rows["u"])[0]
        assert len(g_in) > 0
    assert got[0]["t"][0] == ts[0] and got[0]["u"][0] == 0.0         # the lead: zero flow
    assert total == len(emit_ref.device_rows(ts, pix, sl, cap)) == len(emit_ref.host_rows(ts, pix, sl))
    assert len(got[1]["t"]) < sl[1][1] and len(got[2]["t"]) < sl[2][1]   # covered events are not emitted twice
    # the reach: a same-pixel pair 99 999 ns apart and one 100 000 ns apart exist inside the slices
    order = np.lexsort((ts.astype(np.int64), pix))
    dp = np.diff(ts.astype(np.int64)[order])[np.diff(pix[order]) == 0]
    assert (dp == 99999).any() and (dp == 100000).any()


def test_library_exports_the_calls_and_refuses_a_null_context():
    """No device needed: every new entry point exists, is in the binding's list, and returns BF_ERR_ARG without a context."""
    from better_flow_amd import accel
    lib = accel.load()
    calls = {"bf_global_hold_field": (None, None, None, 0, 127.0, accel.BF_GLOBAL_HOLD_FIELD), "bf_global_hold_best": (None,),
             "bf_global_get_flow": (None,) * 7, "bf_global_flow_field": (None, 24, 24, 0, None, None, None),
             "bf_global_color_flow_img": (None, 24, 24, 0, None, None), "bf_global_flow_frame_render": (None, None, 0, None),
             "bf_global_render_flow_frame": (None, 24, 24, 0, None, None, None),
             "bf_global_emit_slice": (None, None, 0, 0, 0, 0, 0, 0, 0, None)}
    for name, args in calls.items():
        assert name in accel.EXPORTS
        assert getattr(lib, name)(*args) == accel.BF_ERR_ARG, name
    assert (accel.BF_GLOBAL_HOLD_CELLS, accel.BF_GLOBAL_HOLD_FIELD) == (R.CELLS, R.FIELD)
