"""numpy restatement of the interpolated cell flow field (include/bf_accel.h, bf_global_project_field;
include/bf_global_field.h; DESIGN.md "OptimizerGlobal"), on top of tests/global_ref.py, the membership of
tests/global_cells_ref.py and the per-event projection of tests/global_piecewise_ref.py:

  * cell a of an axis has its nominal centre at (a + 0.5) * size - 0.5; for the recorded address x: p = 2x + 1 - size,
    D = 2 * size, a0 = floor(p / D), w = p - a0 * D; a0 < 0 -> (0, w = 0); a0 >= n_cell - 1 -> (n_cell - 1, w = 0);
    a1 = min(a0 + 1, n_cell - 1);
  * per event, all double, one operation after the other: tx = wx / Dx, ty = wy / Dy, top = n00 + ty * (n01 - n00),
    bot = n10 + ty * (n11 - n10), n_e = top + tx * (bot - top);
  * kx = float(float(nx_e) / nz) per event; from there on it is the piecewise projection: one image, the 8-bit Gaussian,
    the window score, S_f(cell) = sum of floor(score * 2^32) over the accepted events of the event's own cell;
  * the whole grid is read and must be finite; u / v are Event::compute_uv of (nx_e, ny_e) with the C library's hypot;
  * the fill: a cell without an answer takes the (nx, ny) of the nearest valid cell in cell indices (smallest
    da^2 + db^2, lowest row-major index among equals); (0, 0) without any.
"""
import functools

import numpy as np

import global_cells_ref as GC
import global_pyramid_ref as GP
import global_piecewise_ref as PW
import global_ref as G


def axis(x, size, n_cell):
    """(a0, a1, w) of the addresses x (int64 arrays) on an axis of n_cell cells of `size` pixels; D = 2 * size."""
    x = np.asarray(x, dtype=np.int64)
    p = 2 * x + 1 - size
    D = 2 * size
    a0 = p // D                                  # floor division
    w = p - a0 * D
    lo, hi = a0 < 0, a0 >= n_cell - 1
    a0 = np.where(lo, 0, a0)
    w = np.where(lo, 0, w)
    a0 = np.where(hi, n_cell - 1, a0)
    w = np.where(hi, 0, w)
    a1 = np.minimum(a0 + 1, n_cell - 1)
    return a0, a1, w


def interp(n00, n01, n10, n11, tx, ty):
    top = n00 + ty * (n01 - n00)
    bot = n10 + ty * (n11 - n10)
    return top + tx * (bot - top)


def field_at(x, y, cell_rows, cell_cols, n_cell_x, n_cell_y, cell_nx, cell_ny):
    """The field at the addresses (x, y): (nx_e, ny_e), float64 arrays.  cell_nx / cell_ny: n_cells values, row-major."""
    gx = np.asarray(cell_nx, dtype=np.float64).reshape(n_cell_x, n_cell_y)
    gy = np.asarray(cell_ny, dtype=np.float64).reshape(n_cell_x, n_cell_y)
    assert np.isfinite(gx).all() and np.isfinite(gy).all()          # every cell, with events or without
    a0, a1, wx = axis(x, cell_rows, n_cell_x)
    b0, b1, wy = axis(y, cell_cols, n_cell_y)
    tx = wx.astype(np.float64) / np.float64(2 * cell_rows)
    ty = wy.astype(np.float64) / np.float64(2 * cell_cols)
    return (interp(gx[a0, b0], gx[a0, b1], gx[a1, b0], gx[a1, b1], tx, ty),
            interp(gy[a0, b0], gy[a0, b1], gy[a1, b0], gy[a1, b1], tx, ty))


def field_at_events(gc, cell_rows, cell_cols, cell_nx, cell_ny):
    """gc: a global_cells_ref.GlobalCells laid with cells of cell_rows x cell_cols pixels.  (nx_e, ny_e) per event."""
    return field_at(gc.fr_x, gc.fr_y, cell_rows, cell_cols, gc.n_cell_x, gc.n_cell_y, cell_nx, cell_ny)


def event_uv(nx_e, ny_e, nz=G.NZ):
    """Event::compute_uv of every event's (nx_e, ny_e), with libm's hypot (global_pyramid_ref.compute_uv)."""
    uv = np.array([GP.compute_uv(float(a), float(b), nz) for a, b in zip(nx_e, ny_e)], dtype=np.float64).reshape(-1, 2)
    return uv[:, 0].copy(), uv[:, 1].copy()


def project_field(gc, cell_rows, cell_cols, cell_nx, cell_ny, nz=G.NZ):
    """Returns (blurred bordered image uint8, current_scores float32, S_f int, S_f(cell) int64 [n_cell_x, n_cell_y],
    nx_e, ny_e float64 [n])."""
    nx_e, ny_e = field_at_events(gc, cell_rows, cell_cols, cell_nx, cell_ny)
    return PW.render_and_score(gc, nx_e, ny_e, nz) + (nx_e, ny_e)


def fill_cells(valid, cell_nx, cell_ny):
    """valid: bool [n_cell_x, n_cell_y]; returns filled copies of cell_nx / cell_ny in that shape.  Entries of invalid cells
    are not read (they may be NaN); the entries of valid cells must be finite."""
    valid = np.asarray(valid, dtype=bool)
    nx = np.array(cell_nx, dtype=np.float64).reshape(valid.shape)
    ny = np.array(cell_ny, dtype=np.float64).reshape(valid.shape)
    assert np.isfinite(nx[valid]).all() and np.isfinite(ny[valid]).all()
    va, vb = np.nonzero(valid)                                      # row-major order: argmin takes the first of equals
    for a, b in zip(*np.nonzero(~valid)):
        if len(va) == 0:
            nx[a, b] = ny[a, b] = 0.0
            continue
        k = int(np.argmin((va - a) ** 2 + (vb - b) ** 2))
        nx[a, b], ny[a, b] = nx[va[k], vb[k]], ny[va[k], vb[k]]
    return nx, ny


def cells_valid(cells):
    """The fill's validity of a search's per-cell answers: events > 0 and best_sum > 0."""
    return (np.asarray(cells["events"]) > 0) & (np.asarray(cells["best_sum"]) > 0)


# A hand-made validity mask for the fill, and what it must give.
FILL_MASK = np.array([[1, 0, 0, 1],
                      [0, 0, 0, 0],
                      [0, 1, 0, 0]], dtype=bool)
# the nearest valid cell of every cell, as a row-major index (da^2 + db^2 in cell indices).  Two ties, both to the lower
# index: (1, 2) is 2 from (0, 3) and 2 from (2, 1): 3; (2, 3) is 4 from (0, 3) and 4 from (2, 1): 3.
FILL_FROM = np.array([[0, 0, 3, 3],
                      [0, 9, 3, 3],
                      [9, 9, 9, 3]])


SHEAR = dict(n=16000, H=64, W=128, duration=0.2, seed=5, v_col=-20.0)


def shear_velocity(p_col):
    """The row velocity (px/s) of a scene point at column p_col: linear, -37.5 at column 4, 0 at 64, +37.5 at 124."""
    return 40.0 * (p_col - 64.0) / 64.0


def shear_slice():
    """synth.make_slice's construction with a row velocity linear in the scene point's column: 16 000 events on 64 x 128
    over 0.2 s, seed 5.  Returns (fr_x, fr_y, t), int64, t ascending."""
    from better_flow_amd import synth
    n, H, W, dur, seed = SHEAR["n"], SHEAR["H"], SHEAR["W"], SHEAR["duration"], SHEAR["seed"]
    n_pts = n // 16
    p_row = 10.0 + synth._uniform(seed, 1, n_pts) * (H - 20.0)
    p_col = 10.0 + synth._uniform(seed, 2, n_pts) * (W - 20.0)
    t_ns = np.floor(synth._uniform(seed, 3, n) * (dur * 1e9)).astype(np.int64)
    t_ns.sort(kind="stable")
    pick = (synth.splitmix64(seed, 4, n) % np.uint64(n_pts)).astype(np.int64)
    ts = t_ns.astype(np.float64) * 1e-9
    row = np.floor(p_row[pick] + shear_velocity(p_col[pick]) * ts).astype(np.int64)
    col = np.floor(p_col[pick] + SHEAR["v_col"] * ts).astype(np.int64)
    keep = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    return row[keep], col[keep], t_ns[keep]


def shear_subgrid():
    """The default nx values at even index with |u| <= 46 px/s and the five default ny around the lattice point nearest
    -20 px/s."""
    xs, ys = G.default_grid()
    sx = [v for i, v in enumerate(xs) if i % 2 == 0 and abs(G.compute_uv(v, 0.0)[0]) <= 46.0]
    c = int(np.argmin([abs(G.compute_uv(0.0, v)[1] - SHEAR["v_col"]) for v in ys]))
    return sx, ys[c - 2:c + 3]


@functools.lru_cache(maxsize=None)
def shear_winners():
    """The shear slice on 32 x 32 cells at scale 3, window 15, searched once per process over shear_subgrid(): returns
    (events, per-cell dict of search_cells, the slice's (best_nx, best_ny, S)).  Shared by the CPU and the GPU tests; treat
    it as read-only."""
    ev = shear_slice()
    gc = GC.GlobalCells(*ev, SHEAR["H"], SHEAR["W"], 32, 32, scale=3, metric_wsize=15)
    _, cells, best = gc.search_cells(*shear_subgrid())
    return ev, cells, best


# S_f / S_pw - 1 on the shear slice under shear_winners(), measured by this restatement.  To re-measure: pytest -s
# tests/test_global_field_cpu.py::test_shear_is_recovered_better_by_the_smooth_field prints "field / piecewise <ratio>".
SHEAR_GAIN = 0.0536
