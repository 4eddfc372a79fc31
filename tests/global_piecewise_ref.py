"""numpy restatement of the piecewise projection (include/bf_accel.h, bf_global_project_cells; DESIGN.md "OptimizerGlobal"),
on top of tests/global_ref.py and the membership of tests/global_cells_ref.py:

  * every event is projected by Event::project (float form) under the candidate (nx_c, ny_c) of the cell of its recorded
    address, with one nz for all; kx = float(nx_c) / nz, ky likewise, once per cell;
  * from there on it is project_all, all events in one image: pixel truncation and acceptance test, the saturating
    scale x scale splat, this build's 8-bit Gaussian, per accepted event the mean of the non-zero blurred pixels of its
    metric_wsize^2 window;
  * S_pw(cell) = sum of floor(score * 2^32) over the accepted events of the cell; S_pw = sum over the cells;
  * no per-event state is folded; the entry of a cell without events is never read.
"""
import numpy as np

import global_ref as G


def project_per_event(fr_x, fr_y, t, nx_e, ny_e, nz=G.NZ):
    """G.project with one (nx, ny) per event: float kx = float(nx) / nz; pr = float(fr) - kx * float(t) / 10000.0"""
    kx = (np.asarray(nx_e, dtype=np.float64).astype(np.float32).astype(np.float64) / nz).astype(np.float32)
    ky = (np.asarray(ny_e, dtype=np.float64).astype(np.float32).astype(np.float64) / nz).astype(np.float32)
    ft = np.asarray(t).astype(np.float32)
    px = (kx * ft).astype(np.float32).astype(np.float64)
    py = (ky * ft).astype(np.float32).astype(np.float64)
    pr_x = np.asarray(fr_x).astype(np.float32).astype(np.float64) - px / 10000.0
    pr_y = np.asarray(fr_y).astype(np.float32).astype(np.float64) - py / 10000.0
    return pr_x, pr_y


def render_and_score(gc, nx_e, ny_e, nz=G.NZ):
    """The slice of gc (a global_cells_ref.GlobalCells: its window and membership; its per-event state is left alone) with
    every event under its own (nx_e, ny_e): one image, the 8-bit Gaussian, the window score, the sums by the event's cell.
    Returns (blurred bordered image uint8, current_scores float32, S int, S(cell) int64 [n_cell_x, n_cell_y])."""
    w = gc.w
    pr_x, pr_y = project_per_event(gc.fr_x, gc.fr_y, gc.t, nx_e, ny_e, nz)
    X, Y, ok = G.pixels(pr_x, pr_y, w)
    s, mw = w["scale"], w["metric_wsize"]
    off = s // 2 + mw // 2
    pts = np.zeros((w["scale_bordered_img_x"], w["scale_bordered_img_y"]), dtype=np.int64)
    np.add.at(pts, (X[ok] + off, Y[ok] + off), 1)
    h = s // 2
    cnt = np.minimum(G._box(pts, -h, h), 255)
    img = G.blur8(cnt, s) if s > 1 else cnt.astype(np.uint8)
    ssum, scnt = G.window_sums(img, w)
    es = ssum[X + off, Y + off]
    ec = scnt[X + off, Y + off]
    f32 = np.where(ec > 0, es / np.maximum(ec, 1), 0.0).astype(np.float32)
    cur = np.zeros((w["scale_img_x"], w["scale_img_y"]), dtype=np.float32)
    cur[X[ok], Y[ok]] = f32[ok]
    sums = np.zeros(gc.n_cells, dtype=np.int64)
    np.add.at(sums, gc.cell[ok], G.score_fixed(es[ok], ec[ok]))      # exact: int64 into int64
    return img, cur, int(sums.sum()), sums.reshape(gc.n_cell_x, gc.n_cell_y)


def project_cells(gc, cell_nx, cell_ny, nz=G.NZ):
    """gc: a global_cells_ref.GlobalCells (its window, membership and event counts; its per-event state is left alone).
    cell_nx / cell_ny: n_cells values in any shape, row-major [n_cell_x, n_cell_y].
    Returns (blurred bordered image uint8, current_scores float32, S_pw int, S_pw(cell) int64 [n_cell_x, n_cell_y])."""
    cx = np.asarray(cell_nx, dtype=np.float64).reshape(-1)
    cy = np.asarray(cell_ny, dtype=np.float64).reshape(-1)
    assert len(cx) == len(cy) == gc.n_cells
    occupied = gc.events > 0
    assert np.isfinite(cx[occupied]).all() and np.isfinite(cy[occupied]).all()
    return render_and_score(gc, cx[gc.cell], cy[gc.cell], nz)


def accepted_per_cell(gc, cell_nx, cell_ny, nz=G.NZ):
    """Events accepted under the piecewise field, per cell (int64 [n_cell_x, n_cell_y])."""
    cx = np.asarray(cell_nx, dtype=np.float64).reshape(-1)
    cy = np.asarray(cell_ny, dtype=np.float64).reshape(-1)
    pr_x, pr_y = project_per_event(gc.fr_x, gc.fr_y, gc.t, cx[gc.cell], cy[gc.cell], nz)
    ok = G.pixels(pr_x, pr_y, gc.w)[2]
    return np.bincount(gc.cell[ok], minlength=gc.n_cells).astype(np.int64).reshape(gc.n_cell_x, gc.n_cell_y)


def half_totals(cell_sums):
    """(left, right) totals of a [2, 4] per-cell array of the two-motion slice: cell columns 0, 1 / 2, 3."""
    a = np.asarray(cell_sums)
    assert a.shape == (2, 4)
    return int(a[:, :2].sum()), int(a[:, 2:].sum())
