"""numpy restatement of the per-cell objective of the exhaustive search (include/bf_accel.h, DESIGN.md "OptimizerGlobal"),
on top of tests/global_ref.py:

  * a grid of cell_rows x cell_cols-pixel cells over the res_x x res_y sensor, anchored at sensor pixel (0, 0);
    n_cell_x = ceil(res_x / cell_rows), n_cell_y = ceil(res_y / cell_cols);
  * an event belongs to the cell of its recorded address: cell = (fr_x // cell_rows) * n_cell_y + fr_y // cell_cols;
  * S(k, cell) = sum of floor(score * 2^32) over the events of the cell accepted under candidate k;
  * a cell's answer is the first candidate in sweep order with the largest S(k, cell) (candidate 0 when all are 0);
  * the per-event best state folds as in Global.project_all.
"""
import numpy as np

import global_ref as G

CELL_FIELDS = ("best_nx", "best_ny", "best_u", "best_v", "best_sum", "best_index", "events")


def two_motion_slice():
    """Two motions on one 64 x 128 sensor: the left half moves at (40, -20) px/s, the right half (columns + 64) at
    (-30, 25) px/s; 16 000 events over 0.2 s, stably sorted by t.  Returns (fr_x, fr_y, t), int64."""
    from better_flow_amd import synth
    a = synth.make_slice(8000, 64, 64, 0.2, seed=5, velocity=(40.0, -20.0))
    b = synth.make_slice(8000, 64, 64, 0.2, seed=6, velocity=(-30.0, 25.0))
    fr_x = np.concatenate([a["fr_x"], b["fr_x"]]).astype(np.int64)
    fr_y = np.concatenate([a["fr_y"], np.asarray(b["fr_y"]).astype(np.int64) + 64]).astype(np.int64)
    t = np.concatenate([a["t"], b["t"]]).astype(np.int64)
    o = np.argsort(t, kind="stable")
    return fr_x[o], fr_y[o], t[o]


TWO_MOTION_TRUTH = {"left": (40.0, -20.0), "right": (-30.0, 25.0)}   # cells 0, 1, 4, 5 / 2, 3, 6, 7 of the 2 x 4 grid
GRID_STEP = 0.001 / G.NZ * 1e5                                        # px/s per candidate step: 0.787


class GlobalCells(G.Global):
    def __init__(self, fr_x, fr_y, t, res_x, res_y, cell_rows, cell_cols, scale=5, metric_wsize=None):
        super().__init__(fr_x, fr_y, t, scale, metric_wsize)
        assert min(res_x, res_y, cell_rows, cell_cols) > 0
        if len(self.fr_x):
            assert 0 <= self.fr_x.min() and self.fr_x.max() < res_x and 0 <= self.fr_y.min() and self.fr_y.max() < res_y
        self.n_cell_x = -(-res_x // cell_rows)
        self.n_cell_y = -(-res_y // cell_cols)
        self.n_cells = self.n_cell_x * self.n_cell_y
        self.cell = (self.fr_x // cell_rows) * self.n_cell_y + self.fr_y // cell_cols
        self.events = np.bincount(self.cell, minlength=self.n_cells).astype(np.int64)

    def project_all_cells(self, nx, ny, nz=G.NZ):
        """Global.project_all with the sum kept per cell: returns S(k, cell), int64 [n_cells]."""
        w = self.w
        img, pr_x, pr_y, X, Y, ok = G.project_img(self.fr_x, self.fr_y, self.t, w, nx, ny, nz)
        off = w["scale"] // 2 + w["metric_wsize"] // 2
        ssum, scnt = G.window_sums(img, w)
        es = ssum[X + off, Y + off]
        ec = scnt[X + off, Y + off]
        f32 = np.where(ec > 0, es / np.maximum(ec, 1), 0.0).astype(np.float32)
        S = np.zeros(self.n_cells, dtype=np.int64)
        np.add.at(S, self.cell[ok], G.score_fixed(es[ok], ec[ok]))      # exact: int64 into int64
        up = ok & (f32.astype(np.float64) > self.max_score)             # apply_score, strict >
        self.max_score[up] = f32[up]
        self.best_nx[up] = nx
        self.best_ny[up] = ny
        self.best_nz[up] = nz
        self.best_pr_x[up] = pr_x[up]
        self.best_pr_y[up] = pr_y[up]
        return S

    def search_cells(self, xs, ys, nz=G.NZ):
        """The sweep (nx outer, ny inner).  Returns (cell surface [n_cell_x, n_cell_y, n_x, n_y], per-cell dict of
        [n_cell_x, n_cell_y] arrays (CELL_FIELDS), slice (best_nx, best_ny, best_sum) from the sum over cells)."""
        surf = np.zeros((self.n_cells, len(xs), len(ys)), dtype=np.int64)
        for i, nx in enumerate(xs):
            for j, ny in enumerate(ys):
                surf[:, i, j] = self.project_all_cells(nx, ny, nz)
        flat = surf.reshape(self.n_cells, -1)
        k = np.argmax(flat, axis=1) if flat.shape[1] else np.zeros(self.n_cells, dtype=np.int64)   # the first maximum
        shape = (self.n_cell_x, self.n_cell_y)
        cells = {"best_index": k.astype(np.int64).reshape(shape), "events": self.events.reshape(shape),
                 "best_sum": flat[np.arange(self.n_cells), k].reshape(shape),
                 "best_nx": np.array([xs[i // len(ys)] for i in k]).reshape(shape),
                 "best_ny": np.array([ys[i % len(ys)] for i in k]).reshape(shape)}
        uv = [G.compute_uv(a, b, nz) for a, b in zip(cells["best_nx"].ravel(), cells["best_ny"].ravel())]
        cells["best_u"] = np.array([p[0] for p in uv], dtype=np.float64).reshape(shape)
        cells["best_v"] = np.array([p[1] for p in uv], dtype=np.float64).reshape(shape)
        total = flat.sum(axis=0)
        b = int(np.argmax(total)) if total.size else 0
        return (surf.reshape(shape + (len(xs), len(ys))), cells,
                (xs[b // len(ys)], ys[b % len(ys)], int(total[b])))


def two_motion_subgrid():
    """Every 6th default nx (4th default ny) plus the five default values around each truth's nearest grid point: 39 x 28."""
    xs, ys = G.default_grid()

    def pick(vals, every, truths):
        keep = set(range(0, len(vals), every))
        for u in truths:
            c = int(np.argmin([abs(G.compute_uv(v, 0.0)[0] - u) for v in vals]))
            keep.update(range(c - 2, c + 3))
        return [vals[i] for i in sorted(keep)]
    return (pick(xs, 6, [TWO_MOTION_TRUTH["left"][0], TWO_MOTION_TRUTH["right"][0]]),
            pick(ys, 4, [TWO_MOTION_TRUTH["left"][1], TWO_MOTION_TRUTH["right"][1]]))


# Ties in the per-cell best, at the smallest shapes where the rule can go wrong: 7 x 5 = 35 candidates (a batch of 32 and
# one of 3), 3 x 3 cells (9: one full group of 8 cells in the best kernel and one cell in the next), the middle cell empty.
TIE_GRID = (24, 24, 8, 8)
TIE_EQUAL = (-0.003, 0.0035, -0.002, 0.0025)    # x_low, x_hi, y_low, y_hi at step 0.001
TIE_ZERO = (5.0, 5.0065, 5.0, 5.0045)           # 39 px/s per ns-tick of t / 10000 and more: far off any motion


def tie_slice(equal):
    """300 events on the 24 x 24 sensor, none in the middle cell, the corners occupied.  equal: every t is 0, so every
    candidate leaves every event on its own pixel and S(k, cell) is the same non-zero number for all k.  Otherwise t lies
    in [2e7, 3e7): under TIE_ZERO every event leaves the image (by 78 pixels or more) and every S(k, cell) is 0."""
    rng = np.random.default_rng(17)
    fr_x, fr_y = rng.integers(0, 24, 600), rng.integers(0, 24, 600)
    keep = ~((fr_x // 8 == 1) & (fr_y // 8 == 1))
    fr_x, fr_y = fr_x[keep][:300], fr_y[keep][:300]
    fr_x[:2], fr_y[:2] = (0, 23), (0, 23)
    t = np.zeros(300, dtype=np.int64) if equal else np.sort(rng.integers(20000000, 30000000, 300))
    return fr_x.astype(np.int64), fr_y.astype(np.int64), t.astype(np.int64)
