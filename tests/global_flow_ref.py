"""numpy restatement of the held flow of the exhaustive search (include/bf_accel.h, "the held flow"; DESIGN.md
"OptimizerGlobal") and of what reads it, on top of tests/global_field_ref.py, tests/global_piecewise_ref.py,
tests/flowimg_ref.py and tests/emit_ref.py -- TEST INFRASTRUCTURE ONLY.

  * a held flow is, per event in upload order, (nx, ny), (u, v) = Event::compute_uv of them with the flow's nz, and the
    position pr = float(fr) - (kx * float(t)) / 10000.0 with kx = float(float(nx) / nz);
  * the grid modes give an event its cell's entry (CELLS) or the field interpolated at its address (FIELD), with one nz;
    the best mode takes (best_nx, best_ny, best_nz) of every event from a search's state;
  * the renders read it by flowimg_ref's rule with no noise flags: every event takes part;
  * the frame's grey tiles are the scale-1 projection images of the held and of the raw positions;
  * the -o rows of a slice are emit_ref's, with (u, v) of upload index g - first (0 for the lead).

(u, v) here is the HOST's value (libm's hypot); the device's own hypot may differ in the last places, see uv_bound."""
import numpy as np

import emit_ref
import flowimg_ref as FI
import global_field_ref as F
import global_piecewise_ref as PW
import global_pyramid_ref as GP
import global_ref as G

CELLS, FIELD = 1, 2                      # BF_GLOBAL_HOLD_CELLS, BF_GLOBAL_HOLD_FIELD
KEYS = ("nx", "ny", "u", "v", "pr_x", "pr_y")

# |device - host| <= UV_REL * |host| for each of u, v.  Derived, not measured: with c = nz / 100000 (one rounding, the same
# on both sides) the value is ((len / c) * n) / len.  Whatever len either hypot returned, len / c = (len / c)(1 + e1),
# times n: (1 + e2), over len: (1 + e3), |e_i| <= 2^-53, and len cancels: each side is n / c (1 + e1)(1 + e2)(1 + e3), within
# 3 * 2^-53 + O(2^-106) of n / c; two such values differ by at most 6 * 2^-53 + O(2^-106) < 4 * 2^-52 relative to either.
UV_REL = 4 * 2.0 ** -52


def event_uv(nx, ny, nz):
    """Event::compute_uv per event, libm's hypot; nz a scalar or one per event."""
    nz = np.broadcast_to(np.asarray(nz, dtype=np.float64), np.shape(nx))
    uv = np.array([GP.compute_uv(float(a), float(b), float(c)) for a, b, c in zip(nx, ny, nz)], dtype=np.float64).reshape(-1, 2)
    return uv[:, 0].copy(), uv[:, 1].copy()


def _held(fr_x, fr_y, t, nx, ny, nz):
    nx, ny = np.asarray(nx, dtype=np.float64), np.asarray(ny, dtype=np.float64)
    pr_x, pr_y = PW.project_per_event(fr_x, fr_y, t, nx, ny, nz)
    u, v = event_uv(nx, ny, nz)
    return dict(nx=nx, ny=ny, u=u, v=v, pr_x=pr_x, pr_y=pr_y)


def hold_field(gc, cell_rows, cell_cols, cell_nx, cell_ny, mode, nz=G.NZ):
    """gc: a global_cells_ref.GlobalCells laid with cells of cell_rows x cell_cols pixels.  The held flow as a dict of KEYS."""
    cx = np.asarray(cell_nx, dtype=np.float64).reshape(-1)
    cy = np.asarray(cell_ny, dtype=np.float64).reshape(-1)
    assert len(cx) == len(cy) == gc.n_cells and nz > 0
    if mode == CELLS:
        occupied = gc.events > 0
        assert np.isfinite(cx[occupied]).all() and np.isfinite(cy[occupied]).all()     # no empty cell is read
        nx, ny = cx[gc.cell], cy[gc.cell]
    else:
        assert mode == FIELD
        nx, ny = F.field_at_events(gc, cell_rows, cell_cols, cx, cy)                    # (checks the whole grid)
    return _held(gc.fr_x, gc.fr_y, gc.t, nx, ny, nz)


def hold_best(g):
    """g: a global_ref.Global (or GlobalCells) after its searches: the snapshot of its per-event best state."""
    return _held(g.fr_x, g.fr_y, g.t, g.best_nx.copy(), g.best_ny.copy(), g.best_nz.copy())


def flow_field(held, res_x, res_y, rule):
    """(owner, U, V) of flowimg_ref.flow_field fed the held positions and flow; no noise flags."""
    return FI.flow_field(held["pr_x"], held["pr_y"], held["u"], held["v"], None, res_x, res_y, rule)


def projection_img1(pr_x, pr_y, res_x, res_y):
    """EventFile::projection_img at scale 1 (event_file.h:460-515) of events at (pr_x, pr_y): truncation, the window test
    against (res - 1), saturating count, no blur at scale 1, brightness 127 / mean of the non-zero pixels in float."""
    x, y = FI.trunc_x86(pr_x), FI.trunc_x86(pr_y)
    ok = (x >= 0) & (x < res_x - 1) & (y >= 0) & (y < res_y - 1)
    cnt = np.zeros((res_x, res_y), dtype=np.int64)
    np.add.at(cnt, (x[ok], y[ok]), 1)
    img = np.minimum(cnt, 255)
    nz = img[img > 0]
    if len(nz) == 0:
        return np.zeros((res_x, res_y), dtype=np.uint8)
    a = np.float32(127.0 / (float(nz.sum()) / len(nz)))
    return np.minimum(np.rint(img.astype(np.float32) * a), 255).astype(np.uint8)


def frame_tiles(held, fr_x, fr_y, res_x, res_y):
    """(left, right): the projection images of the held positions and of the raw ones."""
    return (projection_img1(held["pr_x"], held["pr_y"], res_x, res_y),
            projection_img1(np.asarray(fr_x, dtype=np.float64), np.asarray(fr_y, dtype=np.float64), res_x, res_y))


def uv_bound(dev, host):
    """Largest |dev - host| / |host| over the non-zero host values, and whether every zero is met exactly."""
    dev, host = np.asarray(dev, dtype=np.float64), np.asarray(host, dtype=np.float64)
    zero = host == 0
    rel = np.abs(dev[~zero] - host[~zero]) / np.abs(host[~zero])
    return (float(rel.max()) if rel.size else 0.0), bool((dev[zero] == 0).all())


# ---- the -o table: one short stream on a 64 x 128 sensor and three overlapping slices of it ----
EMIT_SENSOR = (64, 128)


def emit_stream(seed=3, n=700):
    """(ts uint64 non-decreasing, row, col): random events about 30 us apart, with hand-placed same-pixel pairs 99 999 and
    100 000 ns apart (the 0.1 ms reach, either side of it) and same-pixel same-instant twins, inside every slice below."""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(1, 60000, n)).astype(np.int64) + 1_000_000
    row, col = rng.integers(0, EMIT_SENSOR[0], n), rng.integers(0, EMIT_SENSOR[1], n)
    extra = []
    for k in range(20, n - 20, 45):
        d = (99999, 100000, 0)[(k // 45) % 3]                                           # 0: a twin
        extra.append((ts[k] + d, row[k], col[k]))
    e = np.array(extra, dtype=np.int64)
    ts, row, col = np.concatenate([ts, e[:, 0]]), np.concatenate([row, e[:, 1]]), np.concatenate([col, e[:, 2]])
    o = np.argsort(ts, kind="stable")
    return ts[o].astype(np.uint64), row[o].astype(np.int64), col[o].astype(np.int64)


def emit_slices(ts):
    """Three overlapping slices (first, n, start_time, lead): the first leads with the ring's oldest element (arrival 0, in
    no slice), the second starts one past its oldest timestamp (the t == -1 mark), the third runs to the end."""
    N = len(ts)
    a, b = N // 3, (2 * N) // 3
    return [(1, b - 1, int(ts[1]), 1), (a, b - a + 60, int(ts[a]) + 1, 0), (b - 40, N - (b - 40), int(ts[b - 40]), 0)]


def emit_rows(ts, row, col, slices, k, uv, cap):
    """The rows slice k adds to the table, as a dict of t, row, col, u, v: emit_ref.device_rows over slices[:k + 1] less what
    slices[:k] gave; uv = (u, v) of slice k's events in upload order (the lead's flow is zero)."""
    pix = row * EMIT_SENSOR[1] + col
    before = emit_ref.device_rows(ts, pix, slices[:k], cap)
    upto = emit_ref.device_rows(ts, pix, slices[:k + 1], cap)
    assert upto[:len(before)] == before
    g = np.array(upto[len(before):], dtype=np.int64)
    first = slices[k][0]
    inside = g >= first
    u, v = np.zeros(len(g)), np.zeros(len(g))
    u[inside], v[inside] = uv[0][g[inside] - first], uv[1][g[inside] - first]
    return dict(t=ts[g].astype(np.uint64), row=row[g].astype(np.uint16), col=col[g].astype(np.uint16), u=u, v=v)
