"""The inputs of tests/test_tile_variants_cpu.py and tests/test_gpu_tile_variants.py: one row per compiled instantiation of the
tile-grid optimizers (BASELINE config 4) and per grid size at which the tile sort takes another path.

bf_run_tiles / bf_run_tiles_many pick k_tile_optimizer<256, HS> by scale / 2: HS = 0, 1, 2 for the scales 1, 3, 5 (unrolled box sum),
HS = -1 for 7 and 9 (run-time bounds).  A tile keeps 4096 events in registers and streams the rest; k_tile_scan gives each of its
1024 threads ceil(tiles / 1024) tiles; the sort's LDS histograms grow with the tile count up to 16384 tiles.  bf_local_run_tiles
picks k_local_tile_optimizer<scale / 2>; scale 7 is the 7-tap Gaussian.  Every slice is synth.make_slice(n, H, W, duration, seed,
velocity); the CPU file shows on the oracle alone that each row is what this table says it is.
"""
import numpy as np

from better_flow_amd import synth

LDS_PLANE_BYTES = 156 * 1024    # bf_tiles_abi.cpp, tiles_prepare: max_px * 16 must fit
TILE_REGISTER_EVENTS = 4096     # bf_tiles.hip: kTileUR * THREADS
LOCAL_REGISTER_EVENTS = 2048    # bf_local.hip: the window optimizer's register file

# id -> (n, H, W, scale, grid rows, grid columns, min_events, seed, velocity, max_iter, hard_iter_cap)
ROLLING = {
    "s1": (60000, 128, 160, 1, 8, 8, 200, 41, (-60.0, 110.0), -1, 5000),         # HS = 0; loops up to ~2500 iterations
    "s5": (60000, 128, 160, 5, 8, 8, 200, 41, (-60.0, 110.0), -1, 5000),         # HS = 2; max_px 9900: the fullest LDS layout accepted
    "s7": (60000, 80, 96, 7, 8, 8, 200, 41, (-60.0, 110.0), -1, 5000),           # HS = -1; tiles without events
    "s9": (60000, 64, 80, 9, 8, 8, 200, 44, (-60.0, 110.0), -1, 5000),           # HS = -1 at the largest scale
    "stream": (400000, 128, 160, 3, 8, 8, 200, 41, (-60.0, 110.0), 30, 5000),    # tiles on both sides of the 4096-event register file
    "g1600": (300000, 240, 320, 3, 40, 40, 32, 5, None, 5, 5000),                # 1600 tiles: two per thread of k_tile_scan
    "g16384": (1000000, 512, 512, 3, 128, 128, 32, 6, None, 3, 5000),            # the largest grid accepted; 128 KiB histogram
}
ROLLING_DURATION = 0.020
# lower bounds on the number of tiles the oracle optimises (rc 0); "stream" runs all 64
MIN_RAN = {"s1": 60, "s5": 60, "s7": 40, "s9": 38, "stream": 64, "g1600": 1400, "g16384": 14000}
SCALE_ROWS = ("s1", "s5", "s7", "s9")

# id -> (n, H, W, scale, grid rows, grid columns, wsz, seed)
LOCAL = {
    "l7a": (60000, 180, 240, 7, 6, 6, 20, 9),    # HS = 3; 147 x 147 window; tiles on both sides of the 2048-event register file
    "l7b": (30000, 90, 120, 7, 5, 7, 12, 9),     # HS = 3; a non-square grid that does not divide the sensor
}
LOCAL_DURATION = 0.030
LOCAL_MAX_EVALUATIONS = 4000


class Row:
    """One rolling row: the slice, its events by tile, and the oracle of one tile."""

    def __init__(self, rid, seed_offset=0):
        (self.n, self.H, self.W, self.scale, self.gr, self.gc, self.min_events, seed, velocity, self.max_iter,
         self.hard_cap) = ROLLING[rid]
        self.id = rid
        self.sl = synth.make_slice(self.n, self.H, self.W, ROLLING_DURATION, seed=seed + seed_offset, velocity=velocity)
        self.guard = (max(1, self.H // self.gr), max(1, self.W // self.gc))
        self.nt = self.gr * self.gc
        self.order, self.bounds = tile_order(self.sl, self.H, self.W, self.gr, self.gc)

    def sel(self, k):
        """Indices of tile k's events, in upload order."""
        return self.order[self.bounds[k]:self.bounds[k + 1]]

    def max_px(self):
        return max_px(self.H, self.W, self.scale, self.gr, self.gc)

    def oracle(self, oracle_lib, idx, max_iter=None):
        """OptimizerRolling on the events `idx` as a tile of this row -> (rc, iterations, u, v, model)."""
        sl = self.sl
        oc = oracle_lib.Cloud(sl["fr_x"][idx], sl["fr_y"][idx], sl["t"][idx])
        ow = oc.set_cloud(self.scale, self.H, self.W)
        om = oracle_lib.Model()
        rc, loop, _ = oc.run(ow, om, max_iter=self.max_iter if max_iter is None else max_iter, res_x=self.guard[0],
                             res_y=self.guard[1], min_events=self.min_events, hard_cap=self.hard_cap)
        u, v = oc.compute_uv()
        return rc, int(loop.itercount), u, v, om


def order_deviation(fwd, rev):
    """How much of a tile's answer the order of its events decides, from the reference alone: `fwd` the oracle's result on the
    tile's events in upload order, `rev` on the reversed order -> (agree, du, dv), du = max |u_fwd - u_rev| per event and dv
    likewise; agree: both ran, iteration counts within +-1, flow within 1e-4 relative / 0.02 px/s (_flow_close's bar)."""
    (rc, it, u, v, _), (rrc, rit, ru, rv, _) = fwd, rev
    if rc != 0 or rrc != 0:
        return rc == rrc, 0.0, 0.0
    ru, rv = ru[::-1], rv[::-1]
    du, dv = float(np.abs(u - ru).max()), float(np.abs(v - rv).max())
    close = bool(np.all(np.abs(u - ru) <= np.maximum(1e-4 * np.abs(u), 0.02)) and
                 np.all(np.abs(v - rv) <= np.maximum(1e-4 * np.abs(v), 0.02)))
    return abs(it - rit) <= 1 and close, du, dv


def agrees(oracle_lib, row, idx, gu, gv, git, widen=(0.0, 0.0), fwd=None):
    """test_gpu_config4.agrees for a tile of `row`: the GPU's flow gu, gv and iteration count git on the events `idx`
    against the oracle on them in that order (`fwd`: that run, if the caller has it) -> (ok, oracle iterations, worst deviation).
    Iteration count within +-1; per-event flow within 1e-4 relative / 0.02 px/s, widened when the counts differ by one by the size
    of the oracle's own last step, and by `widen` = (du, dv), the tile's order_deviation: both come from the reference alone."""
    rc, it, u, v, _ = fwd if fwd is not None else row.oracle(oracle_lib, idx)
    if rc != 0 or abs(git - it) > 1:
        return False, it, np.inf
    tol_u, tol_v = np.maximum(1e-4 * np.abs(u), 0.02) + widen[0], np.maximum(1e-4 * np.abs(v), 0.02) + widen[1]
    if git != it and it >= 3:
        _, it1, u1, v1, _ = row.oracle(oracle_lib, idx, max_iter=it - 2)   # max_iter = K runs K + 1 iterations
        assert it1 == it - 1
        tol_u, tol_v = tol_u + np.abs(u - u1).max(), tol_v + np.abs(v - v1).max()
    dev = max(np.abs(gu - u).max(), np.abs(gv - v).max())
    return bool(np.all(np.abs(gu - u) <= tol_u) and np.all(np.abs(gv - v) <= tol_v)), it, dev


def tile_ids(sl, H, W, gr, gc):
    tr = np.minimum(sl["fr_x"].astype(np.int64) * gr // H, gr - 1)
    tc = np.minimum(sl["fr_y"].astype(np.int64) * gc // W, gc - 1)
    return tr * gc + tc


def tile_order(sl, H, W, gr, gc):
    """(order, bounds): order[bounds[k]:bounds[k + 1]] are the events of tile k in upload order."""
    tid = tile_ids(sl, H, W, gr, gc)
    order = np.argsort(tid, kind="stable")
    return order, np.searchsorted(tid[order], np.arange(gr * gc + 1))


def max_px(H, W, s, gr, gc):
    """The largest window a tile can have, in scaled pixels (bf_tiles_abi.cpp, tiles_prepare)."""
    tr, tc = -(-H // gr) + 1, -(-W // gc) + 1
    return (s * tr + s) * (s * tc + s)


def local_slice(rid):
    n, H, W, s, gr, gc, wsz, seed = LOCAL[rid]
    return synth.make_slice(n, H, W, LOCAL_DURATION, seed=seed)


def local_oracle(oracle_lib, rid, sl, idx, k):
    """OptimizerLocal on the events `idx` of window k (centre = middle of the tile, t = 0) -> (rc, state)."""
    from test_gpu_config4 import _tile_bounds
    n, H, W, s, gr, gc, wsz, seed = LOCAL[rid]
    guard = (max(1, H // gr), max(1, W // gc))
    xl, xh = _tile_bounds(H, gr, k // gc)
    yl, yh = _tile_bounds(W, gc, k % gc)
    oc = oracle_lib.Cloud(sl["fr_x"][idx], sl["fr_y"][idx], sl["t"][idx])
    ow = oc.local_window(s, center=((xl + xh) // 2, (yl + yh) // 2, 0), wsz=wsz)
    rc, st, _ = oc.local_run(ow, res_x=guard[0], res_y=guard[1], max_evaluations=LOCAL_MAX_EVALUATIONS)
    return rc, st
