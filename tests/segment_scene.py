"""The two-motion scene of the segmentation tests: a background of scene points at one image velocity (synth.make_slice) and
a small dense patch of points at another, in one time-sorted slice.  Compensating the slice with the BACKGROUND's flow leaves
every background point on one pixel (mean timestamp ~ half the slice) and smears the patch along the relative velocity: the
pixels ahead of the patch collect only late events, and those are what the threshold keeps.

Seeded and counter-based like synth itself: the same scene everywhere."""
import numpy as np

from better_flow_amd import synth

H, W = 90, 120
DURATION_S = 0.030
V_BACKGROUND = (-50.0, 100.0)      # (row, column) px / s
V_PATCH = (400.0, -300.0)
PATCH_ROWS = (30, 44)              # the patch's points start inside [r0, r1) x [c0, c1)
PATCH_COLS = (50, 64)
N_BACKGROUND, N_PATCH_POINTS, EVENTS_PER_PATCH_POINT = 6000, 400, 24

# the options the CPU test tuned on the restatement until it gave exactly one component (tests/test_segment_cpu.py)
SCALE = 1
OPTS = dict(above_s=0.35 * DURATION_S, below_s=-1.0, min_count=3, connectivity=8, min_pixels=20)


def flow_of(velocity):
    """(nx, ny) of Event::apply_project for an image velocity in px / s: pr = fr - (n / 127) * t_ns / 10000."""
    return velocity[0] * 1.27e-3, velocity[1] * 1.27e-3


def make(seed=11):
    """dict(fr_x, fr_y, t, is_patch): int32 rows / columns, int64 ns, bool; time-sorted (stable: background first on ties)."""
    bg = synth.make_slice(N_BACKGROUND, H, W, DURATION_S, seed=seed, velocity=V_BACKGROUND)
    n = N_PATCH_POINTS * EVENTS_PER_PATCH_POINT
    u = lambda stream, m: (synth.splitmix64(seed, stream, m) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    p_row = PATCH_ROWS[0] + u(11, N_PATCH_POINTS) * (PATCH_ROWS[1] - PATCH_ROWS[0])
    p_col = PATCH_COLS[0] + u(12, N_PATCH_POINTS) * (PATCH_COLS[1] - PATCH_COLS[0])
    t_ns = np.floor(u(13, n) * (DURATION_S * 1e9)).astype(np.int64)
    pick = (synth.splitmix64(seed, 14, n) % np.uint64(N_PATCH_POINTS)).astype(np.int64)
    ts = t_ns.astype(np.float64) * 1e-9
    row = np.floor(p_row[pick] + V_PATCH[0] * ts).astype(np.int64)
    col = np.floor(p_col[pick] + V_PATCH[1] * ts).astype(np.int64)
    keep = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    fr_x = np.concatenate([bg["fr_x"].astype(np.int64), row[keep]])
    fr_y = np.concatenate([bg["fr_y"].astype(np.int64), col[keep]])
    t = np.concatenate([bg["t"], t_ns[keep]])
    is_patch = np.concatenate([np.zeros(len(bg["t"]), dtype=bool), np.ones(int(keep.sum()), dtype=bool)])
    order = np.argsort(t, kind="stable")
    return dict(fr_x=fr_x[order].astype(np.int32), fr_y=fr_y[order].astype(np.int32), t=t[order], is_patch=is_patch[order])


def swept_box(window, dilate):
    """The box the patch sweeps in the COMPENSATED frame -- the frame the time image is in: a patch point at p0 lands on
    p0 + (V_PATCH - V_BACKGROUND) t --, in window pixels (position * scale + shift), dilated by `dilate` pixels:
    (row_min, row_max, col_min, col_max)."""
    s = int(window.scale)
    out = []
    for (lo, hi), vp, vb, sh in ((PATCH_ROWS, V_PATCH[0], V_BACKGROUND[0], int(window.x_shift)),
                                 (PATCH_COLS, V_PATCH[1], V_BACKGROUND[1], int(window.y_shift))):
        d = (vp - vb) * DURATION_S
        a, b = lo + min(0.0, d), hi + max(0.0, d)
        out += [int(np.floor(a * s + sh)) - dilate, int(np.ceil(b * s + sh)) + dilate]
    return tuple(out)
