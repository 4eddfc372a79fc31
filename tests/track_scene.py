"""The two-motion scene of tests/segment_scene.py continued over three consecutive slices: the same scene points (background
and patch), the same two velocities, three times the events over three times the duration, cut by time into slices of
segment_scene.DURATION_S with slice-local times.  Slice 0 is not segment_scene.make()'s own event set (the times are drawn over
the whole stretch), but the same scene in the same place.

Seeded and counter-based through synth.splitmix64: the same slices everywhere."""
import numpy as np

import segment_scene as scene
from better_flow_amd import synth

H, W = scene.H, scene.W
N_SLICES = 3
STEP_NS = int(round(scene.DURATION_S * 1e9))   # the time origin of slice s + 1 minus that of slice s


def _uniform(seed, stream, n):
    return (synth.splitmix64(seed, stream, n) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def _moving_points(seed, streams, p_row, p_col, n_events, velocity):
    """n_events events of the given scene points over the whole stretch: (row, col, t_ns) of those still on the sensor."""
    t_ns = np.floor(_uniform(seed, streams[0], n_events) * (N_SLICES * STEP_NS)).astype(np.int64)
    pick = (synth.splitmix64(seed, streams[1], n_events) % np.uint64(len(p_row))).astype(np.int64)
    ts = t_ns.astype(np.float64) * 1e-9
    row = np.floor(p_row[pick] + velocity[0] * ts).astype(np.int64)
    col = np.floor(p_col[pick] + velocity[1] * ts).astype(np.int64)
    keep = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    return row[keep], col[keep], t_ns[keep]


def make(seed=11):
    """-> (slices, step_ns): slices a list of N_SLICES dicts(fr_x, fr_y: int32; t: int64 ns from the slice's origin; is_patch:
    bool; t0_ns: the slice's origin), each time-sorted (stable: background first on ties)."""
    # the background's points as synth.make_slice places them for segment_scene.make (streams 1, 2), the patch's as segment_scene's
    n_pts = max(1, scene.N_BACKGROUND // 16)
    b_row = 10.0 + _uniform(seed, 1, n_pts) * (H - 20.0)
    b_col = 10.0 + _uniform(seed, 2, n_pts) * (W - 20.0)
    p_row = scene.PATCH_ROWS[0] + _uniform(seed, 11, scene.N_PATCH_POINTS) * (scene.PATCH_ROWS[1] - scene.PATCH_ROWS[0])
    p_col = scene.PATCH_COLS[0] + _uniform(seed, 12, scene.N_PATCH_POINTS) * (scene.PATCH_COLS[1] - scene.PATCH_COLS[0])
    bg = _moving_points(seed, (23, 24), b_row, b_col, N_SLICES * scene.N_BACKGROUND, scene.V_BACKGROUND)
    pa = _moving_points(seed, (33, 34), p_row, p_col, N_SLICES * scene.N_PATCH_POINTS * scene.EVENTS_PER_PATCH_POINT, scene.V_PATCH)
    row, col, t = (np.concatenate([a, b]) for a, b in zip(bg, pa))
    is_patch = np.concatenate([np.zeros(len(bg[2]), dtype=bool), np.ones(len(pa[2]), dtype=bool)])
    order = np.argsort(t, kind="stable")
    row, col, t, is_patch = row[order], col[order], t[order], is_patch[order]
    slices = []
    for s in range(N_SLICES):
        t0 = s * STEP_NS
        m = (t >= t0) & (t < t0 + STEP_NS)
        slices.append(dict(fr_x=row[m].astype(np.int32), fr_y=col[m].astype(np.int32), t=t[m] - t0, is_patch=is_patch[m], t0_ns=t0))
    return slices, STEP_NS
