"""The restatement of bf_run_groups (include/bf_accel.h, "event groups") on the CPU oracle: per group an oracle Cloud of the
group's events in upload order, set_cloud, optional set_model, run, compute_uv, scattered back to upload order.  Events with
id -1 read zeros.  The window (box, rows, cols) is the oracle's own."""
import numpy as np

import oracle
import segment_scene as scene


class GroupResult:
    """rc, iterations, model (oracle.Model), window (oracle.Window), events, idx (upload indices) of one group."""

    def __init__(self, rc, iterations, model, window, idx):
        self.rc, self.iterations, self.model, self.window, self.idx = rc, iterations, model, window, idx
        self.events = len(idx)

    @property
    def box(self):
        """What bf_group_info holds: (events, row_min, row_max, col_min, col_max, rows, cols)."""
        w = self.window
        return (self.events, w.x_min, w.x_max, w.y_min, w.y_max, w.scale_img_x, w.scale_img_y)

    @property
    def pixels(self):
        return self.window.scale_img_x * self.window.scale_img_y


def as_model(m):
    """An oracle.Model from anything with the model's fields (an accel.Model, an oracle.Model, a dict)."""
    out = oracle.Model()
    for k, _ in oracle.Model._fields_:
        setattr(out, k, m[k] if isinstance(m, dict) else getattr(m, k))
    return out


def warm_from_flow(nx, ny):
    """The model whose set_model warp compensates the flow (nx, ny): total_dx, total_dy = -(nx, ny)."""
    m = oracle.Model()
    m.total_dx, m.total_dy = -nx, -ny
    return m


def solve(sl, gid, K, scale, sensor_res, guard_res, min_events, warm=None, max_iter=-1, hard_cap=20000, reverse=False,
          no_run=()):
    """-> (groups: [GroupResult] * K, nx, ny, u, v in upload order).  warm: None, one model, or K models.  reverse: every
    group's events in reversed upload order (the order-stability check).  no_run: groups that stop after set_model (what the
    device does with a window that does not fit its LDS)."""
    gid = np.asarray(gid)
    n = len(gid)
    nx, ny, u, v = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    out = []
    for g in range(K):
        idx = np.flatnonzero(gid == g)
        if reverse:
            idx = idx[::-1].copy()
        oc = oracle.Cloud(sl["fr_x"][idx], sl["fr_y"][idx], sl["t"][idx])
        ow = oc.set_cloud(scale, sensor_res[0], sensor_res[1])
        w = None if warm is None else (warm[g] if isinstance(warm, (list, tuple)) else warm)
        m = oracle.Model()
        if w is not None:
            m = as_model(w)
            if len(idx):
                m = oc.set_model(m)
        if g in no_run or len(idx) == 0:
            rc, it = (1, 0)
        else:
            rc, loop, _ = oc.run(ow, m, max_iter=max_iter, res_x=guard_res[0], res_y=guard_res[1], min_events=min_events,
                                 hard_cap=hard_cap)
            it = int(loop.itercount)
        if len(idx):
            gu, gv = oc.compute_uv()
            nx[idx], ny[idx], u[idx], v[idx] = oc.nx, oc.ny, gu, gv
        out.append(GroupResult(rc, it, m, ow, idx))
    return out, nx, ny, u, v


def scene_groups(sc):
    """The four groups of the scene: 0 the patch, 1 .. 3 three boxes of background events; the rest -1."""
    x, y, p = sc["fr_x"], sc["fr_y"], sc["is_patch"]
    gid = np.full(len(x), -1, dtype=np.int32)
    gid[p] = 0
    gid[~p & (x >= 60) & (y < 40)] = 1
    gid[~p & (x < 28) & (y >= 66) & (y < 98)] = 2
    gid[~p & (x < 30) & (y < 32)] = 3
    return gid


def background_model():
    nx, ny = scene.flow_of(scene.V_BACKGROUND)
    return warm_from_flow(nx, ny)


def median_flow(u, v, idx):
    return float(np.median(u[idx])), float(np.median(v[idx]))
