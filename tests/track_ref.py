"""The restatement of bf_track_keep / bf_track_overlap (include/bf_accel.h, "event groups: tracks") and of
bf::ObjectTracker::match in numpy integers, built from assign_ref.pixels and project_groups_ref.project.

    keep      project_groups_ref.project's label: the owner plane of a slice's grouping under its models
    pixel     assign_ref.pixels on a slice whose t is t + dt_ns as 64-bit integers; assign_ref.pixels then takes float32 of it,
              which numpy rounds to nearest, ties to even: the time operand of the definition
    overlap   overlap[k, j] = the events with id k that are inside and land on a pixel whose kept label is j; column Kp: on a
              pixel whose kept label is -1; inside[k] the row's sum; outside, unassigned as bf_project_groups counts them
    match     repeatedly the largest overlap[k, j] among unmatched k and unmatched j (ties: the smallest k, then the smallest j),
              accepted while it is > 0 and overlap * den >= inside[k] * num

Everything after the pixel is an integer count, so the device is held to equality.

`mutate` switches one rule off for the mutation tests: "no_dt" (dt ignored), "ties_up" (match ties go to the larger index),
"trunc_time" (the time operand rounded toward zero instead of to nearest)."""
import numpy as np

import assign_ref as ar
import project_groups_ref as pr

INFO_FIELDS = ("models", "kept_models", "rows", "cols", "unassigned", "outside")


def keep(sl, ids, models, scale, sensor_res, margin=0):
    """-> (plane int32[R, C], info dict, Kp): what bf_track_keep keeps of the grouping `ids` under `models`."""
    r = pr.project(sl, ids, models, scale, sensor_res, margin, gain=1)
    K = len(models)
    if len(sl["t"]) == 0:
        info = dict.fromkeys(INFO_FIELDS, 0)
    else:
        info = dict(models=K, kept_models=K, rows=r["info"]["rows"], cols=r["info"]["cols"], unassigned=r["info"]["unassigned"],
                    outside=r["info"]["outside"])
    return r["label"], info, K


def pixels(sl, m, w, scale, dt_ns=0, mutate=None):
    """assign_ref.pixels with every event's time operand the float32 nearest to the 64-bit t + dt_ns."""
    dt = 0 if mutate == "no_dt" else int(dt_ns)
    t = np.asarray(sl["t"]).astype(np.int64) + np.int64(dt)
    if mutate == "trunc_time":   # the float32 toward zero instead of the nearest
        f = t.astype(np.float32)
        over = np.abs(f.astype(np.float64)) > np.abs(t.astype(np.float64))   # (exact: |t| < 2^53)
        t = np.where(over, np.nextafter(f, np.float32(0)), f)
    return ar.pixels(dict(fr_x=sl["fr_x"], fr_y=sl["fr_y"], t=t), m, w, scale)


def overlap(sl, ids, models, plane, Kp, dt_ns, scale, sensor_res, margin=0, mutate=None):
    """-> (overlap int32[K, Kp + 1], inside int32[K], info dict).  ids: the new slice's grouping (-1 .. K-1, upload order);
    plane: the kept owner plane (labels -1 .. Kp-1)."""
    K = len(models)
    n = len(sl["t"])
    w = ar.window(scale, sensor_res, margin)
    ids = np.asarray(ids).astype(np.int64)
    assert ids.shape == (n,) and plane.shape == (w["R"], w["C"])
    table = np.zeros((K, Kp + 1), dtype=np.int64)
    outside = 0
    for k, m in enumerate(models):
        mine = ids == k
        if not mine.any():
            continue
        sub = dict(fr_x=np.asarray(sl["fr_x"])[mine], fr_y=np.asarray(sl["fr_y"])[mine], t=np.asarray(sl["t"])[mine])
        ins, X, Y = pixels(sub, m, w, scale, dt_ns, mutate)
        lab = plane[X[ins], Y[ins]].astype(np.int64)
        table[k] = np.bincount(np.where(lab < 0, Kp, lab), minlength=Kp + 1)
        outside += int(mine.sum()) - int(ins.sum())
    info = dict(models=K, kept_models=Kp, rows=w["R"], cols=w["C"], unassigned=int((ids == -1).sum()), outside=outside)
    if n == 0:   # "every output zero"
        info = dict.fromkeys(INFO_FIELDS, 0)
    return table.astype(np.int32), table.sum(axis=1).astype(np.int32), info


def match(table, inside, num=1, den=2, mutate=None):
    """bf::ObjectTracker::match -> a list of K entries: the kept group j that group k continues, or -1.  table: [K, Kp + 1]."""
    table = np.asarray(table).astype(np.int64)
    K, Kp = table.shape[0], table.shape[1] - 1
    out = [-1] * K
    taken = set()
    while True:
        best = None
        for k in range(K):
            if out[k] >= 0:
                continue
            for j in range(Kp):
                if j in taken:
                    continue
                v = int(table[k, j])
                if best is None or v > best[0] or (mutate == "ties_up" and v == best[0]):
                    best = (v, k, j)
        if best is None:
            break
        v, k, j = best
        if not (v > 0 and v * den >= int(inside[k]) * num):
            break
        out[k] = j
        taken.add(j)
    return out


def track_ids(matched, prev_ids, next_id):
    """The track ids after match(): a matched group inherits its track's id, an unmatched one gets next_id++.
    -> (ids per group, ended ids of prev_ids that nobody continues, next_id)."""
    ids = []
    for j in matched:
        if j >= 0:
            ids.append(prev_ids[j])
        else:
            ids.append(next_id)
            next_id += 1
    ended = [t for j, t in enumerate(prev_ids) if j not in matched]
    return ids, ended, next_id
