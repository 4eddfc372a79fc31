"""The restatement of bf_assign_groups (include/bf_accel.h, "event groups": assignment) in numpy integers: every event goes to
the candidate model under which it lands on the largest pile of OTHER events.

    window   np_ref.window (optimizer_rolling.h:248-283) on the whole sensor widened by `margin` on every side
    pixel    np_ref.warp's arithmetic from the reset state (pr = fr) with set_model's parameters
             (optimizer_rolling.h:289-299) and math.sin / math.cos (libm, as step_ref does for bf_set_model), then the
             truncation and the window test of np_ref.time_img (accel_lib.h:154-158)
    votes    V_k[X, Y]: events inside under k whose prior id is k or -1 (no prior: all); B_k: the s x s box sum of V_k
    score    S_k(i) = B_k[pixel_k(i)] - (1 if i voted under k), 0 outside; best = max_k, the id the smallest k that
             reaches it, -1 when best < min_score

Everything after the pixel is an integer count, a maximum or a smallest index, so the device is held to equality.

`mutate` switches one rule off for the mutation tests: "no_loo" (no leave-one-out), "ties_up" (ties go to the larger k)."""
import math

import numpy as np

import np_ref

F32 = np.float32


def window(scale, sensor_res, margin):
    return np_ref.window([-margin, sensor_res[0] - 1 + margin], [-margin, sensor_res[1] - 1 + margin], scale,
                         sensor_res[0], sensor_res[1])


def warp_of(m):
    """(dnx, dny, cx, cy, div, sin, cos) of set_model's warp_reinit for a model (anything with the model's fields)."""
    g = (lambda k: m[k]) if isinstance(m, dict) else (lambda k: getattr(m, k))
    a = -float(g("total_rot"))
    return (-float(g("total_dx")), -float(g("total_dy")), float(g("cx")), float(g("cy")), float(g("total_div")),
            math.sin(a), math.cos(a))


def pixels(sl, m, w, scale):
    """-> (inside: bool[n], X, Y: int64[n], valid where inside) of every event under model m."""
    dnx, dny, cx, cy, div, s, c = (np.float64(v) for v in warp_of(m))
    fx = np.asarray(sl["fr_x"]).astype(F32).astype(np.float64)   # Event::reset: pr = fr
    fy = np.asarray(sl["fr_y"]).astype(F32).astype(np.float64)
    # event.h:99-110,164-168 as np_ref.warp states them: every operation a separate IEEE operation, in its order
    rx, ry = fx - cx, fy - cy
    qx = c * rx - s * ry
    qy = s * rx + c * ry
    nx = ((-qx) * div + (qx - rx)) + dnx
    ny = ((-qy) * div + (qy - ry)) + dny
    kx = (nx.astype(F32).astype(np.float64) / 127.0).astype(F32)
    ky = (ny.astype(F32).astype(np.float64) / 127.0).astype(F32)
    ft = np.asarray(sl["t"]).astype(F32)
    pr_x = fx - (kx * ft).astype(np.float64) / 10000.0
    pr_y = fy - (ky * ft).astype(np.float64) / 10000.0
    hs = scale // 2
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.trunc(pr_x * scale + int(w["x_shift"]))   # accel_lib.h:154-155 (np_ref.time_img)
        y = np.trunc(pr_y * scale + int(w["y_shift"]))
        # accel_lib.h:157; NaN and anything beyond the int range are rejected there too
        inside = ~((x >= w["wsx"] + hs) | (x < hs) | (y >= w["wsy"] + hs) | (y < hs)) & np.isfinite(x) & np.isfinite(y)
    X = np.where(inside, x, 0).astype(np.int64)
    Y = np.where(inside, y, 0).astype(np.int64)
    return inside, X, Y


def box_sum(V, scale):
    """The reference's splat as a gather: B[x, y] = sum of V over the s x s box about (x, y), zero beyond the plane."""
    hs = scale // 2
    R, C = V.shape
    P = np.zeros((R + 2 * hs, C + 2 * hs), dtype=np.int64)
    P[hs:hs + R, hs:hs + C] = V
    B = np.zeros((R, C), dtype=np.int64)
    for dx in range(scale):
        for dy in range(scale):
            B += P[dx:dx + R, dy:dy + C]
    return B


def assign(sl, models, scale, sensor_res, margin=0, min_score=1, prior=None, mutate=None):
    """-> (gid int32[n], score int32[n], counts int32[K + 1] (last: unassigned), info dict).  prior: None (use_prior = 0) or
    the held ids (-1 .. K-1, upload order)."""
    K = len(models)
    n = len(sl["t"])
    w = window(scale, sensor_res, margin)
    R, C = w["R"], w["C"]
    if n == 0:   # "everything zero"
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(K + 1, np.int32),
                dict(models=0, rows=0, cols=0, assigned=0, unassigned=0, changed=0, max_score=0))
    pri = np.full(n, -1, dtype=np.int64) if prior is None else np.asarray(prior).astype(np.int64)
    S = np.zeros((K, n), dtype=np.int64)
    for k, m in enumerate(models):
        inside, X, Y = pixels(sl, m, w, scale)
        votes = inside & ((pri == k) | (pri == -1))
        V = np.bincount((X * C + Y)[votes], minlength=R * C).reshape(R, C)
        B = box_sum(V, scale) if scale > 1 else V
        loo = 0 if mutate == "no_loo" else votes[inside].astype(np.int64)
        S[k, inside] = B[X[inside], Y[inside]] - loo
    if mutate == "ties_up":
        best_k = K - 1 - np.argmax(S[::-1], axis=0)
    else:
        best_k = np.argmax(S, axis=0)   # (the first maximum: the smallest k)
    best = S.max(axis=0)
    gid = np.where(best >= min_score, best_k, -1).astype(np.int32)
    counts = np.array([int((gid == k).sum()) for k in range(K)] + [int((gid < 0).sum())], dtype=np.int32)
    info = dict(models=K, rows=R, cols=C, assigned=int((gid >= 0).sum()), unassigned=int((gid < 0).sum()),
                changed=int((gid != pri).sum()), max_score=int(best.max()))
    return gid, best.astype(np.int32), counts, info


def model_of_velocity(v):
    """The model whose set_model warp compensates the image velocity v (px / s)."""
    import groups_ref
    import segment_scene
    return groups_ref.warm_from_flow(*segment_scene.flow_of(v))


def rounds(sl, models, scale, sensor_res, n_rounds, margin=0, min_score=1):
    """n_rounds assignments, the first without a prior, the others with the one before: the list of (gid, score, counts, info)."""
    out, prior = [], None
    for _ in range(n_rounds):
        r = assign(sl, models, scale, sensor_res, margin, min_score, prior)
        out.append(r)
        prior = r[0]
    return out


def recall_purity(sc, gid, patch_group=1, background_group=0):
    """(patch events in patch_group / patch events, background events in background_group / background events)."""
    p = sc["is_patch"]
    return float((gid[p] == patch_group).mean()), float((gid[~p] == background_group).mean())


def alternate(sc, models, scale, sensor_res, guard_res, min_events, hard_cap, rounds_per_fit=2, max_alternations=5, margin=0,
              min_score=1):
    """bf::MotionAssigner::alternate on the restatement and the CPU oracle.  Per alternation: rounds_per_fit assignments (the
    very first without a prior, every other with the one before), then -- unless this is not the first alternation and its
    first round changed no id: the models are the fit of exactly this membership -- a refit of every group through
    groups_ref.solve, warm from its current model; a group whose rc is not 0 (a guard skipped it) keeps its model.
    -> (models, gid, records); a record: dict(changed, counts, iterations, flows) with changed the first round's, counts the
    last round's, iterations per group (None: no refit) and flows the groups' median (u, v) after the refit."""
    import groups_ref as gr
    models = [gr.as_model(m) for m in models]
    K = len(models)
    prior, records, gid = None, [], None
    for a in range(max_alternations):
        first_changed = None
        for _ in range(rounds_per_fit):
            gid, _, counts, info = assign(sc, models, scale, sensor_res, margin, min_score, prior)
            if first_changed is None:
                first_changed = info["changed"]
            prior = gid
        rec = dict(changed=first_changed, counts=counts.tolist(), iterations=None, flows=None)
        records.append(rec)
        if a > 0 and first_changed == 0:
            break
        res, _, _, u, v = gr.solve(sc, gid, K, scale, sensor_res, guard_res, min_events, warm=list(models), hard_cap=hard_cap)
        for g, r in enumerate(res):
            if r.rc == 0:
                models[g] = r.model
        rec["iterations"] = [r.iterations for r in res]
        rec["rc"] = [r.rc for r in res]
        rec["flows"] = [gr.median_flow(u, v, r.idx) if r.events else (0.0, 0.0) for r in res]
    return models, gid, records
