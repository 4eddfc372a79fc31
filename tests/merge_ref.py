"""The restatement of bf_merge_scores (include/bf_accel.h, "event groups: merge gains") in numpy integers, and of the policy
and loop of bf::ObjectMerger (host/better_flow/object_merge.h) on the restatements of the assignment and the grouped solve.

    window, pixel   assign_ref.window / assign_ref.pixels: exactly bf_assign_groups'
    trial    T[b][a]: the s x s box sum (assign_ref.box_sum) of the events with id b that are inside under MODEL a
    base     B_b = T[b][b]; N = sum_k B_k; S = sum N^2
    gain     gain[b][a] = sum_p T[b][a] (2 (N - B_b) + T[b][a])  (mod 2^64)
    inside   inside[b][a] = events of b inside under a; events[b]
    info     models, rows, cols, unassigned, passes, sum = sum N, sum_sq = S

Everything after the pixel is an integer count or a sum, so the device is held to equality.

    pick     candidates (b, a), b != a, events[b] >= 1, gain[b][b] > 0, and events[a] > events[b] or (equal and a < b); the
             largest gain[b][a] / gain[b][b] as an exact fraction, among equals the smallest b, then the smallest a; accepted
             when gain[b][a] den >= gain[b][b] num
    reduce   dissolve empty and too small groups, score, pick, merge, one alternation after every change, until nothing is
             picked or one group is left

`mutate` switches one rule off for the mutation tests: in scores "count_unassigned" (an event with id -1 is put on plane 0
instead of on none) and "no_cross" (the term 2 (N - B_b) is left out); in pick "no_size_rule" (a group may dissolve into a smaller
one) and "ties_up" (among equal ratios the larger b wins)."""
from fractions import Fraction

import numpy as np

import assign_ref as ar

INFO_FIELDS = ("models", "rows", "cols", "unassigned", "passes", "sum", "sum_sq")
M64 = (1 << 64) - 1
MAX_WORDS = 1 << 27


def passes_of(K, R, C, targets_per_pass=0):
    """info.passes: ceil(K / A), A = min(K, targets_per_pass or K, floor(2^27 / (K R C)))."""
    A = min(K, targets_per_pass or K, MAX_WORDS // (K * R * C))
    return -(-K // A)


def scores(sl, ids, models, scale, sensor_res, margin=0, targets_per_pass=0, mutate=None):
    """-> dict(gain uint64[K, K], inside int32[K, K], events int32[K], info dict), the matrices indexed [b, a].  ids: the held
    grouping, -1 .. K-1 in upload order."""
    K = len(models)
    n = len(sl["t"])
    w = ar.window(scale, sensor_res, margin)
    R, C = w["R"], w["C"]
    ids = np.asarray(ids).astype(np.int64)
    assert ids.shape == (n,)
    gain = np.zeros((K, K), dtype=np.uint64)
    inside = np.zeros((K, K), dtype=np.int32)
    events = np.zeros(K, dtype=np.int32)
    if n == 0:   # "everything zero"
        return dict(gain=gain, inside=inside, events=events, info=dict.fromkeys(INFO_FIELDS, 0))
    subs = []
    for b in range(K):
        mine = ids == b
        if mutate == "count_unassigned" and b == 0:
            mine = mine | (ids == -1)
        events[b] = int(mine.sum())
        subs.append(dict(fr_x=np.asarray(sl["fr_x"])[mine], fr_y=np.asarray(sl["fr_y"])[mine], t=np.asarray(sl["t"])[mine]))

    def trial(b, a):
        if not events[b]:
            return 0, np.zeros((R, C), dtype=np.int64)
        ins, X, Y = ar.pixels(subs[b], models[a], w, scale)
        V = np.bincount((X * C + Y)[ins], minlength=R * C).reshape(R, C)
        return int(ins.sum()), (ar.box_sum(V, scale) if scale > 1 else V)

    B = [trial(b, b)[1] for b in range(K)]
    N = np.sum(B, axis=0).astype(np.uint64)
    for b in range(K):
        rest = N - B[b].astype(np.uint64)
        for a in range(K):
            inside[b, a], T = trial(b, a)
            T = T.astype(np.uint64)
            cross = np.uint64(0) if mutate == "no_cross" else np.uint64(2) * rest
            gain[b, a] = (T * (cross + T)).sum(dtype=np.uint64)   # (uint64 array arithmetic wraps, which is the definition)
    unassigned = 0 if mutate == "count_unassigned" else int((ids == -1).sum())
    info = dict(models=K, rows=R, cols=C, unassigned=unassigned, passes=passes_of(K, R, C, targets_per_pass),
                sum=int(N.sum(dtype=np.uint64)), sum_sq=int((N * N).sum(dtype=np.uint64)))
    return dict(gain=gain, inside=inside, events=events, info=info)


def pick(gain, events, num, den, mutate=None):
    """-> (b, a, accepted) of the best candidate, or None when there is none.  gain: [K, K] of integers, events: [K]."""
    K = len(events)
    g = [[int(gain[b][a]) for a in range(K)] for b in range(K)]
    ev = [int(e) for e in events]
    best = None
    for b in range(K):
        if ev[b] < 1 or g[b][b] <= 0:
            continue
        for a in range(K):
            if a == b:
                continue
            if mutate != "no_size_rule" and not (ev[a] > ev[b] or (ev[a] == ev[b] and a < b)):
                continue
            ratio = Fraction(g[b][a], g[b][b])
            if best is None or ratio > best[0] or (mutate == "ties_up" and ratio == best[0] and b > best[1]):
                best = (ratio, b, a)
    if best is None:
        return None
    _, b, a = best
    return b, a, g[b][a] * int(den) >= g[b][b] * int(num)


def ratios(gain):
    """gain[b][a] / gain[b][b] as floats, for reading (nan where gain[b][b] == 0)."""
    g = np.asarray(gain).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return g / np.diag(g)[:, None]


def compact(ids, models, drop):
    """The grouping without the groups in `drop` (their events -> -1), the others renumbered in order."""
    keep = [k for k in range(len(models)) if k not in drop]
    new = np.full(len(models) + 1, -1, dtype=np.int64)   # (the last word: id -1)
    for j, k in enumerate(keep):
        new[k] = j
    return new[np.asarray(ids)].astype(np.int32), [models[k] for k in keep]


def one_alternation(sc, models, ids, scale, sensor_res, guard_res, min_events, hard_cap, rounds_per_fit, margin, min_score):
    """rounds_per_fit assignments with the current ids as the prior, then one grouped refit, warm from the current models; a
    group whose rc is not 0 keeps its model (assign_ref.alternate's rule)."""
    import groups_ref as gr
    gid = np.asarray(ids).astype(np.int32)
    for _ in range(rounds_per_fit):
        gid = ar.assign(sc, models, scale, sensor_res, margin, min_score, gid)[0]
    res, _, _, u, v = gr.solve(sc, gid, len(models), scale, sensor_res, guard_res, min_events, warm=list(models), hard_cap=hard_cap)
    models = [r.model if r.rc == 0 else m for r, m in zip(res, models)]
    return models, gid


def reduce(sc, models, ids, scale, sensor_res, guard_res, min_events, hard_cap, num, den, dissolve_below=0, max_steps=64,
           rounds_per_fit=2, margin=0, min_score=1, alternation=None, score=None):
    """bf::ObjectMerger::reduce on the restatements.  `alternation(models, ids) -> (models, ids)` and `score(ids, models) ->
    scores dict` default to the restatements (a device test passes the device's).
    -> (models, ids, steps, last scores dict or None); a step: dict(kind, b, a, gain_ba, gain_bb, events_b, K_after)."""
    import groups_ref as gr
    models = [gr.as_model(m) for m in models]
    ids = np.asarray(ids).astype(np.int32)
    if alternation is None:
        alternation = lambda ms, g: one_alternation(sc, ms, g, scale, sensor_res, guard_res, min_events, hard_cap, rounds_per_fit,
                                                    margin, min_score)
    if score is None:
        score = lambda g, ms: scores(sc, g, ms, scale, sensor_res, margin)
    steps, last = [], None
    for _ in range(max_steps):
        K = len(models)
        counts = np.bincount(ids[ids >= 0], minlength=K)
        drop = [k for k in range(K) if counts[k] == 0 or counts[k] < dissolve_below]
        if drop:
            for j, k in enumerate(drop):
                steps.append(dict(kind="dissolve", b=k, a=-1, gain_ba=0, gain_bb=0, events_b=int(counts[k]), K_after=K - 1 - j))
            ids, models = compact(ids, models, drop)
            if not models:
                return models, ids, steps, None
            models, ids = alternation(models, ids)
            continue   # (the alternation may have emptied a group)
        last = score(ids, models)
        p = pick(last["gain"], last["events"], num, den)
        if K == 1 or p is None or not p[2]:
            break
        b, a = p[0], p[1]
        steps.append(dict(kind="merge", b=b, a=a, gain_ba=int(last["gain"][b][a]), gain_bb=int(last["gain"][b][b]),
                          events_b=int(last["events"][b]), K_after=K - 1))
        ids = ids.copy()
        ids[ids == b] = a
        ids, models = compact(ids, models, [b])
        models, ids = alternation(models, ids)
        last = None
    if last is None and models:   # (max_steps ran out behind a change)
        last = score(ids, models)
    return models, ids, steps, last
