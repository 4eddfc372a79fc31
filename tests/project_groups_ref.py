"""The restatement of bf_project_groups (include/bf_accel.h, "event groups: projection") in numpy integers: the slice with every
event warped by its OWN group's model, as an image and a score.

    window, pixel   assign_ref.window / assign_ref.pixels: exactly bf_assign_groups'
    planes   V_k[X, Y]: events with id k that are inside under model k; B_k: the s x s box sum of V_k (assign_ref.box_sum)
    pixel    N = sum_k B_k; label = the smallest k with the largest B_k, -1 where N == 0;
             bgr = PALETTE[label % 12] * min(255, B_label * gain) // 255, 0 where the label is -1
    group    events, inside, pixels_hit, pixels_owned, max, sum_sq = sum B_k^2 (mod 2^64)
    info     models, rows, cols, unassigned, outside, pixels, sum, sum_sq = sum N^2 (mod 2^64)

Everything after the pixel is an integer count, a sum, a maximum or a smallest index, so the device is held to equality.

`mutate` switches one rule off for the mutation tests: "ties_up" (ties go to the larger k), "count_unassigned" (an event with id
-1 is put on plane 0 instead of on none), "label_by_total" (the colour's level from N instead of from B_label)."""
import numpy as np

import assign_ref as ar

# BF_PROJECT_PALETTE of include/bf_accel.h, (B, G, R)
PALETTE = np.array([(255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (255, 255, 0),
                    (0, 128, 255), (255, 128, 0), (128, 0, 255), (0, 255, 128), (128, 128, 255)], dtype=np.int64)
SCORE_FIELDS = ("events", "inside", "pixels_hit", "pixels_owned", "max", "sum_sq")
INFO_FIELDS = ("models", "rows", "cols", "unassigned", "outside", "pixels", "sum", "sum_sq")
M64 = (1 << 64) - 1


def sum_sq(a):
    """sum a^2 modulo 2^64 of a non-negative integer array (uint64 array arithmetic wraps, which is the definition)."""
    a = np.asarray(a).astype(np.uint64).ravel()
    return int((a * a).sum(dtype=np.uint64))


def project(sl, ids, models, scale, sensor_res, margin=0, gain=8, mutate=None):
    """-> dict(count uint32[R, C], label int32[R, C], bgr uint8[R, C, 3], scores [dict per group], info dict).  ids: the held
    grouping, -1 .. K-1 in upload order."""
    K = len(models)
    n = len(sl["t"])
    w = ar.window(scale, sensor_res, margin)
    R, C = w["R"], w["C"]
    ids = np.asarray(ids).astype(np.int64)
    assert ids.shape == (n,)
    B = np.zeros((K, R, C), dtype=np.int64)
    scores = []
    outside = 0
    for k, m in enumerate(models):
        mine = ids == k
        if mutate == "count_unassigned" and k == 0:
            mine = mine | (ids == -1)
        events = int(mine.sum())
        inside = 0
        if events:
            sub = dict(fr_x=np.asarray(sl["fr_x"])[mine], fr_y=np.asarray(sl["fr_y"])[mine], t=np.asarray(sl["t"])[mine])
            ins, X, Y = ar.pixels(sub, m, w, scale)
            inside = int(ins.sum())
            V = np.bincount((X * C + Y)[ins], minlength=R * C).reshape(R, C)
            B[k] = ar.box_sum(V, scale) if scale > 1 else V
        outside += events - inside
        scores.append(dict(events=events, inside=inside, pixels_hit=int((B[k] > 0).sum()), pixels_owned=0, max=int(B[k].max()),
                           sum_sq=sum_sq(B[k])))
    N = B.sum(axis=0)
    if mutate == "ties_up":
        arg = K - 1 - np.argmax(B[::-1], axis=0)
    else:
        arg = np.argmax(B, axis=0)   # (the first maximum: the smallest k)
    label = np.where(N > 0, arg, -1).astype(np.int32)
    for k in range(K):
        scores[k]["pixels_owned"] = int((label == k).sum())
    top = N if mutate == "label_by_total" else B.max(axis=0)
    level = np.minimum(255, top * int(gain))
    bgr = (PALETTE[np.maximum(label, 0) % len(PALETTE)] * level[..., None]) // 255
    bgr[label < 0] = 0
    unassigned = 0 if mutate == "count_unassigned" else int((ids == -1).sum())
    info = dict(models=K, rows=R, cols=C, unassigned=unassigned, outside=outside, pixels=int((N > 0).sum()), sum=int(N.sum()) & M64,
                sum_sq=sum_sq(N))
    if n == 0:   # "scores and info zero (rows and cols too)"
        info = dict.fromkeys(INFO_FIELDS, 0)
    return dict(count=N.astype(np.uint32), label=label, bgr=bgr.astype(np.uint8), scores=scores, info=info)


def flat_scores(scores):
    """[K, 6] of Python-exact integers as uint64 (what bf_group_score holds)."""
    return np.array([[s[f] for f in SCORE_FIELDS] for s in scores], dtype=np.uint64).reshape(len(scores), len(SCORE_FIELDS))


def scene_truth(sc):
    """The scene's true grouping (background 0, patch 1) and true models."""
    import segment_scene as scene
    ids = sc["is_patch"].astype(np.int32)
    return ids, [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity(scene.V_PATCH)]
