"""Restatement of the moving-object segmentation (include/bf_accel.h, "moving-object segmentation") in numpy / plain Python:
quantised time, floor mean, foreground test, components by a row-run union-find, size filter, renumbering, the component
table and the per-event cluster ids.  Integers throughout; no scipy."""
import math

import numpy as np

COMPONENT_DTYPE = np.dtype([(n, np.int32) for n in ("id", "first_pixel", "pixels", "events", "row_min", "row_max", "col_min",
                                                    "col_max")] + [(n, np.int64) for n in ("row_sum", "col_sum", "q_sum")])
Q_ONE = 1 << 30


def quantise(T):
    """q = floor((double)T * 2^30) as int64 (the conversion and the product are exact)."""
    return np.floor(np.asarray(T, dtype=np.float32).astype(np.float64) * float(Q_ONE)).astype(np.int64)


def mean_q(T, c):
    """(n1, Q, mu): pixels with c >= 1, the exact sum of q over them, floor_div(Q, n1) (0 without pixels)."""
    on = np.asarray(c) >= 1
    n1 = int(on.sum())
    Q = int(sum(int(v) for v in quantise(T)[on].tolist()))
    return n1, Q, (Q // n1 if n1 else 0)   # Python's // floors


def threshold(s):
    if math.isnan(s) or math.isinf(s):
        raise ValueError("threshold is NaN or infinite")
    return None if s < 0 else int(math.floor(s * float(Q_ONE)))


def foreground(T, c, above_s=-1.0, below_s=-1.0, min_count=1):
    assert min_count >= 1
    A, B = threshold(above_s), threshold(below_s)
    _, _, mu = mean_q(T, c)
    q = quantise(T)
    enough = np.asarray(c).astype(np.int64) >= min_count
    if A is None and B is None:
        return enough
    hit = np.zeros(q.shape, dtype=bool)
    if A is not None:
        hit |= (q - mu) > A
    if B is not None:
        hit |= (mu - q) > B
    return enough & hit


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        if a < b:
            parent[b] = a
        else:
            parent[a] = b


def label(mask, connectivity=8, min_pixels=1, q=None):
    """(labels int32 (R, C), table COMPONENT_DTYPE (K,), found): components of `mask` by a union-find over row runs; runs are
    created in row-major order, so the smallest run index of a component is the run holding its smallest pixel."""
    assert connectivity in (4, 8) and min_pixels >= 1
    mask = np.asarray(mask) != 0
    R, C = mask.shape
    runs = []            # (row, first col, last col)
    by_row = [[] for _ in range(R)]
    for r in range(R):
        row = mask[r]
        edges = np.flatnonzero(np.diff(np.concatenate(([0], row.view(np.int8), [0]))))
        for a, b in zip(edges[0::2].tolist(), edges[1::2].tolist()):
            by_row[r].append(len(runs))
            runs.append((r, a, b - 1))
    parent = list(range(len(runs)))
    reach = 1 if connectivity == 8 else 0
    for r in range(1, R):
        up = by_row[r - 1]
        j0 = 0
        for i in by_row[r]:
            _, a, b = runs[i]
            while j0 < len(up) and runs[up[j0]][2] < a - reach:
                j0 += 1
            j = j0
            while j < len(up) and runs[up[j]][1] <= b + reach:
                _union(parent, i, up[j])
                j += 1
    roots = [_find(parent, i) for i in range(len(runs))]
    pixels = {}
    for i, rt in enumerate(roots):
        pixels[rt] = pixels.get(rt, 0) + runs[i][2] - runs[i][1] + 1
    found = len(pixels)
    kept = [rt for rt in sorted(pixels) if pixels[rt] >= min_pixels]   # run order == order of the smallest pixel
    ident = {rt: k for k, rt in enumerate(kept)}
    labels = np.full((R, C), -1, dtype=np.int32)
    table = np.zeros(len(kept), dtype=COMPONENT_DTYPE)
    table["id"] = np.arange(len(kept))
    table["row_min"] = table["col_min"] = np.iinfo(np.int32).max
    table["row_max"] = table["col_max"] = np.iinfo(np.int32).min
    for k, rt in enumerate(kept):
        table["first_pixel"][k] = runs[rt][0] * C + runs[rt][1]
    for i, rt in enumerate(roots):
        k = ident.get(rt)
        if k is None:
            continue
        r, a, b = runs[i]
        labels[r, a:b + 1] = k
        t = table[k]
        n = b - a + 1
        t["pixels"] += n
        t["row_min"] = min(t["row_min"], r); t["row_max"] = max(t["row_max"], r)
        t["col_min"] = min(t["col_min"], a); t["col_max"] = max(t["col_max"], b)
        t["row_sum"] += r * n
        t["col_sum"] += (a + b) * n // 2
        if q is not None:
            t["q_sum"] += int(q[r, a:b + 1].sum())
    return labels, table, found


def event_pixels(pr_x, pr_y, window, noise=None):
    """The centre pixel of every event as get_time_img_cpu forms it (accel_lib.h:154-158): (x, y, taken)."""
    s = int(window.scale)
    x_sh, y_sh = int(window.x_shift), int(window.y_shift)            # the double -> int parameter conversion of :147
    x = np.trunc(np.asarray(pr_x, dtype=np.float64) * s + x_sh).astype(np.int64)
    y = np.trunc(np.asarray(pr_y, dtype=np.float64) * s + y_sh).astype(np.int64)
    w, h, hs = int(window.metric_wsizex), int(window.metric_wsizey), s // 2
    taken = ~((x >= w + hs) | (x < hs) | (y >= h + hs) | (y < hs))
    if noise is not None:
        taken &= np.asarray(noise) == 0
    return x, y, taken


def segment(T, c, pr_x, pr_y, window, above_s=-1.0, below_s=-1.0, min_count=1, connectivity=8, min_pixels=1, noise=None):
    """The whole of bf_segment on a time image, a count image and the events' positions (bf_writeout_events).  Returns a dict:
    info fields, labels, table, cl_id."""
    T = np.asarray(T, dtype=np.float32)
    n1, Q, mu = mean_q(T, c)
    mask = foreground(T, c, above_s, below_s, min_count)
    labels, table, found = label(mask, connectivity, min_pixels, quantise(T))
    x, y, taken = event_pixels(pr_x, pr_y, window, noise)
    cl_id = np.full(len(x), -1, dtype=np.int32)
    cl_id[taken] = labels[x[taken], y[taken]]
    table["events"] = np.bincount(cl_id[cl_id >= 0], minlength=len(table))[:len(table)] if len(table) else 0
    return dict(rows=T.shape[0], cols=T.shape[1], n1=n1, q_sum=Q, q_mean=mu, foreground_pixels=int(mask.sum()),
                components_found=found, components=len(table), labels=labels, table=table, cl_id=cl_id)
