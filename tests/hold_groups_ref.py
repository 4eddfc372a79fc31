"""numpy restatement of bf_hold_groups and bf_group_flow_medians (include/bf_accel.h, "the held flow of a grouping"; DESIGN.md
section 19) -- TEST INFRASTRUCTURE ONLY.  Built from what is already stated once:

    warp      assign_ref.warp_of (set_model's warp_reinit, libm's sine and cosine) and the arithmetic of assign_ref.pixels
              lines 39-47: every operation a separate IEEE operation, in its order, from the reset state pr = fr
    held      global_flow_ref._held: the positions of global_piecewise_ref.project_per_event with nz = 127 and
              Event::compute_uv with libm's hypot; an event of no group has (nx, ny) = 0: zero flow, pr = fr
    readers   global_flow_ref.flow_field / frame_tiles / emit_rows, unchanged
    median    np.sort on the 64-bit order keys; element c/2 of an odd count, 0.5 * (a[c/2-1] + a[c/2]) of an even one, 0.0 of none

`mutate` switches one rule off for the mutation tests: "model0" (group 0's model for everyone), "upper" (the upper middle
instead of the mean), "minus_one_in_0" (ids of -1 counted in group 0)."""
import numpy as np

import assign_ref as ar
import global_flow_ref as R

F32 = np.float32
NZ = 127.0
SIGN = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def group_n(sl, m):
    """(nx, ny) of every event of sl under ONE warp_reinit of model m from the reset state (assign_ref.pixels, lines 39-47)."""
    dnx, dny, cx, cy, div, s, c = (np.float64(v) for v in ar.warp_of(m))
    fx = np.asarray(sl["fr_x"]).astype(F32).astype(np.float64)   # Event::reset: pr = fr
    fy = np.asarray(sl["fr_y"]).astype(F32).astype(np.float64)
    rx, ry = fx - cx, fy - cy
    qx = c * rx - s * ry
    qy = s * rx + c * ry
    nx = ((-qx) * div + (qx - rx)) + dnx
    ny = ((-qy) * div + (qy - ry)) + dny
    return nx, ny


def hold(sl, ids, models, mutate=None):
    """The held flow as a dict of global_flow_ref.KEYS, upload order."""
    ids = np.asarray(ids).astype(np.int64)
    n = len(ids)
    nx, ny = np.zeros(n), np.zeros(n)
    for k, m in enumerate(models):
        sel = ids == k
        if mutate == "minus_one_in_0" and k == 0:
            sel = sel | (ids < 0)
        if not sel.any():
            continue
        gx, gy = group_n(sl, models[0] if mutate == "model0" else m)
        nx[sel], ny[sel] = gx[sel], gy[sel]
    return R._held(np.asarray(sl["fr_x"]), np.asarray(sl["fr_y"]), np.asarray(sl["t"]), nx, ny, NZ)


def key(x):
    """The total order of the doubles as uint64 keys: bits ^ (sign ? ~0 : 1 << 63); -0.0 below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where((b >> np.uint64(63)).astype(bool), ALL, SIGN)


def unkey(k):
    k = np.asarray(k, dtype=np.uint64)
    return (k ^ np.where((k >> np.uint64(63)).astype(bool), SIGN, ALL)).view(np.float64)


def median(a, mutate=None):
    """The median of a 1-d array by the key order, as a float64."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    c = len(a)
    if c == 0:
        return np.float64(0.0)
    s = unkey(np.sort(key(a)))
    if c % 2 or mutate == "upper":
        return np.float64(s[c // 2])
    return np.float64(0.5) * (np.float64(s[c // 2 - 1]) + np.float64(s[c // 2]))


def medians(u, v, ids, K, mutate=None):
    """-> (u_med float64[K], v_med float64[K], counts int32[K + 1] (last: ids of -1))."""
    ids = np.asarray(ids).astype(np.int64)
    um, vm = np.zeros(K), np.zeros(K)
    counts = np.zeros(K + 1, dtype=np.int32)
    for k in range(K):
        sel = ids == k
        if mutate == "minus_one_in_0" and k == 0:
            sel = sel | (ids < 0)
        um[k], vm[k] = median(np.asarray(u)[sel], mutate), median(np.asarray(v)[sel], mutate)
        counts[k] = int(sel.sum())
    counts[K] = len(ids) - int(counts[:K].sum())
    return um, vm, counts


def finder_median(a):
    """bf::ObjectFinder::group_flows' formula (object_finder.h): std::sort, then the middle or the mean of the two middles."""
    a = sorted(float(x) for x in a)
    m = len(a) // 2
    return a[m] if len(a) % 2 else 0.5 * (a[m - 1] + a[m])
