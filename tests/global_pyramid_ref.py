"""numpy restatement of the coarse-to-fine / seeded per-cell search (bf_global_search_cells_pyramid, include/bf_accel.h,
DESIGN.md "OptimizerGlobal"), on top of tests/global_cells_ref.py:

  * the lattice: n_x x n_y points, k = i * n_y + j, the values of tests/global_ref.py's sweep_values;
  * the schedule: level l has the stride factor ** (levels - 1 - l); level 0 without seeds is every (i, j) with both
    indices a multiple of the stride; every other level is the union over the cells that have events and a centre (the
    running best when its S > 0, else the seed when >= 0) of the (2 radius + 1)^2 window, stride apart, clipped to the
    lattice, minus everything evaluated before; ascending k within a level;
  * the fold: GlobalCells.project_all_cells per evaluated candidate, in evaluation order (the per-event state);
  * the answer: per cell the evaluated candidate with the largest S(k, cell), lowest k among equals; the slice from the
    sum over cells by the same rule.
"""
import ctypes
import ctypes.util

import numpy as np

import global_cells_ref as GC
import global_ref as G

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]


def compute_uv(nx, ny, nz=G.NZ):
    """Event::compute_uv (event.h:135-142) with the C library's hypot, which the product's host code calls: Python's
    math.hypot (global_ref.compute_uv) rounds a few lattice points differently (2 of this file's tests' 23 x 13, 76 of the
    default 180 x 80), and a search that may land on any of them is compared bit for bit."""
    xy_len = _libm.hypot(nx, ny)
    speed = xy_len / (nz / (1000000000 / (1 * 10000)))
    if xy_len == 0:
        return 0.0, 0.0
    return speed * nx / xy_len, speed * ny / xy_len


def best_uv(ref):
    """compute_uv of each event's winning candidate (G.Global.best_uv with the hypot above)"""
    uv = {}
    u, v = np.zeros(len(ref.best_nx)), np.zeros(len(ref.best_nx))
    for i, key in enumerate(zip(ref.best_nx, ref.best_ny, ref.best_nz)):
        if key not in uv:
            uv[key] = compute_uv(*key)
        u[i], v[i] = uv[key]
    return u, v


def strides(levels, factor):
    return [factor ** (levels - 1 - l) for l in range(levels)]


def strided_level(n_x, n_y, s):
    """level 0 without seeds, ascending k"""
    return [i * n_y + j for i in range(0, n_x, s) for j in range(0, n_y, s)]


def centres(events, best_sum, best_k, seeds):
    """The centre k of every cell that contributes a window (None for the others): a cell with events, centred on its
    running best when that has S > 0, else on its seed when there is one (>= 0)."""
    out = []
    for c in range(len(events)):
        if events[c] == 0:
            out.append(None)
        elif best_sum[c] > 0:
            out.append(int(best_k[c]))
        elif seeds is not None and seeds[c] >= 0:
            out.append(int(seeds[c]))
        else:
            out.append(None)
    return out


def window_level(n_x, n_y, s, r, cents, evaluated):
    """The union of the windows around `cents` (None: no window), clipped, minus the set `evaluated`; ascending k."""
    new = set()
    for kc in cents:
        if kc is None:
            continue
        ic, jc = divmod(kc, n_y)
        for a in range(-r, r + 1):
            for b in range(-r, r + 1):
                i, j = ic + a * s, jc + b * s
                if 0 <= i < n_x and 0 <= j < n_y and i * n_y + j not in evaluated:
                    new.add(i * n_y + j)
    return sorted(new)


def answer(ks, values):
    """index into ks of the largest value, the lowest k among equals"""
    best = 0
    for m in range(1, len(ks)):
        if values[m] > values[best] or (values[m] == values[best] and ks[m] < ks[best]):
            best = m
    return best


class Running:
    """the per-cell running best over evaluated candidates: (largest S, lowest k)"""

    def __init__(self, n_cells):
        self.best_sum = np.zeros(n_cells, dtype=np.int64)
        self.best_k = np.full(n_cells, -1, dtype=np.int64)

    def fold(self, k, S):
        up = (self.best_k < 0) | (S > self.best_sum) | ((S == self.best_sum) & (k < self.best_k))
        self.best_sum[up] = S[up]
        self.best_k[up] = k


def search_pyramid(ref, xs, ys, levels, factor, radius, seeds=None, nz=G.NZ, score=None):
    """The search on a GC.GlobalCells `ref` (whose per-event state folds on).  score(k) -> S(k, cell) [n_cells] replaces
    ref.project_all_cells (a cache of an order-free quantity: the per-event state is then not folded).  Returns a dict:
    evaluated (list of k, evaluation order), level_count, surface int64 [n_cells, n_evaluated], cells (the dict of
    GC.GlobalCells.search_cells), slice (best_nx, best_ny, best_sum)."""
    n_x, n_y = len(xs), len(ys)
    assert 1 <= levels <= 8 and factor >= 2 and radius >= 1
    st = strides(levels, factor)
    assert st[0] <= max(n_x, n_y)
    if seeds is not None:
        seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
        assert len(seeds) == ref.n_cells and ((seeds >= -1) & (seeds < n_x * n_y)).all()
    if score is None:
        score = lambda k: ref.project_all_cells(xs[k // n_y], ys[k % n_y], nz)
    run = Running(ref.n_cells)
    evaluated, done, cols, level_count = [], set(), [], []
    for l, s in enumerate(st):
        if l == 0 and seeds is None:
            ks = strided_level(n_x, n_y, s)
        else:
            ks = window_level(n_x, n_y, s, radius, centres(ref.events, run.best_sum, run.best_k, seeds), done)
        level_count.append(len(ks))
        for k in ks:
            S = score(k)
            cols.append(S)
            run.fold(k, S)
        evaluated += ks
        done.update(ks)
    assert evaluated, "nothing to evaluate"
    surf = np.stack(cols, axis=1) if cols else np.zeros((ref.n_cells, 0), dtype=np.int64)
    k = run.best_k
    shape = (ref.n_cell_x, ref.n_cell_y)
    cells = {"best_index": k.copy().reshape(shape), "events": ref.events.reshape(shape),
             "best_sum": run.best_sum.copy().reshape(shape),
             "best_nx": np.array([xs[i // n_y] for i in k]).reshape(shape),
             "best_ny": np.array([ys[i % n_y] for i in k]).reshape(shape)}
    uv = [compute_uv(a, b, nz) for a, b in zip(cells["best_nx"].ravel(), cells["best_ny"].ravel())]
    cells["best_u"] = np.array([p[0] for p in uv], dtype=np.float64).reshape(shape)
    cells["best_v"] = np.array([p[1] for p in uv], dtype=np.float64).reshape(shape)
    total = surf.sum(axis=0)
    b = evaluated[answer(evaluated, total)]
    return {"evaluated": evaluated, "level_count": level_count, "surface": surf, "cells": cells,
            "slice": (xs[b // n_y], ys[b % n_y], int(total[evaluated.index(b)]))}
