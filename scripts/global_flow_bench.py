"""The held flow of the exhaustive search (bf_global_hold_field and its readers) on the inputs of scripts/global_field_bench.py:

  * the 52 000-event 240 x 180 slice, scale 5, window 21, with 8 x 8- and 32 x 32-pixel cells;
  * config 4's input (1M events, 346 x 260, scale 3, window 15) with 8 x 11-pixel cells (33 x 32 of them).

Per input and grid (the grid of global_field_bench.py: the injected flow's lattice point plus a ramp), ms per call, best of
--reps (3) after one warm-up repeat of --inner calls, every call ending in its own synchronise:

  per_event_outputs   bf_global_hold_field (smooth form) + bf_global_get_flow(nx, ny, u, v) against bf_global_project_field
                      asked for the same four arrays and nothing else; with --parent-lib PATH the latter is also timed on that
                      library (a build of the parent commit), in the same process; all through the C-ABI with the caller's
                      arrays made once.  get_flow_alone: the copy-out without the hold.  ns_per_event: the first, per event.
  hold_alone          bf_global_hold_field in either form (one launch, the grid's upload and a synchronise).
  flow_frame          bf_global_render_flow_frame against the rolling bf_render_flow_frame of the same slice after one warp.
  emit                bf_global_emit_slice + wait + release against bf_emit_slice + wait + release, a fresh ring position range
                      per call (every event is emitted every time).

--kernels: only a few calls of bf_global_hold_field (both forms), bf_global_project_cells and bf_global_project_field per input,
for a kernel trace of the process.  Writes profiles/global_flow_bench.json (--out to change) and prints the same JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from better_flow_amd import accel, synth  # noqa: E402

NZ = 127.0
KEYS = ("nx", "ny", "u", "v")


def best_ms(call, reps, inner):
    """ms per call: the best of `reps` repeats of `inner` calls after one warm-up repeat, and every repeat's value."""
    every = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        if rep:
            every.append((time.perf_counter() - t0) / inner * 1e3)
    return {"ms": round(min(every), 4), "ms_all": [round(t, 4) for t in every]}


def grid_of(acc, sl, sensor, cell):
    tu, tv = sl["velocity"]
    nx, ny = round(tu * NZ * 1e-5, 3), round(tv * NZ * 1e-5, 3)
    g = acc.global_set_cells(*sensor, *cell)
    shape = (g.n_cell_x, g.n_cell_y)
    cx = np.full(shape, nx) + np.linspace(-0.002, 0.002, shape[1])[None, :] * np.ones(shape)
    cy = np.full(shape, ny) + np.linspace(-0.001, 0.001, shape[0])[:, None] * np.ones(shape)
    return cx, cy


class OtherBuild:
    """bf_global_project_field with the four per-event outputs on another build of the library (the parent commit's, which
    lacks the entry points this module's binding declares): the five calls that takes, through ctypes alone."""

    def __init__(self, path, sl, scale, mw):
        self.L = L = C.CDLL(path)
        self.h = C.c_void_p()
        n = len(sl["t"])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        fx, fy, t = (np.ascontiguousarray(sl[k], dtype=np.int32) for k in ("fr_x", "fr_y", "t"))
        L.bf_create.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.bf_upload_events.argtypes = [C.c_void_p] * 5 + [C.c_int64]
        L.bf_global_set_window.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.bf_global_set_cells.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]
        L.bf_global_project_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 4 + \
            [C.c_int64] + [C.c_void_p] * 4
        L.bf_destroy.argtypes = [C.c_void_p]
        L.bf_destroy.restype = None
        self.ok(L.bf_create(0, n, 1024, 1280, None, C.byref(self.h)))
        self.ok(L.bf_upload_events(self.h, p(fx), p(fy), p(t), None, n))
        self.ok(L.bf_global_set_window(self.h, scale, mw, None))
        self.ev = [np.zeros(n) for _ in range(4)]

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError("the other build returned %d" % rc)

    def set_cells(self, sensor, cell):
        self.ok(self.L.bf_global_set_cells(self.h, sensor[0], sensor[1], cell[0], cell[1], None))

    def project_events(self, cx, cy):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.ok(self.L.bf_global_project_field(self.h, p(cx), p(cy), cx.size, NZ, None, None, None, None, 0, *[p(a) for a in self.ev]))

    def close(self):
        self.L.bf_destroy(self.h)


def emit_loop(acc, n, sensor, held):
    """A call that enqueues the slice at a fresh range of ring positions, waits for its rows and releases them."""
    L = acc.L
    em = accel.Emit(acc, 4 * n, sensor[0], sensor[1], 2 * n + 1)
    call = L.bf_global_emit_slice if held else L.bf_emit_slice
    state = {"first": 0}

    def one():
        t, fr, nr = C.c_int64(), C.c_uint64(), C.c_int64()
        # (a start time of its own per call: no event meets the previous call's newest timestamp)
        acc._chk(call(acc.h, em.h, n, state["first"], state["first"] * 1000, 0, 0, 0, 0, C.byref(t)))
        acc._chk(L.bf_emit_wait(acc.h, em.h, t.value, C.byref(fr), C.byref(nr)))
        if nr.value != n:
            raise RuntimeError("the slice emitted %d of %d rows" % (nr.value, n))
        acc._chk(L.bf_emit_release(em.h, fr.value + nr.value))
        state["first"] += n
    return em, one


def one_input(sl, sensor, scale, mw, cell_shapes, reps, inner, parent, kernels):
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n)
    old = OtherBuild(parent, sl, scale, mw) if parent else None
    out = {"events": int(n), "sensor": list(sensor), "scale": scale, "metric_wsize": mw, "calls_per_repeat": inner, "grids": []}
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    if not kernels:
        # the rolling side first: one warp, so that its frame and its table carry a flow
        acc.set_cloud(scale, *sensor)
        acc.project_4param_reinit(-0.013, 0.021, sensor[0] / 2.0, sensor[1] / 2.0, 0.00011, 0.00007)
        out["rolling_flow_frame"] = best_ms(lambda: acc.render_flow_frame(*sensor), reps, inner)
        em, one = emit_loop(acc, n, sensor, False)
        out["rolling_emit"] = best_ms(one, reps, inner)
        em.close()
    acc.global_set_window(scale, mw)
    for cell in cell_shapes:
        cx, cy = grid_of(acc, sl, sensor, cell)
        if kernels:
            for _ in range(inner):
                acc.global_hold_field(cx, cy, mode=accel.BF_GLOBAL_HOLD_CELLS)
                acc.global_hold_field(cx, cy, mode=accel.BF_GLOBAL_HOLD_FIELD)
                acc.global_project_cells(cx, cy, want_img=False, want_scores=False, want_cell_sums=False)
                acc.global_project_field(cx, cy, want_img=False, want_scores=False, want_cell_sums=False)
            continue
        entry = {"cell": list(cell), "cells": list(cx.shape)}
        acc.global_hold_field(cx, cy)
        held = acc.global_get_flow(KEYS)
        ev = acc.global_project_field(cx, cy, want_img=False, want_scores=False, want_cell_sums=False, want_events=True)[4]
        if not all(np.array_equal(held[k], ev[k]) for k in ("nx", "ny")):
            raise RuntimeError("the held (nx, ny) differ from bf_global_project_field's")
        rel = max(float(np.max(np.abs(held[k] - ev[k]) / np.maximum(np.abs(ev[k]), 1e-300))) for k in ("u", "v"))
        entry["uv_max_rel_diff_vs_host"] = rel

        # through the C-ABI with the caller's arrays made once, as a consumer would call it (the binding's methods allocate
        # and zero their outputs per call, which at a million events costs more than the calls)
        L, ptr = acc.L, lambda a: a.ctypes.data_as(C.c_void_p)
        fx, fy = np.ascontiguousarray(cx.reshape(-1)), np.ascontiguousarray(cy.reshape(-1))
        bufs = [np.zeros(n) for _ in range(4)]

        def get_flow():
            acc._chk(L.bf_global_get_flow(acc.h, *[ptr(a) for a in bufs], None, None))

        def hold_and_get():
            acc._chk(L.bf_global_hold_field(acc.h, ptr(fx), ptr(fy), fx.size, NZ, accel.BF_GLOBAL_HOLD_FIELD))
            get_flow()

        def project_events():
            acc._chk(L.bf_global_project_field(acc.h, ptr(fx), ptr(fy), fx.size, NZ, None, None, None, None, 0, *[ptr(a) for a in bufs]))

        pe = {"hold_field_get_flow": best_ms(hold_and_get, reps, inner), "get_flow_alone": best_ms(get_flow, reps, inner),
              "project_field_events": best_ms(project_events, reps, inner)}
        pe["ns_per_event"] = round(pe["hold_field_get_flow"]["ms"] * 1e6 / n, 3)
        if old:
            old.set_cells(sensor, cell)
            pe["parent_project_field_events"] = best_ms(lambda: old.project_events(fx, fy), reps, inner)
            pe["ratio_vs_parent"] = round(pe["hold_field_get_flow"]["ms"] / pe["parent_project_field_events"]["ms"], 4)
        entry["per_event_outputs"] = pe
        entry["hold_alone"] = {"cells": best_ms(lambda: acc.global_hold_field(cx, cy, mode=accel.BF_GLOBAL_HOLD_CELLS), reps, inner),
                               "field": best_ms(lambda: acc.global_hold_field(cx, cy, mode=accel.BF_GLOBAL_HOLD_FIELD), reps, inner)}
        entry["flow_frame"] = best_ms(lambda: acc.global_render_flow_frame(*sensor), reps, inner)
        em, one = emit_loop(acc, n, sensor, True)
        entry["emit"] = best_ms(one, reps, inner)
        em.close()
        out["grids"].append(entry)
    for a in (acc, old):
        if a:
            a.close()
    return out


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    reps, inner = arg("--reps", 3), arg("--inner", 30)
    path = arg("--out", os.path.join(ROOT, "profiles", "global_flow_bench.json"))
    parent = arg("--parent-lib", "") or None
    kernels = "--kernels" in sys.argv
    out = {"slice_52k": one_input(synth.make_slice(52000, 180, 240, 0.03, seed=1), (180, 240), 5, 21, [(8, 8), (32, 32)], reps, inner,
                                  parent, kernels),
           "config4": one_input(synth.make_slice(1000000, 260, 346, 0.03, seed=1), (260, 346), 3, 15, [(8, 11)], reps, inner, parent,
                                kernels)}
    if kernels:
        return
    line = json.dumps({"global_flow": out})
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
