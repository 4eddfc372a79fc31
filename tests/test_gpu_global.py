"""OptimizerGlobal on the GPU (bf_global_*): bit-identical to the numpy restatement of the reference (tests/global_ref.py)."""
import os

import numpy as np
import pytest

import global_ref as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "slice_6k_120x90.npz"))
    return d["fr_x"].astype(np.int64), d["fr_y"].astype(np.int64), d["t"].astype(np.int64)


def _synth(n, h, w, dur=0.03, seed=11, velocity=None):
    from better_flow_amd import synth
    sl = synth.make_slice(n, h, w, dur, seed=seed, velocity=velocity)
    return sl["fr_x"].astype(np.int64), sl["fr_y"].astype(np.int64), sl["t"].astype(np.int64)


SLICES = {"golden": _golden, "synth346": lambda: _synth(20000, 260, 346), "synth640": lambda: _synth(20000, 480, 640, seed=12)}


def _accel(accel_mod, ev):
    fr_x, fr_y, t = ev
    acc = accel_mod.Accel(device=0, max_events=max(len(t), 1))
    acc.upload_events(fr_x, fr_y, t)
    return acc


def _state(acc):
    return acc.global_get_events()


def _check_state(got, ref):
    assert np.array_equal(got["max_score"], ref.max_score)
    assert np.array_equal(got["best_nx"], ref.best_nx)
    assert np.array_equal(got["best_ny"], ref.best_ny)
    assert np.array_equal(got["best_pr_x"], ref.best_pr_x)
    assert np.array_equal(got["best_pr_y"], ref.best_pr_y)


XS, YS = G.default_grid()
CANDS = [(0.0, 0.0), (XS[0], YS[0]), (XS[-1], YS[-1]), (XS[0], YS[-1]), (XS[90], YS[40]), (3.0, -2.0)]

CASES = [("golden", 1, 5), ("golden", 1, 21), ("golden", 3, 15), ("golden", 3, 21), ("golden", 5, 25), ("golden", 5, 9),
         ("golden", 7, 35), ("golden", 7, 21), ("golden", 7, 3), ("golden", 5, 63),
         ("synth346", 5, 21), ("synth346", 7, 35), ("synth346", 3, 11), ("synth640", 3, 15), ("synth640", 5, 25)]


@pytest.mark.parametrize("name,scale,mw", CASES)
def test_project_all_bit_identical(accel_mod, name, scale, mw):
    ev = SLICES[name]()
    acc = _accel(accel_mod, ev)
    try:
        w = acc.global_set_window(scale, mw)
        ref = G.Global(*ev, scale=scale, metric_wsize=mw)
        for k in ("x_min", "y_min", "x_max", "y_max", "scale_img_x", "scale_img_y", "scale_bordered_img_x",
                  "scale_bordered_img_y"):
            assert getattr(w, k) == ref.w[k], k
        cands = CANDS if name == "golden" else CANDS[:3] + CANDS[-1:]
        for nx, ny in cands:
            S, img, cur = acc.global_project_all(nx, ny)
            rimg, rcur, rS = ref.project_all(nx, ny)
            assert np.array_equal(img, rimg), (nx, ny)
            assert np.array_equal(cur.view(np.uint32), rcur.view(np.uint32)), (nx, ny)
            assert S == rS, (nx, ny)
        _check_state(_state(acc), ref)
    finally:
        acc.close()


def _opts(accel_mod, xlo, xhi, ylo, yhi, step=0.001):
    return accel_mod.Accel.global_search_opts(x_low=xlo, x_hi=xhi, x_step=step, y_low=ylo, y_hi=yhi, y_step=step)


def test_search_subgrid_equals_restatement_and_project_all_loop(accel_mod):
    ev = _golden()
    xs, ys = G.sweep_values(-0.03, 0.0005, 0.001), G.sweep_values(-0.01, 0.0105, 0.001)
    assert (len(xs), len(ys)) == (31, 21)
    ref = G.Global(*ev, scale=3, metric_wsize=15)
    rsurf, (rbx, rby, rbs) = ref.search(xs, ys)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(3, 15)
        r, surf = acc.global_search(_opts(accel_mod, -0.03, 0.0005, -0.01, 0.0105))
        assert (r.n_x, r.n_y) == (31, 21)
        assert np.array_equal(surf, rsurf)
        assert (r.best_nx, r.best_ny, r.best_sum) == (rbx, rby, rbs)
        got = _state(acc)
        _check_state(got, ref)
        u, v = ref.best_uv()
        assert np.array_equal(got["best_u"], u) and np.array_equal(got["best_v"], v)
        # the second device path: one project_all per candidate
        acc.global_set_window(3, 15)
        loop = np.array([[acc.global_project_all(x, y, want_img=False, want_scores=False)[0] for y in ys] for x in xs])
        assert np.array_equal(loop, surf)
        again = _state(acc)
        for k in got:
            assert np.array_equal(again[k], got[k]), k
    finally:
        acc.close()


def test_default_sweep_50k(accel_mod):
    ev = _synth(52000, 180, 240, seed=21)
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window()                        # OptimizerGlobal(events): scale 5, window 21
        r1, s1 = acc.global_search()
        st1 = _state(acc)
        acc.global_set_window()
        r2, s2 = acc.global_search()
        st2 = _state(acc)
    finally:
        acc.close()
    assert (r1.n_x, r1.n_y) == (180, 80)
    assert np.array_equal(s1, s2)
    for k in st1:
        assert np.array_equal(st1[k], st2[k]), k
    assert (r1.best_nx, r1.best_ny, r1.best_sum) == (r2.best_nx, r2.best_ny, r2.best_sum)
    k = int(np.argmax(s1))
    assert (r1.best_nx, r1.best_ny, r1.best_sum) == (XS[k // 80], YS[k % 80], s1.max())
    ref = G.Global(*ev, scale=5, metric_wsize=21)
    rng = np.random.default_rng(3)
    picks = [(k // 80, k % 80), (0, 0), (179, 79)] + [tuple(p) for p in zip(rng.integers(0, 180, 37), rng.integers(0, 80, 37))]
    for i, j in picks:
        assert ref.project_all(XS[i], YS[j])[2] == s1[i, j], (i, j)


def test_half_grids_accumulate_and_window_resets(accel_mod):
    ev = _golden()
    step = 2.0 ** -7                                  # exact in binary: the half grids hold the union's values
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window(5, 21)
        _, a = acc.global_search(_opts(accel_mod, -0.0625, 0.0, -0.03125, 0.03125, step))
        _, b = acc.global_search(_opts(accel_mod, 0.0, 0.0625, -0.03125, 0.03125, step))
        halves = _state(acc)
        acc.global_set_window(5, 21)
        _, whole = acc.global_search(_opts(accel_mod, -0.0625, 0.0625, -0.03125, 0.03125, step))
        union = _state(acc)
        assert np.array_equal(np.vstack([a, b]), whole)
        for k in union:
            assert np.array_equal(halves[k], union[k]), k
        assert union["max_score"].max() > 0
        acc.global_set_window(5, 21)
        reset = _state(acc)
        assert not reset["max_score"].any() and not reset["best_nx"].any() and not reset["best_u"].any()
        assert np.array_equal(reset["best_pr_x"], ev[0].astype(np.float64))
        assert np.array_equal(reset["best_pr_y"], ev[1].astype(np.float64))
    finally:
        acc.close()


def test_edge_cases(accel_mod):
    from better_flow_amd.accel import BF_ERR_ARG, BfError
    small = _opts(accel_mod, -0.002, 0.002, -0.002, 0.002)
    # an empty cloud: every S is 0
    acc = accel_mod.Accel(device=0, max_events=16)
    try:
        acc.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        w = acc.global_set_window(3, 5)
        assert (w.scale_img_x, w.scale_bordered_img_x) == (0, 5)
        r, s = acc.global_search(small)
        assert (r.n_x, r.n_y) == (4, 4) and not s.any() and r.best_sum == 0
        S, img, cur = acc.global_project_all(0.0, 0.0)
        assert S == 0 and not img.any() and cur.size == 0
    finally:
        acc.close()
    # one event: its bounding box leaves no accepted pixel; several events all pushed off the window
    # (the third: (7, 9) sits on the bounding box's far edge; the other two move ~400 px under (50, 50), 0 under (0, 0))
    pushed = (np.array([2, 2, 7]), np.array([2, 3, 9]), np.array([10000000, 20000000, 0]))
    for ev, cand in (((np.array([5]), np.array([7]), np.array([100])), (0.0, 0.0)), (pushed, (50.0, 50.0))):
        acc = _accel(accel_mod, ev)
        try:
            acc.global_set_window(5, 21)
            S, img, cur = acc.global_project_all(*cand)
            assert S == 0 and not img.any() and not cur.any()
            st = _state(acc)
            assert not st["max_score"].any()
            assert np.array_equal(st["best_pr_x"], ev[0].astype(np.float64))
        finally:
            acc.close()
    acc = _accel(accel_mod, pushed)
    try:
        acc.global_set_window(5, 21)
        assert acc.global_project_all(0.0, 0.0)[0] == G.Global(*pushed, scale=5, metric_wsize=21).project_all(0.0, 0.0)[2] > 0
    finally:
        acc.close()
    # bad arguments
    acc = _accel(accel_mod, _golden())
    try:
        with pytest.raises(BfError) as e:
            acc.global_search(small)                  # no window yet
        assert e.value.code == BF_ERR_ARG
        for scale, mw in ((2, 21), (4, 0), (9, 21), (5, 20), (3, 65)):
            with pytest.raises(BfError) as e:
                acc.global_set_window(scale, mw)
            assert e.value.code == BF_ERR_ARG, (scale, mw)
        acc.global_set_window(3, 0)
        assert acc._gwin.metric_wsize == 15
        for kw in (dict(x_step=0.0), dict(y_step=-0.001), dict(x_low=0.1, x_hi=0.1), dict(y_low=0.05, y_hi=-0.05)):
            o = accel_mod.Accel.global_search_opts(**kw)
            with pytest.raises(BfError) as e:
                acc.global_search(o, want_surface=False)
            assert e.value.code == BF_ERR_ARG, kw
        with pytest.raises(BfError) as e:
            acc.global_search(small, surface_cap=15)      # 16 candidates
        assert e.value.code == BF_ERR_ARG
    finally:
        acc.close()


def test_recovers_injected_flow(accel_mod):
    """A slice moving at (40, -20) px/s (rows, columns) over 0.2 s: inside the default range.  The restatement's objective
    peaks on the grid point next to the truth (checked on the CPU, DESIGN.md "OptimizerGlobal").  Asserted here: the device's
    slice best, and the median of the events' best_u / best_v, each within RECOVERY_TOL (1 px/s) of the truth."""
    ev = _synth(50000, 180, 240, dur=0.2, seed=5, velocity=(40.0, -20.0))
    acc = _accel(accel_mod, ev)
    try:
        acc.global_set_window()
        r, surf = acc.global_search()
        st = _state(acc)
    finally:
        acc.close()
    u_best, v_best = G.compute_uv(r.best_nx, r.best_ny)
    assert abs(u_best - 40.0) <= RECOVERY_TOL and abs(v_best + 20.0) <= RECOVERY_TOL, (u_best, v_best)
    assert abs(np.median(st["best_u"]) - 40.0) <= RECOVERY_TOL and abs(np.median(st["best_v"]) + 20.0) <= RECOVERY_TOL


RECOVERY_TOL = 1.0


def test_upload_invalidates_the_window(accel_mod):
    """A new slice of the SAME size (the fixed-size ring case) must not run on the previous slice's window and state."""
    from better_flow_amd.accel import BF_ERR_ARG, BF_ERR_STATE, BfError
    a = _synth(6000, 90, 120, seed=31)
    b = _synth(6000, 90, 120, seed=32, velocity=(60.0, -90.0))
    n = min(len(a[0]), len(b[0]))
    a = tuple(x[:n] for x in a)
    b = tuple(x[:n] for x in b)
    small = _opts(accel_mod, -0.002, 0.002, -0.002, 0.002)
    acc = _accel(accel_mod, a)
    try:
        with pytest.raises(BfError) as e:          # no window yet: an argument error, not an AttributeError
            acc.global_project_all(0.0, 0.0)
        assert e.value.code == BF_ERR_ARG
        acc.global_set_window(3, 15)
        acc.global_search(small)
        for upload in ("sync", "async"):
            if upload == "sync":
                acc.upload_events(*b)
            else:
                bx, by, bt = (np.ascontiguousarray(x, dtype=np.int32) for x in b)
                acc.upload_events_async(bx, by, bt, n)
                acc.commit_upload()
            for call in (lambda: acc.global_search(small), lambda: acc.global_project_all(0.0, 0.0), acc.global_get_events):
                with pytest.raises(BfError) as e:
                    call()
                assert e.value.code == BF_ERR_STATE, upload
            # a window on the new slice: its own bounding box, fresh state, the restatement's numbers
            w = acc.global_set_window(3, 15)
            ref = G.Global(*b, scale=3, metric_wsize=15)
            assert (w.x_min, w.x_max, w.y_min, w.y_max) == (ref.w["x_min"], ref.w["x_max"], ref.w["y_min"], ref.w["y_max"])
            S, img, cur = acc.global_project_all(0.001, -0.002)
            rimg, rcur, rS = ref.project_all(0.001, -0.002)
            assert S == rS and np.array_equal(img, rimg) and np.array_equal(cur, rcur)
            _check_state(_state(acc), ref)
    finally:
        acc.close()
