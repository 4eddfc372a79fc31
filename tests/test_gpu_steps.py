"""Every iteration of the descent loop on the device against an exact stepwise reference (tests/step_ref.py).

All loop forms run ONE definition of the per-iteration update (model_update_wave + model_update_rest), so their agreeing bit for
bit cannot show a defect in it, and the oracle can hold a trajectory to its own f32 order noise only.  Here every record of the
device's trace is checked against what the step must give, TEACHER-FORCED: the events of step k are rebuilt on the CPU from
the totals, the centre and the angle the device itself recorded after step k - 1 (np_ref.warp's arithmetic, which the device's
warp has bit for bit: tests/test_gpu_parity.py), so every step has one right answer and nothing accumulates.

Per run (step_ref.CASES x the loop forms of test_gpu_exact.FORMS, with its bf_get_stat proof of the form that ran):
* sine and cosine: the device's own (bf_eval_sincos) of -total_rot of every record; the table and the non-table variant give equal
  bits, and both are within 1 ulp of the correctly rounded value (mpmath).  The warp of bf_set_model takes the host's libm.
* every iteration: the valid-pixel count is exact_ref's; dx, dy, rot, div within exact_ref.moment_bound; total_rot, total_div
  within step_ref.step_bound, total_dx and total_dy BIT-EQUAL, cx and cy within 2 ulp; the four dividers are Control's.
* the stop: info.iterations, rc and the dividers of bf_run_info are Control's, exactly; the returned model is the last record.
* after the run: writeout_events() is the replay's final pr_x, pr_y, nx, ny bit for bit; compute_uv() is event.h:135-142 on
  those nx, ny to 1e-14; get_time_img() is exact_ref on the final pr (test_gpu_exact.check_images).
A convergence test within 4 ulp of its threshold makes the run inconclusive, and the test fails saying so (step_ref.Undecidable).

The cases and what each is there for are step_ref.CASES and tests/test_step_ref_cpu.py's PURPOSE, proven there on the oracle:
translation at scales 3, 1 and 5, rotation, divergence, both, a warm start (the set_model warp fused into the first counting
sort), a max_iter stop on an iteration that would double dividers, and |angle| = 0.3, where every update takes the out-of-line
library sine (sincos_large) inside the loop kernel.

No case ends by the divider limit (optimizer_rolling.h:76-79).  A search on the CPU oracle over 64 slices (synth.make_slice seeds
1 .. 40 at 60 x 80, 20 000 events, scale 1; seeds 1 .. 12 at scale 3; seeds 1 .. 12 at 48 x 64, 12 000 events, scale 5; at most
3000 iterations each) found none: every run ended by convergence.  Config 2's divider assertion (tests/test_gpu_geometries.py)
remains that branch's only cover on the device; Control's own branch runs on a made-up sequence in tests/test_step_ref_cpu.py.

All forms return the same trace, so the CPU replay (about 10 ms per iteration) is cached on the trace's bytes; the GPU part of a
run is milliseconds.  All inputs are valid slices; nothing here provokes anything.
"""
import math

import numpy as np
import pytest

import exact_ref as X
import step_ref as SR
from test_gpu_exact import FORMS, check_images, new_accel, stage

pytestmark = pytest.mark.gpu

TRACE_CAP = 1024
FAMILIES = ("global atomics", "dense slabs", "event lists", "one-kernel pass", "persistent loop")
RUNS = [(case, i) for case, c in SR.CASES.items() for i, f in enumerate(FORMS) if c["all_forms"] or f[0] in FAMILIES]
assert len(RUNS) == 3 * len(FORMS) + 6 * len(FAMILIES)

_replays = {}
_exact_sincos = {}
# per case, the worst observed fraction of each bound over the forms that ran (printed; nothing is asserted on it)
worst_fraction = {}


def exact_sincos(x):
    """The correctly rounded sine and cosine of the double x (mpmath at 200 bits, rounded once to f64)."""
    if x not in _exact_sincos:
        import mpmath
        with mpmath.workprec(200):
            _exact_sincos[x] = (float(mpmath.sin(mpmath.mpf(x))), float(mpmath.cos(mpmath.mpf(x))))
    return _exact_sincos[x]


def start_model(oracle_lib, case):
    st = SR.CASES[case]["start"]
    if isinstance(st, str):   # the oracle's final model of that case: an input like any other
        return {k: v for k, v in SR.oracle_run(oracle_lib, st)["trace"][-1].items() if k != "dividers"}
    return None if st is None else dict(SR.zero_model(), **st)


def model_bits(recs):
    """The bits of every field of a list of records (the structures' padding left out)."""
    return np.array([[r[f] for f in ("cx", "cy", "dx", "dy", "rot", "div", "cnt") + SR.TOTALS] + list(r.get("dividers", ())) for r in recs],
                    np.float64).tobytes()


def note(case, key, frac):
    w = worst_fraction.setdefault(case, {})
    w[key] = max(w.get(key, 0.0), frac)


@pytest.mark.parametrize("case,form", RUNS, ids=["%s-%s" % (c, FORMS[i][0].replace(" ", "_").replace(",", "")) for c, i in RUNS])
def test_every_step_of_a_run(accel_mod, oracle_lib, case, form):
    name, opts, want_stat = FORMS[form]
    cs = SR.CASES[case]
    sl, scale = SR.get_slice(cs["slice"]), cs["scale"]
    what = "%s case, %s loop" % (case, name)
    start = start_model(oracle_lib, case)
    acc = new_accel(accel_mod, len(sl["t"]), opts, scale=scale, H=sl["H"], W=sl["W"])
    try:
        w = stage(acc, sl, scale)
        stat = {k: acc.get_stat(k) for k in want_stat}
        assert stat == want_stat, (what, stat, want_stat)
        if start is not None:
            acc.set_model(accel_mod.Model(**start))
            if "persistent" in want_stat:
                assert acc.get_stat("persistent") == want_stat["persistent"], what
        o = acc.default_opts()
        o.res_x, o.res_y, o.trace_cap, o.want_uv, o.max_iter = sl["res"][0], sl["res"][1], TRACE_CAP, 1, cs["max_iter"]
        rc, m, info = acc.run(o)
        raw = acc.get_trace(TRACE_CAP)
        if opts.get("binned") == 2:
            assert acc.get_stat("k1_threads") > 0 and acc.get_stat("k3_mode") >= 0, what   # the two-kernel loop's kernels ran
        else:
            assert acc.get_stat("k1_threads") == -1, what
        if "unpacked" in name and not opts.get("fused"):
            assert info.overflow_events > 0, what
        trace = SR.records(raw, lambda r: (r.x_divider, r.y_divider, r.rot_divider, r.div_divider))
        n = len(trace)
        print("%s: rc %d, %d iterations, %d launches, %d re-bins" % (what, rc, info.iterations, info.launches, info.rebins))
        assert 1 <= n < TRACE_CAP and [r.iteration for r in raw] == list(range(1, n + 1)), (what, n)

        # ---- sine and cosine: the device's own, of the recorded angles
        angles = np.array([-r["total_rot"] for r in trace])
        sn, cn = acc.eval_sincos(angles, table=False)
        sn_t, cn_t = acc.eval_sincos(angles, table=True)
        for k in range(n):
            a = float(angles[k])
            assert sn[k].tobytes() == sn_t[k].tobytes() and cn[k].tobytes() == cn_t[k].tobytes(), \
                "%s, iteration %d: sin / cos of %.17g differ between the table and the non-table variant" % (what, k + 1, a)
            es, ec = exact_sincos(a)
            ds, dc = X.ulp_distance64(float(sn[k]), es), X.ulp_distance64(float(cn[k]), ec)
            assert ds <= 1 and dc <= 1, ("%s, iteration %d: sin / cos of %.17g: got %.17g / %.17g, correctly rounded %.17g / %.17g, "
                                         "%d / %d ulp (bound 1)" % (what, k + 1, a, sn[k], cn[k], es, ec, ds, dc))
            note(case, "sincos_ulp", max(ds, dc))
        start_sc = None if start is None else (math.sin(-start["total_rot"]), math.cos(-start["total_rot"]))

        # ---- the replay, cached on what it is built from
        key = (case, model_bits(trace), sn.tobytes(), cn.tobytes())
        if key not in _replays:
            _replays[key] = SR.replay(sl, w, scale, trace, (sn, cn), start=start, start_sincos=start_sc)
        rp = _replays[key]

        # ---- every iteration
        ctl = SR.Control(max_iter=o.max_iter, hard_cap=o.hard_iter_cap, what=what)
        for k, (rec, st) in enumerate(zip(trace, rp["steps"])):
            at = "%s, iteration %d" % (what, k + 1)
            ref, exp = st["ref"], st["exp"]
            assert rec["cnt"] == ref["cnt"], "%s: valid-pixel count got %d want %d" % (at, rec["cnt"], ref["cnt"])
            for f in SR.MOMENTS:
                d, b = abs(rec[f] - ref[f]), st["mbound"][f]
                assert d <= b, "%s: %s got %.17g want %.17g, off by %.3e (bound %.3e)" % (at, f, rec[f], ref[f], d, b)
                note(case, f, d / b)
            for f in ("total_dx", "total_dy"):
                d = X.ulp_distance64(rec[f], exp[f])
                assert d == 0 and rec[f] == exp[f], "%s: %s got %.17g want %.17g, %d ulp off (must be bit-equal)" % (at, f, rec[f], exp[f], d)
            for f in ("total_rot", "total_div"):
                d, b = abs(rec[f] - exp[f]), st["sbound"][f]
                assert d <= b, "%s: %s got %.17g want %.17g, off by %.3e (bound %.3e)" % (at, f, rec[f], exp[f], d, b)
                note(case, f, d / b)
            for f in ("cx", "cy"):
                d, b = X.ulp_distance64(rec[f], exp[f]), st["sbound"][f + "_ulp"]
                assert d <= b, "%s: %s got %.17g want %.17g, %d ulp off (bound %d)" % (at, f, rec[f], exp[f], d, b)
                note(case, f + "_ulp", d / b)
            assert not ctl.done, "%s: the device went on after Control stopped (%s at iteration %d)" % (at, ctl.reason, ctl.it)
            want_div = tuple(float(v) for v in ctl.step(rec["dx"], rec["dy"], rec["rot"], rec["div"]))   # (raises if undecidable)
            assert rec["dividers"] == want_div, "%s: dividers got %s want %s" % (at, rec["dividers"], want_div)

        # ---- the stop
        assert ctl.done, "%s: the device stopped after %d iterations, Control goes on" % (what, n)
        want_rc = accel_mod.BF_ERR_NOCONV if ctl.rc == -2 else ctl.rc
        assert (info.iterations, rc, info.rc) == (ctl.it, want_rc, want_rc), \
            "%s: stop got (%d iterations, rc %d / %d) want (%d, %d) by %s" % (what, info.iterations, rc, info.rc, ctl.it, want_rc, ctl.reason)
        got_div = (info.x_divider, info.y_divider, info.rot_divider, info.div_divider)
        assert got_div == tuple(float(v) for v in ctl.dividers), "%s: bf_run_info dividers got %s want %s" % (what, got_div, ctl.dividers)
        assert model_bits([SR.model_dict(m)]) == model_bits([SR.model_dict(raw[-1].model)]), "%s: the returned model is not the last trace record" % what
        if cs["max_iter"] > 0:
            assert ctl.reason == "max_iter" and n == cs["max_iter"] + 1, (what, ctl.reason, n)
        if case == "large_angle":   # sincos_large at every update
            assert np.abs(angles).min() > 0.25, what
        if case == "rotation":
            assert np.abs(angles).max() > 3e-3, what

        # ---- after the run
        got = acc.writeout_events()
        for f, g in zip(("pr_x", "pr_y", "nx", "ny"), got):
            bad = np.nonzero(g != rp[f])[0]
            assert len(bad) == 0 and np.array_equal(g.view(np.uint64), rp[f].view(np.uint64)), \
                "%s: %s after the run differs at %d events; first: event %d got %.17g want %.17g" % (
                    what, f, len(bad), bad[0] if len(bad) else -1, g[bad[0]] if len(bad) else 0, rp[f][bad[0]] if len(bad) else 0)
        u, v = acc.compute_uv()
        wu, wv = SR.compute_uv(rp["nx"], rp["ny"])
        np.testing.assert_allclose(u, wu, rtol=1e-14, atol=0, err_msg=what)
        np.testing.assert_allclose(v, wv, rtol=1e-14, atol=0, err_msg=what)
        check_images(acc, dict(sl, kind=case), w, scale, what + ", after the run")
    finally:
        acc.close()
    print("%s: stop by %s after %d iterations, dividers %s; worst fraction of each bound so far: %s" %
          (what, ctl.reason, ctl.it, tuple(float(d) for d in ctl.dividers), {k: "%.2e" % v for k, v in sorted(worst_fraction[case].items())}))
