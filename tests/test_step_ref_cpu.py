"""tests/step_ref.py proven on the CPU, on the oracle's own traces, before any GPU test relies on it (no GPU needed).

For every case of step_ref.CASES (the runs tests/test_gpu_steps.py holds the device to), on oracle/bf_oracle.c's trace:
* the teacher-forced replay (every warp rebuilt from the recorded totals, centre and libm's sine of the recorded angle) gives the
  oracle's final pr_x, pr_y, nx, ny bit for bit;
* exact_ref's valid-pixel count equals the oracle's at every iteration up to the oracle's first order-noise difference (its f32
  sums in container order can put a pixel's mean time on the other side of 1e-6), which on the cold cases comes no earlier than
  iteration 9, the bar tests/test_gpu_forced_vs_oracle.py holds; up to there cx, cy are expected_step's bits;
* expected_step gives the oracle's four totals bit for bit at EVERY iteration (it is the oracle's own arithmetic, fed the
  oracle's own dx .. div and previous totals);
* Control, fed the recorded dx .. div, reproduces the oracle's dividers at every iteration, its itercount and its rc; no step of
  any case is undecidable;
* each case reaches what it is there for (PURPOSE).

The device's way of forming a step (reciprocals of the dividers and of the scale, model_update_wave) is restated here in plain
Python (`device_step`) and shown to lie inside step_bound on every record of every case, with total_dx / total_dy bit-equal -- so
the bound is one a correct device meets -- and the mutations below, made to that restatement, to fall outside it.

Mutations, each caught on the oracle's trace:
* the sign of the angle flipped: the valid-pixel count and the final events differ (rotation case);
* the post-doubling divider used in the accumulation: the totals differ at every iteration that doubles a divider;
* the sign flips applied before the max_iter test: the dividers at the stop differ from the recorded ones (max_iter case);
* old_* updated on the stopping iteration: Control's old_* after the stop are no longer the floats of the record BEFORE the last.
  This one shows only in the state: old_* is read by the sign tests of the NEXT step and a stopped loop has none (bf_run resets
  it), so no output of a run -- the oracle's or the device's -- depends on it.
"""
import math

import numpy as np
import pytest

import exact_ref as X
import step_ref as SR

F32 = np.float32
COLD = [n for n, c in SR.CASES.items() if c["start"] is None]

# What each case is there for, asserted on the oracle's run: the stop reason, the least number of doublings per channel
# (x, y, rot, div), the range of |angle| = |total_rot| over the trace, and the least number of iterations.
PURPOSE = {
    "translation": dict(reason="converged", doublings=(0, 1, 1, 1), iters=10),
    "translation_scale1": dict(reason="converged", doublings=(2, 10, 1, 1), iters=200),
    "translation_scale5": dict(reason="converged", doublings=(1, 0, 1, 1), iters=15),
    "rotation": dict(reason="converged", doublings=(3, 2, 0, 3), iters=30, angle_above=3e-3),
    "divergence": dict(reason="converged", doublings=(2, 2, 1, 0), iters=30, div_above=1e-3),
    "both": dict(reason="converged", doublings=(1, 3, 0, 0), iters=25, angle_above=1e-3, div_above=1e-3),
    "warm_start": dict(reason="converged", doublings=(1, 1, 0, 1), iters=3, iters_at_most=8),
    "max_iter": dict(reason="max_iter", doublings=(0, 0, 2, 0), iters=SR.MAX_ITER_CAP + 1, iters_at_most=SR.MAX_ITER_CAP + 1),
    "large_angle": dict(reason="max_iter", doublings=(0, 0, 0, 0), iters=9, iters_at_most=9, every_angle_above=0.25),
}


@pytest.fixture(scope="module")
def proven(oracle_lib):
    """Per case, computed once: the oracle's run and the teacher-forced replay of its trace."""
    cache = {}

    def get(name):
        if name not in cache:
            o = SR.oracle_run(oracle_lib, name)
            sc = SR.libm_sincos([-r["total_rot"] for r in o["trace"]])
            st = o["start"]
            st_sc = None if st is None else (math.sin(-st["total_rot"]), math.cos(-st["total_rot"]))
            cache[name] = (o, SR.replay(o["sl"], o["window"], o["scale"], o["trace"], sc, start=st, start_sincos=st_sc))
        return cache[name]
    return get


def first_count_difference(o, rp):
    return next((k for k, s in enumerate(rp["steps"]) if s["ref"]["cnt"] != o["trace"][k]["cnt"]), len(o["trace"]))


@pytest.mark.parametrize("name", list(SR.CASES))
def test_replay_gives_the_oracles_events_and_counts(proven, name):
    o, rp = proven(name)
    for k in ("pr_x", "pr_y", "nx", "ny"):
        assert np.array_equal(rp[k], o[k]), (name, k, int((rp[k] != o[k]).sum()))
    k_g = first_count_difference(o, rp)
    print("%s: %d iterations, valid-pixel counts equal for the first %d" % (name, len(o["trace"]), k_g))
    if name in COLD:
        assert k_g >= min(9, len(o["trace"])), (name, k_g)
    assert k_g >= 1, name
    for k in range(k_g):
        rec, st = o["trace"][k], rp["steps"][k]
        assert rec["cx"] == st["exp"]["cx"] and rec["cy"] == st["exp"]["cy"], (name, k)
        # (dx .. div are not compared: the oracle takes them from ITS time image, f32 sums in container order, 1e-6 from the
        # exact one; that bar is tests/test_exact_ref_cpu.py's.  The device's are held to exact_ref.moment_bound.)
    u, v = SR.compute_uv(rp["nx"], rp["ny"])
    assert np.isfinite(u).all() and np.isfinite(v).all()


@pytest.mark.parametrize("name", list(SR.CASES))
def test_expected_step_gives_the_oracles_totals(proven, name):
    o, rp = proven(name)
    for k, (rec, st) in enumerate(zip(o["trace"], rp["steps"])):
        for f in SR.TOTALS:
            assert X.ulp_distance64(rec[f], st["exp"][f]) == 0 and rec[f] == st["exp"][f], (name, k, f, rec[f], st["exp"][f])


@pytest.mark.parametrize("name", list(SR.CASES))
def test_control_reproduces_the_oracles_loop(oracle_lib, proven, name):
    o, _ = proven(name)
    c, seen = SR.run_control(o["trace"], max_iter=SR.CASES[name]["max_iter"], hard_cap=200000, what=name)   # (raises if undecidable)
    assert c.done and c.it == o["loop"].itercount == len(o["trace"]) and c.rc == o["rc"] == 0, (name, c.it, c.reason)
    assert seen == [r["dividers"] for r in o["trace"]], name
    lp = o["loop"]
    assert tuple(float(d) for d in c.dividers) == (lp.x_divider, lp.y_divider, lp.rot_divider, lp.div_divider)
    # what the case is there for
    p = PURPOSE[name]
    angles = [abs(r["total_rot"]) for r in o["trace"]]
    print("%s: %d iterations, stop by %s, doublings %s, |angle| up to %.3e, |total_div| up to %.3e" %
          (name, c.it, c.reason, c.doublings, max(angles), max(abs(r["total_div"]) for r in o["trace"])))
    assert c.reason == p["reason"], (name, c.reason)
    assert all(g >= w for g, w in zip(c.doublings, p["doublings"])), (name, c.doublings)
    assert p["iters"] <= c.it <= p.get("iters_at_most", 4096), (name, c.it)
    if "angle_above" in p:
        assert max(angles) > p["angle_above"], (name, max(angles))
    if "div_above" in p:
        assert max(abs(r["total_div"]) for r in o["trace"]) > p["div_above"], name
    if "every_angle_above" in p:   # sincos_large at the warm start and in every update
        assert min(angles) > p["every_angle_above"] and abs(o["start"]["total_rot"]) > p["every_angle_above"], (name, min(angles))
        assert min(r["cnt"] for r in o["trace"]) > 19000, name   # nothing degenerate: the image keeps its pixels


def test_max_iter_stops_where_the_uncapped_run_doubles(oracle_lib, proven):
    """The capped run stops at iteration MAX_ITER_CAP + 1, where the uncapped run (the translation case) doubles a divider; the
    capped run's dividers there are those of the iteration before (:94-96 come before :98-101)."""
    capped, _ = proven("max_iter")
    free, _ = proven("translation")
    k = SR.MAX_ITER_CAP
    assert len(capped["trace"]) == k + 1 < len(free["trace"])
    assert free["trace"][k]["dividers"] != free["trace"][k - 1]["dividers"]
    assert capped["trace"][k]["dividers"] == capped["trace"][k - 1]["dividers"] == free["trace"][k - 1]["dividers"]
    for f in SR.TOTALS + SR.MOMENTS:   # the same trajectory up to the stop
        assert capped["trace"][k][f] == free["trace"][k][f], f


def test_hard_cap_and_divider_limit_branches(oracle_lib, proven):
    """The two stops no case of the table takes.  hard_cap: the oracle's translation run capped at 7 iterations returns -2 after
    the sign flips of that iteration, and so does Control.  The divider limit (optimizer_rolling.h:76-79), which 64 searched
    slices never reached (step_ref's docstring), on a made-up sequence: alternating signs double every divider at every step
    until all four are past their limits (x, y: 512 after 9 doublings), before any ratio is small enough to converge."""
    o = SR.oracle_run(oracle_lib, "translation", hard_cap=7)
    assert o["rc"] == -2 and o["loop"].itercount == 7
    c, seen = SR.run_control(o["trace"], hard_cap=7)
    assert (c.reason, c.rc, c.it) == ("hard_cap", -2, 7) and seen == [r["dividers"] for r in o["trace"]]
    assert o["trace"][6]["dividers"] == SR.oracle_run(oracle_lib, "translation")["trace"][6]["dividers"]   # flips applied
    c = SR.Control()
    k = 0
    while not c.done:
        sgn = -1.0 if k % 2 else 1.0
        c.step(sgn * 1e3, sgn * 1e3, sgn * 1e7, sgn * 1e7)
        k += 1
    assert (c.reason, c.rc, c.it) == ("dividers", 0, 10), (c.reason, c.it)
    assert tuple(float(d) for d in c.dividers) == (512.0, 512.0, 5120000.0, 5120000.0)


def test_an_undecidable_convergence_test_is_reported():
    """A ratio within 4 ulp of its threshold raises, naming the iteration and the channel; 40 ulp away on either side it is
    decided, the way the comparison says."""
    def value(i, steps, towards):
        d = float(SR.START_DIVIDERS[i])
        r = SR.THRESHOLDS[i]
        for _ in range(steps):
            r = math.nextafter(r, towards)
        vals = [0.0, 0.0, 0.0, 0.0]
        vals[i] = -r * d   # (the test takes the absolute value)
        return vals, X.ulp_distance64(abs(vals[i] / d), SR.THRESHOLDS[i])
    for i in range(4):
        for towards in (0.0, 1.0):
            vals, dist = value(i, 2, towards)
            assert dist <= SR.UNDECIDABLE_ULPS
            with pytest.raises(SR.Undecidable, match="made-up: INCONCLUSIVE at iteration 1: .%s / divider" % SR.MOMENTS[i]):
                SR.Control(what="made-up").step(*vals)
            vals, dist = value(i, 40, towards)
            assert dist > SR.UNDECIDABLE_ULPS
            c = SR.Control()
            c.step(*vals)
            assert (c.reason == "converged") == (towards == 0.0) and c.done == (towards == 0.0), (i, towards)
            if not c.done:
                assert c.old == tuple(F32(v) for v in vals)


# ---- the device's arithmetic, restated, against step_bound -------------------------------------------------------------------------

def device_step(prev, rec, ref, window, scale, dividers):
    """model_update_wave's way: one division gives the reciprocals, the update multiplies by them."""
    inv = [1.0 / float(F32(d)) for d in dividers]
    inv_scale = 1.0 / float(scale)
    out = {"total_" + f: prev["total_" + f] + rec[f] * inv[i] for i, f in enumerate(SR.MOMENTS)}
    out["cx"] = (ref["cx"] - float(window["x_shift"])) * inv_scale
    out["cy"] = (ref["cy"] - float(window["y_shift"])) * inv_scale
    return out


def within_step_bound(got, st):
    """The assertion tests/test_gpu_steps.py makes on a record, as a predicate: (ok, field that failed)."""
    for f in SR.TOTALS:
        if not abs(got[f] - st["exp"][f]) <= st["sbound"][f]:
            return False, f
    for f in ("total_dx", "total_dy"):
        if X.ulp_distance64(got[f], st["exp"][f]) != 0:
            return False, f
    for f in ("cx", "cy"):
        if X.ulp_distance64(got[f], st["exp"][f]) > st["sbound"][f + "_ulp"]:
            return False, f
    return True, None


@pytest.mark.parametrize("name", list(SR.CASES))
def test_the_devices_arithmetic_lies_inside_step_bound(proven, name):
    """Reciprocal products instead of divisions, on every record of the oracle's trace: inside step_bound, total_dx / total_dy
    bit-equal; and the bound is tight (a few 1e-16 of the total), so a wrong divider, a dropped term or a sign cannot hide."""
    o, rp = proven(name)
    prev, dividers = (o["start"] or SR.zero_model()), SR.START_DIVIDERS
    worst = 0.0
    for k, (rec, st) in enumerate(zip(o["trace"], rp["steps"])):
        got = device_step(prev, rec, st["ref"], o["window"], o["scale"], dividers)
        ok, f = within_step_bound(got, st)
        assert ok, (name, k, f, got[f], st["exp"][f])
        for f in ("total_rot", "total_div"):
            b = st["sbound"][f]
            # 4 u |q| < 4 ulp(q), plus one ulp of the total (two where the sum reaches the next binade)
            assert b <= 6 * math.ulp(max(abs(st["exp"][f]), abs(st["exp"]["q_" + f[6:]]))), (name, k, f, b)
            worst = max(worst, abs(got[f] - st["exp"][f]) / b)
        prev, dividers = rec, rec["dividers"]
    print("%s: the restated device arithmetic uses at most %.2f of step_bound" % (name, worst))


# ---- mutations ------------------------------------------------------------------------------------------------------------------------

def test_mutation_angle_sign_is_caught(proven):
    """-total_rot -> +total_rot (the sine changes sign): the replay no longer gives the oracle's valid-pixel counts nor its
    final events, on the rotation case and, with |angle| = 0.3, on the large-angle case at the first record."""
    for name in ("rotation", "large_angle"):
        o, good = proven(name)
        sc = SR.libm_sincos([-r["total_rot"] for r in o["trace"]])
        st = o["start"]
        st_sc = None if st is None else (math.sin(-st["total_rot"]), math.cos(-st["total_rot"]))
        bad = SR.replay(o["sl"], o["window"], o["scale"], o["trace"], sc, start=st, start_sincos=st_sc, angle_sign=-1.0)
        k_good, k_bad = first_count_difference(o, good), first_count_difference(o, bad)
        print("%s: counts equal for %d iterations, with the angle's sign flipped for %d" % (name, k_good, k_bad))
        assert k_bad < k_good and k_bad < 9, (name, k_bad, k_good)
        assert not np.array_equal(bad["pr_x"], o["pr_x"]) and not np.array_equal(bad["nx"], o["nx"])


def test_mutation_post_doubling_divider_is_caught(proven):
    """Accumulating with the dividers recorded AFTER the step: the totals leave the oracle's at every iteration that doubles a
    divider of a non-zero moment, and the device's arithmetic mutated this way leaves step_bound there."""
    for name in ("translation", "rotation"):
        o, good = proven(name)
        sc = SR.libm_sincos([-r["total_rot"] for r in o["trace"]])
        bad = SR.replay(o["sl"], o["window"], o["scale"], o["trace"], sc, late_dividers=True)
        doubling = [k for k in range(1, len(o["trace"])) if o["trace"][k]["dividers"] != o["trace"][k - 1]["dividers"]]
        assert len(doubling) >= 3, name
        caught = [k for k, (rec, st) in enumerate(zip(o["trace"], bad["steps"])) if any(rec[f] != st["exp"][f] for f in SR.TOTALS)]
        assert caught == doubling, (name, caught, doubling)
        prev = SR.zero_model()
        outside = []
        for k, (rec, st) in enumerate(zip(o["trace"], good["steps"])):
            got = device_step(prev, rec, st["ref"], o["window"], o["scale"], rec["dividers"])
            if not within_step_bound(got, st)[0]:
                outside.append(k)
            prev = rec
        assert outside == doubling, (name, outside, doubling)


def test_mutation_flips_before_max_iter_is_caught(proven):
    o, _ = proven("max_iter")
    good, seen = SR.run_control(o["trace"], max_iter=SR.MAX_ITER_CAP)
    bad, seen_bad = SR.run_control(o["trace"], max_iter=SR.MAX_ITER_CAP, mutate="flips_before_max_iter")
    assert good.reason == bad.reason == "max_iter" and good.it == bad.it == SR.MAX_ITER_CAP + 1
    assert seen == [r["dividers"] for r in o["trace"]]
    assert seen_bad[:-1] == seen[:-1] and seen_bad[-1] != o["trace"][-1]["dividers"], (seen_bad[-1], o["trace"][-1]["dividers"])


def test_mutation_old_on_the_stopping_iteration_is_caught(proven):
    """old_* are taken (:86-89) after the convergence test and before the next step, so after a run they are the floats of the
    record before the last.  The mutated Control holds the last record's instead.  (State only: see the module docstring.)"""
    for name in ("translation", "max_iter"):
        o, _ = proven(name)
        mi = SR.CASES[name]["max_iter"]
        want = tuple(F32(o["trace"][-2][f]) for f in SR.MOMENTS)
        last = tuple(F32(o["trace"][-1][f]) for f in SR.MOMENTS)
        assert want != last
        good, _ = SR.run_control(o["trace"], max_iter=mi)
        bad, _ = SR.run_control(o["trace"], max_iter=mi, mutate="old_on_stop")
        assert good.old == want and bad.old == last, name
        assert good.dividers == bad.dividers and good.it == bad.it   # nothing a run returns tells them apart
