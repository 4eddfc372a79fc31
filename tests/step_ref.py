"""One iteration step of the descent loop and the control of run(), restated exactly -- TEST INFRASTRUCTURE ONLY.

Every loop form of the library runs ONE definition of the per-iteration update (model_update_wave + model_update_rest,
better_flow_amd/csrc/bf_device_fns.h), so that the forms agree bit for bit says nothing about it.  This module states what a
step must give, so that a trace -- the oracle's or the device's -- can be checked record by record:

    replay_warp     np_ref.warp's arithmetic (event.h:99-110,164-168) with sin / cos passed in: the caller decides whose sine
                    it is (the host's libm for the oracle and for bf_set_model, the device's own for the device loops)
    expected_step   optimizer_rolling.h:328-346 from the recorded dx, dy, rot, div of step k and the totals after step k - 1
    step_bound      how far a correct device may be from expected_step (derived below, not measured)
    Control         the state machine of run(), optimizer_rolling.h:61-101, as oracle/bf_oracle.c's bfo_run states it
    replay          the whole check of a trace, TEACHER-FORCED: every step starts from the values the trace itself recorded
                    after the step before, so nothing accumulates from one step to the next

Teacher forcing.  The recurrent state of the loop is 8 bytes per event, the two f32 products of apply_project
(event.h:164-168).  The warp of step k is built from total_dx, total_dy, total_div, total_rot, cx and cy, all of which the
trace records as f64.  With those recorded parameters (and the sine and cosine of the recorded angle) np_ref.warp's arithmetic
gives the events' pr bit for bit, so the integer planes, the time image, the valid-pixel count and the moments
(tests/exact_ref.py) of the NEXT step have one right answer however far the trajectory as a whole has drifted from another
implementation's; no pixel-crossing argument is needed.

`math.sin` / `math.cos` (libm) are what "the host's sine" means here, not numpy's.

CASES lists the runs tests/test_step_ref_cpu.py proves the reference on and tests/test_gpu_steps.py holds the device to.

No run that ends by the divider limit (optimizer_rolling.h:76-79) is among them: a search on the CPU oracle over 64 slices
(synth.make_slice seeds 1 .. 40 at 60 x 80, 20 000 events, scale 1; seeds 1 .. 12 at scale 3; seeds 1 .. 12 at 48 x 64,
12 000 events, scale 5; at most 3000 iterations each) found none, every run ended by convergence.  Control reproduced the
oracle's dividers in all 64.  The divider assertion of config 2 (tests/test_gpu_geometries.py) stays that branch's only cover on
the device; Control's own branch is exercised on a made-up sequence in tests/test_step_ref_cpu.py.
"""
import math

import numpy as np

import exact_ref as X

F32 = np.float32
U = X.U
TOTALS = ("total_dx", "total_dy", "total_rot", "total_div")
MOMENTS = ("dx", "dy", "rot", "div")
# the convergence thresholds of optimizer_rolling.h:81-84, in the order x, y, rot, div
THRESHOLDS = (1e-5, 1e-5, 1e-4, 1e-1)
# the divider limits of optimizer_rolling.h:76-79
LIMITS = (32 * 10, 32 * 10, 32 * 1000, 32 * 1000)
START_DIVIDERS = (F32(1), F32(1), F32(10000), F32(10000))
UNDECIDABLE_ULPS = 4


class Undecidable(AssertionError):
    """A convergence test whose ratio lies within UNDECIDABLE_ULPS of its threshold: a correct device (which multiplies by a
    rounded reciprocal, <= 2 ulp from the quotient: step_bound) may decide either way, so the case proves nothing."""


def model_dict(m):
    """A trace record's model (ctypes, the oracle's or the library's) as a dict of Python floats."""
    return {k: getattr(m, k) for k in ("cx", "cy", "dx", "dy", "rot", "div", "cnt") + TOTALS}


def zero_model():
    return dict(cx=0.0, cy=0.0, dx=0.0, dy=0.0, rot=0.0, div=0.0, cnt=0, total_dx=0.0, total_dy=0.0, total_rot=0.0, total_div=0.0)


def warp_params(m):
    """(dnx, dny, cx, cy, div) and the angle of the warp a model asks for (optimizer_rolling.h:340-344, :289-299)."""
    return (-m["total_dx"], -m["total_dy"], m["cx"], m["cy"], m["total_div"]), -m["total_rot"]


def replay_warp(sl, pr_x, pr_y, params, s, c):
    """Event::project_4param_reinit + apply_project (event.h:99-110,164-168) on the previous pr, as np_ref.warp states them
    (every operation a separate IEEE operation, in its order), with the sine `s` and cosine `c` of the angle given.
    params = (dnx, dny, cx, cy, div).  Returns pr_x, pr_y, nx, ny (f64 arrays)."""
    dnx, dny, cx, cy, div = (np.float64(v) for v in params)
    s, c = np.float64(s), np.float64(c)
    rx, ry = pr_x - cx, pr_y - cy
    qx = c * rx - s * ry
    qy = s * rx + c * ry
    nx = ((-qx) * div + (qx - rx)) + dnx
    ny = ((-qy) * div + (qy - ry)) + dny
    kx = (nx.astype(F32).astype(np.float64) / 127.0).astype(F32)
    ky = (ny.astype(F32).astype(np.float64) / 127.0).astype(F32)
    ft = sl["t"].astype(F32)
    px = (kx * ft).astype(np.float64)
    py = (ky * ft).astype(np.float64)
    npr_x = sl["fr_x"].astype(F32).astype(np.float64) - px / 10000.0
    npr_y = sl["fr_y"].astype(F32).astype(np.float64) - py / 10000.0
    return npr_x, npr_y, nx, ny


def compute_uv(nx, ny):
    """Event::compute_uv, event.h:135-142: speed = |n| / (127 / 100000) along n; 0 where n is 0."""
    ln = np.hypot(nx, ny)
    speed = ln / (127.0 / float(1000000000 // (1 * 10000)))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ln == 0, 0.0, speed * nx / ln)
        v = np.where(ln == 0, 0.0, speed * ny / ln)
    return u, v


def expected_step(prev, moments_dev, window, scale, dividers):
    """What optimizer_rolling.h:328-346 gives for one step.

    prev         the totals after the step before (a model dict: the start model for step 0)
    moments_dev  the recorded dx, dy, rot, div of this step (f64, taken as they are: whether THEY are right is
                 exact_ref.moment_bound's business) and cx_img, cy_img, the centre of mass in image coordinates
                 (object_model.cpp:103-126: an exact integer sum divided once, so exact_ref.moments' cx, cy)
    dividers     (x, y, rot, div) as np.float32: the dividers the step STARTED with (the ones recorded after the step before)
    total_* = total_prev + value / (double)divider (object_model.h:48-53); cx = (cx_img - x_shift) / scale with the DOUBLE
    shift, cy alike.  Returns the four totals, cx, cy, the four quotients q_dx .. q_div and the dividers as doubles."""
    w = X.as_window(window)
    xd, yd, rd, dd = (float(F32(d)) for d in dividers)
    q = dict(q_dx=moments_dev["dx"] / xd, q_dy=moments_dev["dy"] / yd, q_rot=moments_dev["rot"] / rd, q_div=moments_dev["div"] / dd)
    out = dict(q)
    for k in MOMENTS:
        out["total_" + k] = prev["total_" + k] + q["q_" + k]
    out["cx"] = (moments_dev["cx_img"] - float(w["x_shift"])) / float(scale)
    out["cy"] = (moments_dev["cy_img"] - float(w["y_shift"])) / float(scale)
    out["dividers"] = (xd, yd, rd, dd)
    return out


def is_pow2(d):
    return d > 0 and math.frexp(d)[0] == 0.5


def step_bound(exp):
    """How far a correct device may be from expected_step(...) = `exp` -- derived, not measured.  u = 2^-53.

    The device does not divide by the dividers and the scale: one lane-parallel division gives RN(1 / divider) and
    RN(1 / scale), and the update multiplies by them (model_update_wave).  Every accumulation rounds once on either side.

    * total_dx, total_dy.  The x and y dividers start at 1 and only ever double, so they are powers of two (asserted here).
      Then 1 / d is exact, v * (1 / d) and v / d are the same real number, itself a double (short of underflow, 2^-1022),
      and total_prev + it rounds once to the same double: the device's total_dx and total_dy must equal the reference's BIT
      FOR BIT.  Bound 0.
    * total_rot, total_div.  The dividers are 10000 x 2^k, no powers of two.  inv = (1 / d)(1 + e1), q_dev = v inv (1 + e2)
      and q_ref = (v / d)(1 + e3) with |e_i| <= u, so |q_dev - q_ref| <= (3 u + 3 u^2 + u^3) |v / d| <= 4 u |q_ref| (the last
      step pays for the second-order terms and for q_ref's own rounding: "a few ulp of the quotient").  Each side then rounds
      total_prev + q once, by at most half an ulp of its own result, together at most one ulp of the larger:
          |total_dev - total_ref| <= 4 u |q_ref| + ulp(|total_ref| + 4 u |q_ref|).
    * cx, cy.  a = RN(cx_img - shift) is the same double on both sides (cx_img is an exact integer sum divided once, the same
      division on both sides).  a RN(1 / s) = (a / s)(1 + e1): the two real numbers that are then rounded lie less than u |a / s|
      < 1 ulp apart, and rounding is monotone, so the results are neighbours at most: 1 ulp, 2 where a power of two lies between
      them (the ulps below it are half as large).  <= 2 ulp, the bar tests/test_gpu_exact.py::check_model holds iteration 0 to;
      0 ulp at scale 1.
    Returns the absolute bounds of the four totals and cx_ulp, cy_ulp."""
    xd, yd, _, _ = exp["dividers"]
    assert is_pow2(xd) and is_pow2(yd), (xd, yd)
    out = dict(total_dx=0.0, total_dy=0.0, cx_ulp=2, cy_ulp=2)
    for k in ("rot", "div"):
        dq = 4.0 * U * abs(exp["q_" + k])
        out["total_" + k] = dq + math.ulp(abs(exp["total_" + k]) + dq)
    return out


class Control:
    """run(), optimizer_rolling.h:61-101, as a state machine fed one step's recorded dx, dy, rot, div (doubles) at a time, in
    the order bfo_run states: [max_iter, :94-96] before [the four sign tests against the FLOAT old_*, :98-101] before
    [hard_cap] before [the divider limit, :76-79] before [the convergence test on value / (double)divider, :81-84]; old_* is
    taken (:86-89) only when the loop goes on.

    After step(): .dividers (np.float32 x 4), .it, .done, .reason ("converged" / "dividers" / "max_iter" / "hard_cap" / None),
    .rc (0, or -2 at the hard cap, as bfo_run returns it) and .old (the four floats, None before the first step).

    A convergence test within UNDECIDABLE_ULPS of its threshold raises Undecidable naming the step and the channel.
    `mutate` (tests only) is one of "old_on_stop" (old_* taken on the stopping iteration too) and "flips_before_max_iter"
    (the sign tests applied before the max_iter test): what tests/test_step_ref_cpu.py shows a trace to tell apart."""

    def __init__(self, max_iter=-1, hard_cap=0, mutate=None, what=""):
        self.dividers = START_DIVIDERS
        self.max_iter, self.hard_cap, self.mutate, self.what = max_iter, hard_cap, mutate, what
        self.it, self.done, self.reason, self.rc, self.old = 0, False, None, 0, None
        self.doublings = [0, 0, 0, 0]

    def _stop(self, reason, rc=0):
        self.done, self.reason, self.rc = True, reason, rc

    def _flips(self, vals):
        d = list(self.dividers)
        for i in range(4):
            if vals[i] * float(self.old[i]) < 0:          # double * float -> double
                d[i] = F32(d[i] * F32(2))                 # float *= 2
                self.doublings[i] += 1
        self.dividers = tuple(d)

    def _converged(self, vals):
        ok = True
        for i, name in enumerate(MOMENTS):
            ratio = abs(vals[i] / float(self.dividers[i]))
            if X.ulp_distance64(ratio, THRESHOLDS[i]) <= UNDECIDABLE_ULPS:
                raise Undecidable("%s: INCONCLUSIVE at iteration %d: |%s / divider| = %.17g is within %d ulp of its threshold %g"
                                  % (self.what, self.it, name, ratio, UNDECIDABLE_ULPS, THRESHOLDS[i]))
            ok = ok and ratio < THRESHOLDS[i]
        return ok

    def step(self, dx, dy, rot, div):
        assert not self.done, "step() after the loop has stopped"
        vals = (float(dx), float(dy), float(rot), float(div))
        self.it += 1
        if self.it > 1:
            if self.mutate == "flips_before_max_iter":
                self._flips(vals)
            if self.max_iter > 0 and self.it > self.max_iter:
                self._stop("max_iter")
            else:
                if self.mutate != "flips_before_max_iter":
                    self._flips(vals)
                if self.hard_cap > 0 and self.it >= self.hard_cap:
                    self._stop("hard_cap", -2)
        if not self.done:
            if not any(float(d) < lim for d, lim in zip(self.dividers, LIMITS)):
                self._stop("dividers")
            elif self._converged(vals):
                self._stop("converged")
        if not self.done or self.mutate == "old_on_stop":
            self.old = tuple(F32(v) for v in vals)
        return self.dividers


def replay(sl, window, scale, trace, sincos, start=None, start_sincos=None, what="", angle_sign=1.0, late_dividers=False):
    """The teacher-forced check of a whole trace.

    sl        the slice: fr_x, fr_y (int), t (ns)
    trace     per step a dict: the model's fields and `dividers` (x, y, rot, div recorded AFTER the step)
    sincos    (sn, cs): per step k the sine and cosine of -total_rot of record k, as the implementation that made the trace
              evaluates them
    start     the model of a warm start (set_model) or None; start_sincos its (sin, cos) of -total_rot (the host's libm)
    Per step k it builds the image from the pr the PREVIOUS record's warp gives (the identity before step 0 of a cold run),
    takes exact_ref's planes, time image and moments, and forms expected_step from the record's own dx .. div and the previous
    record's totals and dividers.  Nothing is asserted here.  Returns a dict:
        steps   per step: ref (exact_ref.moments), mbound (exact_ref.moment_bound), exp (expected_step), sbound (step_bound)
        pr_x, pr_y, nx, ny   the events after the last record's warp
    (angle_sign and late_dividers are the mutations tests/test_step_ref_cpu.py shows to be caught.)"""
    pr_x, pr_y = sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64)
    nx = ny = np.zeros(len(pr_x))
    prev = zero_model()
    if start is not None:
        prev = dict(start)
        prm, _ = warp_params(prev)
        pr_x, pr_y, nx, ny = replay_warp(sl, pr_x, pr_y, prm, angle_sign * start_sincos[0], start_sincos[1])
    dividers = START_DIVIDERS
    steps = []
    for k, rec in enumerate(trace):
        cnt, S = X.planes(pr_x, pr_y, sl["t"], window, scale)
        ref = X.moments(X.time_from_planes(cnt, S))
        mdev = dict(dx=rec["dx"], dy=rec["dy"], rot=rec["rot"], div=rec["div"], cx_img=ref["cx"], cy_img=ref["cy"])
        used = tuple(F32(d) for d in rec["dividers"]) if late_dividers else dividers
        exp = expected_step(prev, mdev, window, scale, used)
        steps.append(dict(ref=ref, mbound=X.moment_bound(ref) if ref["cnt"] else None, exp=exp, sbound=step_bound(exp)))
        prm, _ = warp_params(rec)
        pr_x, pr_y, nx, ny = replay_warp(sl, pr_x, pr_y, prm, angle_sign * sincos[0][k], sincos[1][k])
        prev, dividers = rec, tuple(F32(d) for d in rec["dividers"])
    return dict(steps=steps, pr_x=pr_x, pr_y=pr_y, nx=nx, ny=ny)


def libm_sincos(angles):
    return [math.sin(a) for a in angles], [math.cos(a) for a in angles]


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _synth(n, H, W, T, seed):
    from better_flow_amd import synth
    mv = synth.make_slice(n, H, W, T, seed=seed)
    return dict(H=H - 1, W=W - 1, res=(H, W), fr_x=mv["fr_x"], fr_y=mv["fr_y"], t=mv["t"])


def scene(rng, n, H, W, T, v, rot, div, inset=5):
    """tests/test_gpu_parity.py::test_run_to_convergence_with_rotation_and_divergence's generator (points that translate,
    rotate and diverge about the sensor centre) on an H x W sensor with an `inset`-pixel border."""
    npts = n // 16
    pr, pc = rng.uniform(inset, H - inset, npts), rng.uniform(inset, W - inset, npts)
    t = np.sort(rng.uniform(0, T, n))
    pick = rng.integers(0, npts, n)
    r0, c0 = pr[pick] - H / 2, pc[pick] - W / 2
    row = pr[pick] + (v[0] + div * r0 - rot * c0) * t
    col = pc[pick] + (v[1] + div * c0 + rot * r0) * t
    keep = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    return dict(H=H - 1, W=W - 1, res=(H, W), fr_x=np.floor(row[keep]).astype(np.int32), fr_y=np.floor(col[keep]).astype(np.int32),
                t=(t[keep] * 1e9).astype(np.int64))


SCENES = (("rotation", (-80.0, 120.0), 3.0, 0.0), ("divergence", (60.0, -40.0), 0.0, 2.5), ("both", (-50.0, 90.0), -2.0, 1.5))
_slices = {}


def get_slice(key):
    if key not in _slices and key in [s[0] for s in SCENES]:
        rng = np.random.default_rng(7)   # ONE generator drawn from in this order, as in the test the scenes come from
        for name, v, rot, div in SCENES:
            _slices[name] = scene(rng, 20000, 60, 80, 0.03, v, rot, div)
    if key not in _slices:
        _slices[key] = {
            "translation": lambda: _synth(20000, 60, 80, 0.03, 5),
            "translation48": lambda: _synth(12000, 48, 64, 0.03, 5),
            "next": lambda: _synth(20000, 60, 80, 0.03, 6),
            "short": lambda: _synth(20000, 60, 80, 0.001, 5),
        }[key]()
    return _slices[key]


# The runs.  slice: get_slice's key; start: None (cold), "translation" (warm start from the oracle's final model of that case) or a
# dict of model fields (set_model with the other fields 0); max_iter as bf_run_opts / bfo_run take it (<= 0: none);
# all_forms: every loop form of test_gpu_exact.FORMS runs it on the device (else the five families).
MAX_ITER_CAP = 5   # the uncapped translation run doubles the rot and the div divider at iteration 6 (asserted on the CPU)
CASES = {
    "translation": dict(slice="translation", scale=3, start=None, max_iter=0, all_forms=True),
    "translation_scale1": dict(slice="translation", scale=1, start=None, max_iter=0, all_forms=False),
    "translation_scale5": dict(slice="translation48", scale=5, start=None, max_iter=0, all_forms=False),
    "rotation": dict(slice="rotation", scale=3, start=None, max_iter=0, all_forms=True),
    "divergence": dict(slice="divergence", scale=3, start=None, max_iter=0, all_forms=False),
    "both": dict(slice="both", scale=3, start=None, max_iter=0, all_forms=False),
    "warm_start": dict(slice="next", scale=3, start="translation", max_iter=0, all_forms=False),
    "max_iter": dict(slice="translation", scale=3, start=None, max_iter=MAX_ITER_CAP, all_forms=False),
    "large_angle": dict(slice="short", scale=3, start=dict(cx=30.0, cy=40.0, total_rot=0.3), max_iter=8, all_forms=True),
}


def records(trace, dividers_of):
    """A ctypes trace as the list of dicts replay() takes."""
    out = []
    for r in trace:
        d = model_dict(r.model)
        d["dividers"] = tuple(float(v) for v in dividers_of(r))
        out.append(d)
    return out


_oracle_runs = {}


def oracle_run(oracle_lib, name, max_iter=None, hard_cap=200000):
    """The oracle's run of a case (cached): dict(sl, scale, window, start, rc, loop, trace (records), pr_x, pr_y, nx, ny)."""
    case = CASES[name]
    mi = case["max_iter"] if max_iter is None else max_iter
    key = (name, mi, hard_cap)
    if key in _oracle_runs:
        return _oracle_runs[key]
    sl = get_slice(case["slice"])
    start = case["start"]
    if isinstance(start, str):
        start = {k: v for k, v in oracle_run(oracle_lib, start)["trace"][-1].items() if k != "dividers"}
    elif start is not None:
        start = dict(zero_model(), **start)
    oc = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
    ow = oc.set_cloud(case["scale"], *sl["res"])
    m = oracle_lib.Model() if start is None else oc.set_model(oracle_lib.Model(**start))
    rc, lp, tr = oc.run(ow, m, max_iter=mi if mi > 0 else -1, res_x=sl["res"][0], res_y=sl["res"][1], hard_cap=hard_cap, trace_cap=4096)
    assert lp.itercount == len(tr) <= 4096, (name, lp.itercount)
    rec = records(tr, lambda r: (r.loop.x_divider, r.loop.y_divider, r.loop.rot_divider, r.loop.div_divider))
    out = dict(sl=sl, scale=case["scale"], window=X.as_window(ow), start=start, rc=rc, loop=lp, trace=rec,
               pr_x=oc.pr_x.copy(), pr_y=oc.pr_y.copy(), nx=oc.nx.copy(), ny=oc.ny.copy())
    _oracle_runs[key] = out
    return out


def run_control(trace, max_iter=0, hard_cap=0, mutate=None, what=""):
    """Control fed a trace's recorded dx .. div; returns it and the dividers after every step."""
    c = Control(max_iter=max_iter, hard_cap=hard_cap, mutate=mutate, what=what)
    seen = []
    for r in trace:
        if c.done:
            break
        seen.append(tuple(float(d) for d in c.step(r["dx"], r["dy"], r["rot"], r["div"])))
    return c, seen
