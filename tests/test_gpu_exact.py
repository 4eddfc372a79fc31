"""The time image and the moments of every device path against an exact, order-free reference (tests/exact_ref.py).

The device keeps a count and an integer nanosecond sum per pixel and turns them into f32 with one documented sequence
(time_from_sums), so its time image has ONE right answer per pixel; the oracle adds f32 in container order and can hold it
to 1e-6 only (tests/test_gpu_parity.py).  Here the bar is the bits: count and time image on every pixel, for the stand-alone
operators at every scale bf_set_cloud accepts and both accumulator packings, after warps that move and drop events, with a
noise mask, in iteration 0 of every loop form and after converged runs.  The moments are held to a bound that is derived from
the arithmetic (exact_ref.moment_bound), not measured.  tests/test_exact_ref_cpu.py proves the reference itself on the CPU.

The slices are tests/exact_slices.py's: times of a few microseconds (every box sum below 2^22 ns: one nanosecond shows in the
bits of every pixel), piles of exactly 254 .. 257 events around the end of the reciprocal table, signed times with a sum of
exactly 0 ns and means on both sides of the 1e-6f validity threshold, and times up to 2^31 - 1.  The images span several
16 x 64 stencil tiles, ragged in both directions (75 x 123 scaled pixels at scale 3).

A mismatch prints the pixel, its cnt and S, the bit patterns got and wanted and the options of the case.  Nothing here
provokes anything: all inputs are valid slices.

Scales: 1, 3, 5, 7 and 9 are every half-scale the stencil kernels are compiled for.  bf_set_cloud refuses an even scale, as the
reference asserts (optimizer_rolling.h:274), so for 2, 4 and 8 the case that can be held is the refusal itself (BF_ERR_ARG,
nothing launched).
"""
import numpy as np
import pytest

import exact_ref as X

from exact_slices import (EVEN_SCALES, KINDS, ODD_SCALES, PAIR_A, PILE_KS, SENSORS, SPECIAL, make_slice, reference_images, warps,
                          window_of)


def new_accel(accel_mod, n_max, opts=None, scale=9, H=70, W=90):
    from helpers import make_accel
    return make_accel(accel_mod, opts, max_events=max(n_max, 8192), max_rows=scale * (H + 1) + scale, max_cols=scale * (W + 1) + scale)


def stage(acc, sl, scale, noise=None):
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise)
    gw = acc.set_cloud(scale, sl["H"] + 1, sl["W"] + 1)
    w = window_of(sl, scale)
    assert (gw.scale_img_x, gw.scale_img_y, gw.metric_wsizex, gw.metric_wsizey, gw.x_shift, gw.y_shift) == \
        (w["R"], w["C"], w["wsx"], w["wsy"], w["x_shift"], w["y_shift"])
    return w


def check_images(acc, sl, w, scale, what, noise=None):
    """The device's count and time image against the reference built from the device's own pr (writeout_events: pinned to
    the oracle bit for bit by test_gpu_parity.py).  Returns (cnt, S, time image) of the reference."""
    pr_x, pr_y, _, _ = acc.writeout_events()
    cnt, S, want = reference_images(sl, w, scale, pr_x, pr_y, noise)
    got_t, got_c = acc.get_time_img()
    msg = X.first_mismatch(got_t, got_c, want, cnt, S, what)
    assert msg is None, msg
    return cnt, S, want


def check_model(got, ref, what, cx=None, cy=None):
    """cnt equal; dx, dy, rot, div within exact_ref.moment_bound; cx, cy equal (or, given, within 2 ulp of them)."""
    bound = X.moment_bound(ref)
    print("%s: n = %d, bounds %s" % (what, ref["cnt"], {k: "%.2e" % v for k, v in bound.items()}))
    assert got.cnt == ref["cnt"], (what, got.cnt, ref["cnt"])
    for k in ("dx", "dy", "rot", "div"):
        g, r = getattr(got, k), ref[k]
        print("    %s: got %.17g want %.17g, off by %.3e (bound %.3e)" % (k, g, r, abs(g - r), bound[k]))
        assert abs(g - r) <= bound[k], (what, k, g, r, abs(g - r), bound[k])
    if cx is None:
        assert got.cx == ref["cx"] and got.cy == ref["cy"], (what, got.cx, ref["cx"], got.cy, ref["cy"])
    else:
        assert X.ulp_distance64(got.cx, cx) <= 2 and X.ulp_distance64(got.cy, cy) <= 2, (what, got.cx, cx, got.cy, cy)


# ---- 1. time image bits, stand-alone operators ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_time_image_bits_standalone(accel_mod, kind):
    """set_cloud, then project_4param_reinit with the identity, the moderate and the strong warp, at every odd scale and with the
    packed and the split accumulators; once more with a noise mask.  Count and time bits on every pixel.

    The grid is not thinned further: all 30 cases of a slice run in 0.1 - 0.25 s on an MI355X (`pytest --durations=0`; the
    whole file in 1.3 s), and every scale compiles its own stencil kernel while the warps decide which events the edges drop.
    Which accumulator layout ran is not observable through the C-ABI (no statistic reports it): force_split = 1 is the documented
    switch to the split planes and bf_set_option accepts it; that the wide slice still packs without it is the host rule
    bit_length(sum(t - tmin)) + bit_length(n) <= 64, which exact_slices.make_slice asserts on the slice."""
    acc = new_accel(accel_mod, 8192)
    try:
        for scale in ODD_SCALES:
            sl = make_slice(kind, *SENSORS[1 if scale == 1 else 3])
            for split in (0, 1):
                acc.set_option("force_split", split)
                w = stage(acc, sl, scale)
                if scale == 3:
                    assert (w["R"], w["C"]) == (75, 123)
                for name, prm in warps(sl):
                    acc.project_4param_reinit(*prm)
                    what = "%s slice, scale %d, force_split %d, %s warp" % (kind, scale, split, name)
                    cnt, S, _ = check_images(acc, sl, w, scale, what)
                    _case_properties(kind, name, scale, sl, cnt, S)
        # a noise mask (every third event): the atomics scatter skips them, the window is still the whole cloud's
        sl = make_slice(kind, *SENSORS[3])
        noise = (np.arange(len(sl["t"])) % 3 == 0).astype(np.uint8)
        for split in (0, 1):
            acc.set_option("force_split", split)
            w = stage(acc, sl, 3, noise)
            acc.project_4param_reinit(*warps(sl)[1][1])
            cnt, _, _ = check_images(acc, sl, w, 3, "%s slice, scale 3, force_split %d, moderate warp, noise mask" % (kind, split), noise)
            assert 0 < cnt.sum() < 9 * len(sl["t"]) * 0.7
    finally:
        acc.close()


def _case_properties(kind, warp, scale, sl, cnt, S):
    """What a case exists for, asserted on the reference's planes."""
    # (before a warp the window holds every event but those of the last row and column: accel_lib.h:157)
    inside = scale * scale * int(X.targets(sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64), window_of(sl, scale), scale)[2].sum())
    if warp == "identity":
        assert cnt.sum() == inside > 0.9 * scale * scale * len(sl["t"])
    if warp == "strong":
        assert 0 < cnt.sum() < inside, "the strong warp must move events out of the window"
    if kind == "small":
        assert int(S.max()) < (1 << 22) and int(S.min()) >= 0   # where 1 ns is visible in the bits of every pixel
    if kind == "piles" and warp == "identity":
        have = set(np.unique(cnt).tolist())
        assert set(PILE_KS) <= have, sorted(set(PILE_KS) - have)   # box counts of exactly k, both sides of the table's end
    if kind == "piles" and warp == "moderate" and scale == 3:
        w = window_of(sl, scale)
        r0, c0 = PAIR_A[0] * scale + int(w["x_shift"]), PAIR_A[1] * scale + int(w["y_shift"])
        box = cnt[r0 - 2:r0 + 3, c0 - 2:c0 + 6]
        assert (box == 255).any() and (box == 256).any(), box   # the pair: 255 next to 255 + 1
    if kind == "signed" and warp == "identity":
        w = window_of(sl, scale)
        at = lambda name: (SPECIAL[name][0] * scale + int(w["x_shift"]), SPECIAL[name][1] * scale + int(w["y_shift"]))
        tim = X.time_from_planes(cnt, S)
        assert cnt[at("zero")] == 4 and S[at("zero")] == 0 and tim[at("zero")] == 0
        for name, mean in (("m999", 999), ("m1000", 1000), ("m1001", 1001)):
            assert cnt[at(name)] == 2 and S[at(name)] == 2 * mean
        v = X.valid(tim)
        assert not v[at("zero")] and not v[at("m999")] and not v[at("m1000")] and v[at("m1001")]


@pytest.mark.gpu
def test_even_scales_are_refused(accel_mod):
    """Scales 2, 4 and 8: the reference asserts an odd scale (optimizer_rolling.h:274) and bf_set_cloud refuses an even one with
    BF_ERR_ARG before it launches anything; the context then goes on to give the right bits at scale 3."""
    sl = make_slice("small", *SENSORS[3])
    acc = new_accel(accel_mod, 8192)
    try:
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        for scale in EVEN_SCALES:
            with pytest.raises(accel_mod.BfError) as e:
                acc.set_cloud(scale, sl["H"] + 1, sl["W"] + 1)
            assert e.value.code == accel_mod.BF_ERR_ARG
        w = stage(acc, sl, 3)
        check_images(acc, sl, w, 3, "small slice, scale 3, after the refused scales")
    finally:
        acc.close()


# ---- 2. moments, stand-alone --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_moments_standalone(accel_mod, kind):
    """fast_model() on the device's own planes after the identity and the moderate warp, and fast_model(img) on the reference
    image: cnt, cx, cy equal, dx, dy, rot, div within the derived bound."""
    acc = new_accel(accel_mod, 8192)
    try:
        for scale in (1, 3, 5):
            sl = make_slice(kind, *SENSORS[1 if scale == 1 else 3])
            w = stage(acc, sl, scale)
            for name, prm in warps(sl)[:2]:
                acc.project_4param_reinit(*prm)
                what = "%s slice, scale %d, %s warp" % (kind, scale, name)
                _, _, img = check_images(acc, sl, w, scale, what)
                ref = X.moments(img)
                assert ref["cnt"] > 100, (what, ref["cnt"])
                check_model(acc.fast_model(), ref, what + ", device planes")
                check_model(acc.fast_model(img), ref, what + ", reference image")
    finally:
        acc.close()


# ---- 3. iteration 0 of a cold run, every loop form -------------------------------------------------------------------------

# (name, options, what bf_get_stat must say after set_cloud)
# What proves that a form ran: scatter_format / one_kernel / persistent are the plan bf_run follows, k1_threads and k3_mode are set
# only by a launch of the two-kernel loop, and overflow_events > 0 shows the unpacked tiles of that loop (every event takes the
# overflow path).  The one-kernel loop has no overflow path, so for ITS unpacked tiles neither bf_get_stat nor bf_run_info carries
# a signal: that row is held by the option being accepted (bf_set_option fails on an unknown key or value) and by the packing rule
# (20 bits cannot hold the count and time fields of a bin of these slices), which test_gpu_fused.py relies on in the same way.
FORMS = (
    ("global atomics", dict(binned=0, fused=0), dict(scatter_format=-1, one_kernel=0)),
    ("dense slabs", dict(binned=2, fused=0, bin_compact=0, bin_split=0), dict(scatter_format=0, one_kernel=0)),
    ("event lists", dict(binned=2, fused=0, bin_compact=2), dict(scatter_format=2, one_kernel=0)),
    ("own pixels + margin plane", dict(binned=2, fused=0, bin_compact=0, bin_split=2), dict(scatter_format=3, one_kernel=0)),
    ("dense slabs, tail update", dict(binned=2, fused=0, bin_compact=0, bin_split=0, co_schedule=1), dict(scatter_format=0, one_kernel=0)),
    ("one-kernel pass", dict(fused=2, persist=0), dict(one_kernel=1, persistent=0)),
    ("persistent loop", dict(fused=2, persist=2), dict(one_kernel=1, persistent=1)),
    ("one-kernel pass, unpacked tiles", dict(fused=2, persist=0, bin_pack_limit=20), dict(one_kernel=1, persistent=0)),
    ("dense slabs, unpacked tiles", dict(binned=2, fused=0, bin_compact=0, bin_split=0, bin_pack_limit=20), dict(scatter_format=0, one_kernel=0)),
)


def cold_run(accel_mod, sl, scale, opts, want_stat, name):
    """A cold run (max_iter = 0: no cap, the loop ends by its own rules; trace_cap = 1: the record of iteration 0) of the form
    `opts` asks for; asserts that the form is the one that ran, and the time image after the run.  Returns the model of
    iteration 0, the run's info and the reference's count image after the run."""
    acc = new_accel(accel_mod, len(sl["t"]), opts, scale=scale, H=sl["H"], W=sl["W"])
    try:
        w = stage(acc, sl, scale)
        stat = {k: acc.get_stat(k) for k in want_stat}
        assert stat == want_stat, (name, stat, want_stat)
        o = acc.default_opts()
        o.res_x, o.res_y, o.trace_cap, o.want_uv, o.max_iter = sl["H"] + 1, sl["W"] + 1, 1, 1, 0
        rc, m, info = acc.run(o)
        tr = acc.get_trace(1)
        print("%s: rc %d, %d iterations, %d launches, %d re-bins, %d overflow events" %
              (name, rc, info.iterations, info.launches, info.rebins, info.overflow_events))
        assert rc == 0 and len(tr) == 1 and info.iterations >= 1, (name, rc, len(tr), info.iterations)
        if "unpacked" in name and not opts.get("fused"):
            assert info.overflow_events > 0, name   # a bin that cannot pack sends every event down the exact overflow path
        if opts.get("binned") == 2:
            assert acc.get_stat("k1_threads") > 0 and acc.get_stat("k3_mode") >= 0, name   # the two-kernel loop's kernels ran
        else:
            assert acc.get_stat("k1_threads") == -1, name
        after = check_images(acc, sl, w, scale, "%s slice, scale %d, after a run of the %s loop" % (sl["kind"], scale, name))
        return tr[0].model, info, after[0]
    finally:
        acc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("piles", "signed"))
def test_iteration_zero_every_loop_form(accel_mod, kind):
    """The first iteration of a cold run scatters with the identity warp, so no sin / cos enters: trace[0].model has the
    reference's valid-pixel count, dx, dy, rot, div within the derived bound, and cx, cy within 2 ulp of
    (cx_ref - x_shift) / scale (the device multiplies by the reciprocal of the scale there)."""
    scale = 3
    sl = make_slice(kind, *SENSORS[3])
    w = window_of(sl, scale)
    cnt, S, img = reference_images(sl, w, scale, sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64))
    ref = X.moments(img)
    assert ref["cnt"] > 1000
    cx = (ref["cx"] - w["x_shift"]) / scale
    cy = (ref["cy"] - w["y_shift"]) / scale
    for name, opts, want_stat in FORMS:
        m0, _, _ = cold_run(accel_mod, sl, scale, opts, want_stat, name)
        check_model(m0, ref, "%s slice, iteration 0 of the %s loop" % (kind, name), cx=cx, cy=cy)


# ---- 4. after a run -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("form", (0, 1, 5), ids=lambda i: FORMS[i][0].replace(" ", "_"))
def test_time_image_bits_after_a_converged_run(accel_mod, form):
    """One run to convergence per loop family (atomics, two-kernel, one-kernel): the events are where the last warp left them
    (and, in the binned loops, sorted by tile); get_time_img() must equal the reference built from the pr read back."""
    from better_flow_amd import synth
    name, opts, want_stat = FORMS[form]
    H, W = 60, 80
    mv = synth.make_slice(20000, H, W, 0.03, seed=5)
    sl = dict(kind="moving", H=H - 1, W=W - 1, fr_x=mv["fr_x"], fr_y=mv["fr_y"], t=mv["t"])
    _, info, cnt = cold_run(accel_mod, sl, 3, opts, want_stat, name)
    assert info.iterations > 5, info.iterations   # it did warp: the image is not the identity's
    idc, _, _ = reference_images(sl, window_of(sl, 3), 3, sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64))
    assert not np.array_equal(cnt, idc)
