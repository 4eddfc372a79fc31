"""Delta scatter ("delta_scatter" = 2) against the plain global-atomic loop ("binned" = 0, "delta_scatter" = 0), byte for byte.

The plane words are exact integers, so a plane that is kept from launch to launch -- every event whose scatter pixel changed
taken off the old pixel and added to the new one -- must hold the bits of a rebuilt one, and everything behind it with it: the
per-iteration trace, the final model and loop state, the images read back after the run, the per-event flow.  The inputs are
those of tests/delta_cases.py; tests/test_delta_transitions_cpu.py shows on the oracle that events there change pixel, leave
the window and come back in numbers.  Every scenario is a short script of calls run on one context; the reference runs it
once per (input, planes) and the forms are compared record by record."""
import numpy as np
import pytest

import delta_cases as dc

pytestmark = pytest.mark.gpu

PLAIN = dict(binned=0, fused=0, delta_scatter=0)
DELTA = dict(delta_scatter=2)                       # (whatever the slice would take otherwise: the form replaces it)
DELTA_NO_BINS = dict(binned=0, fused=0, delta_scatter=2)


def info_key(info):
    return (info.rc, info.iterations, info.x_divider, info.y_divider, info.rot_divider, info.div_divider)


def run_record(a, rec, H, W, **kw):
    """One bf_run on context `a` and everything it leaves behind, appended to `rec` as bytes; returns the model."""
    o = a.default_opts()
    o.res_x, o.res_y, o.trace_cap, o.want_uv = H, W, dc.K, 1
    for k, v in kw.items():
        setattr(o, k, v)
    rc, m, info = a.run(o)
    rec.append(("loop", a.get_stat("loop_form")))
    rec.append(("info", info_key(info)))
    rec.append(("model", bytes(m)))
    tr = a.get_trace(dc.K)
    rec.append(("trace", [(bytes(t.model), t.x_divider, t.y_divider, t.rot_divider, t.div_divider, t.iteration) for t in tr]))
    u, v = a.compute_uv()
    rec.append(("uv", u.tobytes(), v.tobytes()))
    return m


def image_record(a, rec):
    t, c = a.get_time_img()
    rec.append(("images", t.tobytes(), c.tobytes()))


def play(accel_mod, scenario, options, sl, H, W, scale, split, noise=None):
    a = accel_mod.Accel(max_events=len(sl["t"]), max_rows=scale * H + scale, max_cols=scale * W + scale)
    try:
        for k, v in options.items():
            a.set_option(k, v)
        if split:
            a.set_option("force_split", 1)
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise)
        a.set_cloud(scale, H, W)
        rec = []
        scenario(accel_mod, a, rec, H, W, scale)
        return rec
    finally:
        a.close()


def cold(accel_mod, a, rec, H, W, scale):
    run_record(a, rec, H, W)
    image_record(a, rec)


def capped(accel_mod, a, rec, H, W, scale):
    run_record(a, rec, H, W, max_iter=10)
    image_record(a, rec)


def queued_past_done(accel_mod, a, rec, H, W, scale):
    """Batches of 64 launches: the loop ends after about twenty iterations, the rest of the batch finds `done`."""
    run_record(a, rec, H, W, poll_interval=64)
    image_record(a, rec)


def warm(accel_mod, a, rec, H, W, scale):
    """bf_set_model before the second slice's run: the first launch of that run applies the pending warp."""
    m = run_record(a, rec, H, W)
    a.set_cloud(scale, H, W)
    a.set_model(dc.overshoot(accel_mod.Model, m))
    run_record(a, rec, H, W)
    image_record(a, rec)


def reuse(accel_mod, a, rec, H, W, scale):
    """Which plane buffer is clean and which is dirty, across runs and stand-alone operators on one context."""
    run_record(a, rec, H, W, max_iter=7)      # leaves the loop's buffer dirty
    run_record(a, rec, H, W, max_iter=4)      # a second run straight behind it, from the warped events
    image_record(a, rec)                      # a stand-alone scatter + stencil pass
    image_record(a, rec)                      # ... and another one, into the other buffer
    a.set_cloud(scale, H, W)                  # Event::reset
    run_record(a, rec, H, W)
    image_record(a, rec)
    a.project_4param_reinit(0.3, -0.2, H / 2.0, W / 2.0, 0.01, 0.02)
    image_record(a, rec)
    run_record(a, rec, H, W, max_iter=3)
    image_record(a, rec)


def compare(got, ref, want_loop, ref_loop, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0]
        if g[0] == "loop":
            assert g[1] == want_loop and r[1] == ref_loop, (what, k, g[1], r[1])
        else:
            assert g == r, "%s: record %d (%s) differs from the plain loop's" % (what, k, g[0])


_REF = {}


def reference(accel_mod, scenario, scale, split):
    key = (scenario.__name__, scale, split)
    if key not in _REF:
        _REF[key] = play(accel_mod, scenario, PLAIN, dc.small_slice(), dc.H, dc.W, scale, split)
    return _REF[key]


@pytest.mark.parametrize("split", (False, True), ids=("packed", "split"))
@pytest.mark.parametrize("scale", dc.SCALES)
@pytest.mark.parametrize("scenario", (cold, capped, queued_past_done, warm, reuse), ids=lambda f: f.__name__)
def test_delta_scatter_same_bits(accel_mod, scenario, scale, split):
    ref = reference(accel_mod, scenario, scale, split)
    assert any(r[0] == "info" and r[1][1] >= 3 for r in ref)
    got = play(accel_mod, scenario, DELTA, dc.small_slice(), dc.H, dc.W, scale, split)
    compare(got, ref, accel_mod.BF_LOOP_DELTA, accel_mod.BF_LOOP_ATOMIC, (scenario.__name__, scale, split))


@pytest.mark.parametrize("scale", dc.SCALES)
def test_delta_scatter_same_bits_without_bin_buffers(accel_mod, scale):
    """... on a context whose slice was never planned for the tile-binned loop (no count planes, no bitmaps)."""
    ref = reference(accel_mod, reuse, scale, False)
    got = play(accel_mod, reuse, DELTA_NO_BINS, dc.small_slice(), dc.H, dc.W, scale, False)
    compare(got, ref, accel_mod.BF_LOOP_DELTA, accel_mod.BF_LOOP_ATOMIC, ("reuse, no bins", scale))


@pytest.mark.parametrize("scale", dc.SCALES)
def test_noise_mask_keeps_the_plain_loop(accel_mod, scale):
    sl = dc.small_slice()
    noise = (np.arange(len(sl["t"])) % 7 == 3).astype(np.uint8)
    ref = play(accel_mod, cold, PLAIN, sl, dc.H, dc.W, scale, False, noise)
    got = play(accel_mod, cold, DELTA, sl, dc.H, dc.W, scale, False, noise)
    compare(got, ref, accel_mod.BF_LOOP_ATOMIC, accel_mod.BF_LOOP_ATOMIC, ("noise mask", scale))


def test_delta_scatter_against_the_binned_default(accel_mod):
    """60 x 90, 50 000 events, scale 3: forced delta scatter against what a context takes by default."""
    sl = dc.medium_slice()
    ref = play(accel_mod, cold, {}, sl, 60, 90, 3, False)
    ref_loop = next(r[1] for r in ref if r[0] == "loop")
    assert ref_loop in (accel_mod.BF_LOOP_BINNED, accel_mod.BF_LOOP_ONE_KERNEL, accel_mod.BF_LOOP_PERSISTENT), ref_loop
    got = play(accel_mod, cold, DELTA, sl, 60, 90, 3, False)
    compare(got, ref, accel_mod.BF_LOOP_DELTA, ref_loop, "60 x 90 against the default")
    two = play(accel_mod, cold, dict(binned=2, fused=0, co_schedule=1), sl, 60, 90, 3, False)   # the headline's two-kernel loop
    compare(got, two, accel_mod.BF_LOOP_DELTA, accel_mod.BF_LOOP_BINNED, "60 x 90 against the co-scheduled tile-binned loop")
