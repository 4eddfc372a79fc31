"""The small cases of the loop-form table (scripts/loop_form_table.py, tests/test_gpu_loop_forms.py, tests/test_loop_forms_cpu.py).

One case = one context: options, one slice, bf_set_cloud, optionally a first run and bf_set_model (a warm start), the run whose
loop is recorded.  Everything but the forcing options is left to "auto", and the cases sit on both sides of each of its
thresholds a small input reaches.  The slices pin an event to two opposite corners of the sensor, so the window is the whole
sensor: scale * H x scale * W pixels.  60 x 90 at scale 3 has P = 48 600 pixels; the thresholds in events are
    n >= P (48 600)     delta scatter, for a "co_schedule" context
    2 n <= P (24 300)   the one-kernel iteration, for a context alone
    8 n <= P (6 075)    the one-kernel iteration, for a "co_schedule" context
    4 n <  P (12 149)   event lists instead of dense slabs in the two-kernel loop
`home` is where the model update runs; the table's last column (finish_updates_per_stencil_launch) tells k_finish_update from the
stencil tail, "k1_head" the scatter head from both."""
import numpy as np

from better_flow_amd import synth

ITER = 5          # cap of a run that is not about the cap
COLUMNS = ("loop_form", "scatter_format", "k1_head", "k1_threads", "k1_events_per_thread", "k3_mode", "k3_capped")
OPTION_KEYS = ("binned", "fused", "persist", "delta_scatter", "sep_update", "bin_compact", "bin_split", "co_schedule", "force_split")
OPTION_DEFAULTS = dict(binned=1, fused=1, persist=1, delta_scatter=1, sep_update=1, bin_compact=1, bin_split=1, co_schedule=0, force_split=0)
CO = dict(co_schedule=1)


def case(cid, n, home, opts=None, H=60, W=90, scale=3, noise=False, warm=False, live=1, max_iter=ITER):
    return dict(id=cid, n=n, home=home, opts=dict(opts or {}), H=H, W=W, scale=scale, noise=noise, warm=warm, live=live, max_iter=max_iter)


CASES = [
    # a context alone: one-kernel iteration up to one event per two pixels, then the two-kernel loop with the update at the scatter head
    case("alone_2n_at_pixels", 24300, "head"),
    case("alone_2n_above_pixels", 24301, "head"),
    case("alone_sparse", 6000, "head"),
    case("alone_dense", 48600, "head"),
    case("alone_warm", 20000, "head", warm=True),                  # the persistent kernel
    case("alone_warm_dense", 30000, "head", warm=True),
    case("alone_warm_second_context", 20000, "head", warm=True, live=2),
    case("alone_noise_mask", 20000, "tail", noise=True),
    case("alone_force_split", 20000, "tail", dict(force_split=1)),
    case("alone_scale1", 2700, "head", scale=1),
    case("alone_scale1_dense", 2701, "head", scale=1),
    # "co_schedule": one-kernel iteration up to one event per eight pixels, event lists with k_finish_update up to one per four,
    # dense slabs with the update in the stencil tail from there, delta scatter from one event per pixel
    case("co_8n_at_pixels", 6075, "head", CO),
    case("co_8n_above_pixels", 6076, "separate", CO),
    case("co_lists", 12149, "separate", CO),
    case("co_slabs", 12150, "tail", CO),
    case("co_below_pixels", 48599, "tail", CO, max_iter=-1),
    case("co_at_pixels", 48600, "tail", CO, max_iter=-1),
    case("co_at_pixels_max_iter_0", 48600, "tail", CO, max_iter=0),
    case("co_at_pixels_max_iter_199", 48600, "tail", CO, max_iter=199),
    case("co_at_pixels_max_iter_200", 48600, "tail", CO, max_iter=200),
    case("co_at_pixels_warm", 48600, "tail", CO, warm=True),
    case("co_at_pixels_noise_mask", 48600, "tail", CO, noise=True, max_iter=-1),
    case("co_at_pixels_force_split", 48600, "tail", dict(CO, force_split=1), max_iter=-1),
    case("co_warm_sparse", 6000, "head", CO, warm=True),
    case("co_scale1_below_pixels", 5399, "tail", CO, scale=1, max_iter=-1),
    case("co_scale1_at_pixels", 5400, "tail", CO, scale=1, max_iter=-1),
    # every forcing option at 0 and at 2, once each
    case("binned_0", 30000, "tail", dict(binned=0)),
    case("binned_2_co_at_pixels", 48600, "tail", dict(CO, binned=2), max_iter=-1),
    case("fused_0", 20000, "head", dict(fused=0)),
    case("fused_2_dense", 40000, "head", dict(fused=2)),
    case("fused_2_co_at_pixels", 48600, "head", dict(CO, fused=2), max_iter=-1),
    case("persist_0_warm", 20000, "head", dict(persist=0), warm=True),
    case("persist_2_cold", 20000, "head", dict(persist=2)),
    case("delta_0_co_at_pixels", 48600, "tail", dict(CO, delta_scatter=0), max_iter=-1),
    case("delta_2_alone", 20000, "tail", dict(delta_scatter=2)),
    case("delta_2_noise_mask", 20000, "tail", dict(delta_scatter=2), noise=True),
    case("sep_update_0_co_lists", 12149, "tail", dict(CO, sep_update=0)),
    case("sep_update_2_co_slabs", 30000, "separate", dict(CO, sep_update=2)),
    case("sep_update_2_alone", 30000, "head", dict(sep_update=2)),
    case("bin_compact_0_co", 12149, "tail", dict(CO, bin_compact=0)),
    case("bin_compact_2_co", 30000, "separate", dict(CO, bin_compact=2)),
    case("bin_compact_2_alone", 30000, "head", dict(bin_compact=2)),
    case("bin_split_0_alone", 30000, "head", dict(bin_split=0)),
    case("bin_split_2_alone", 30000, "head", dict(bin_split=2)),
    case("bin_split_2_co", 30000, "tail", dict(CO, bin_split=2)),
]


def case_slice(c):
    """Exactly c["n"] events in ascending time, one at (0, 0) and one at (H - 1, W - 1)."""
    H, W, n = c["H"], c["W"], c["n"]
    sl = synth.make_slice(int(1.5 * n) + 1000, H, W, 0.03, seed=5)
    m = len(sl["t"])
    assert m >= n
    idx = np.linspace(0, m - 1, n).astype(np.int64)
    out = {k: np.ascontiguousarray(sl[k][idx]) for k in ("fr_x", "fr_y", "t")}
    out["fr_x"][0], out["fr_y"][0] = 0, 0
    out["fr_x"][-1], out["fr_y"][-1] = H - 1, W - 1
    return out


def finish_updates_per_stencil_launch(info, prof):
    """Tells the update as a kernel of its own from the update in the stencil tail, which "k1_head" does not: the launches of
    the run that are neither a scatter nor a stencil launch nor one of the bracketed others (a re-bin, the final warp), per
    stencil launch, rounded.  What is left are the k_finish_update launches -- one per iteration or none -- and two of every
    re-bin's three (one bracket around the trio); a run launches its iterations eight at a time and re-bins a few times in
    hundreds, so the quotient is near 1 or near 0 however many batches the host got in before it saw the end.  -1: the run
    launched no stencil kernel (the one-kernel loops)."""
    if prof.stencil_launches == 0:
        return -1
    rest = info.launches - prof.warp_scatter_launches - prof.stencil_launches - prof.other_launches
    return int(round(rest / prof.stencil_launches))


def case_row(accel_mod, c, lib=None):
    """Runs one case on a fresh context (the only live one, but for the idle extra of live = 2) and returns its table columns."""
    sl = case_slice(c)
    H, W, s = c["H"], c["W"], c["scale"]
    kw = dict(max_events=c["n"], max_rows=s * H + s, max_cols=s * W + s)
    if lib:
        kw["lib"] = lib
    a = accel_mod.Accel(**kw)
    extra = [accel_mod.Accel(**kw) for _ in range(c["live"] - 1)]
    try:
        for k, v in c["opts"].items():
            a.set_option(k, v)
        noise = (np.arange(c["n"]) % 7 == 3).astype(np.uint8) if c["noise"] else None
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise)
        w = a.set_cloud(s, H, W)
        assert (w.scale_img_x, w.scale_img_y) == (s * H, s * W), (w.scale_img_x, w.scale_img_y)
        o = a.default_opts()
        o.res_x, o.res_y = H, W
        if c["warm"]:
            o.max_iter = ITER
            _, m, _ = a.run(o)
            a.set_cloud(s, H, W)
            a.set_model(m)
        o.max_iter = c["max_iter"]
        a.profile_enable(1)
        a.profile_reset()
        _, _, info = a.run(o)
        return tuple(a.get_stat(k) for k in COLUMNS) + (finish_updates_per_stencil_launch(info, a.profile_get()),)
    finally:
        for x in extra:
            x.close()
        a.close()


def format_row(c, row):
    return "%s %s" % (c["id"], " ".join(str(v) for v in row))


def facts_line(c):
    """The case as the plain numbers tests/cpp/test_plan.cpp reads ("forms" mode)."""
    opts = dict(OPTION_DEFAULTS, **c["opts"])
    return "%s %d %d %d %d %d %d %d %d %s\n" % (c["id"], c["H"], c["W"], c["scale"], c["n"], int(c["noise"]), int(c["warm"]), c["live"],
                                                 c["max_iter"], " ".join(str(int(opts[k])) for k in OPTION_KEYS))
