"""bf_run_groups with "groups_wide" = 1 on the MI355X: a group whose window does not fit one work-group's LDS is solved inside
the call by the chip-wide loop (csrc/bf_groups_wide.hip: k_group_gather, k_group_scatter_back around bf_run on the inner
context; the routing rule is csrc/bf_group_rules.h, held on the host by tests/test_group_route_cpu.py).

The bar is equal bytes everywhere (include/bf_accel.h, "wide groups").  A wide group: its model, rc, iterations, the four
dividers and pr_x, pr_y, nx, ny, u, v on its events are those of a SECOND CONTEXT -- a separate Accel of the same capacity after
upload_events(E_g in upload order), set_cloud(scale, sensor), set_model(warm_g) when the call is warm, and bf_run with the group
options' max_iter, min_events, guards and hard_iter_cap on bf_run_opts_default.  Everything else -- the LDS groups, the skipped
ones, the events of none, a group beyond the context's image capacity, every call with the option off -- is the same call's bytes
without the option.  On a library without the option every test here fails at set_option("groups_wide", 1): BF_ERR_ARG."""
import ctypes as C

import numpy as np
import pytest

import groups_ref as gr
import segment_scene as scene
from better_flow_amd import synth

pytestmark = pytest.mark.gpu

H, W = scene.H, scene.W
GUARD = (90, 120)
HARD_CAP = 20000
MIN_EVENTS = 100
PER_EVENT = ("pr_x", "pr_y", "nx", "ny", "u", "v")


def fields(s):
    """A ctypes struct's fields as bytes (no padding; NaN-safe)."""
    return np.array([getattr(s, k) for k, _ in s._fields_ if not k.startswith("_")], dtype=np.float64).tobytes()


def raw(s):
    """A ctypes struct of integers (an info block, array fields included) as its own bytes."""
    return bytes(s)


def outcome(info):
    """What the definition fixes of a bf_run_info: rc, iterations, the four dividers (the other counters are diagnostics)."""
    return (info.rc, info.iterations, np.float32(info.x_divider).tobytes(), np.float32(info.y_divider).tobytes(),
            np.float32(info.rot_divider).tobytes(), np.float32(info.div_divider).tobytes())


def make_acc(accel_mod, n, scale=3, res=(H, W), max_rows=None):
    return accel_mod.Accel(device=0, max_events=max(n, 1), max_rows=max_rows or scale * res[0] + scale,
                           max_cols=scale * res[1] + scale)


def to_accel(accel_mod, warm):
    if warm is None:
        return None
    one = lambda m: accel_mod.Model(**{k: getattr(m, k) for k, _ in gr.oracle.Model._fields_})
    return [one(m) for m in warm] if isinstance(warm, list) else one(warm)


def seeded_models(K):
    """Model 0 the background's; the others seeded non-zero totals about a centre inside the sensor."""
    rng = np.random.default_rng(5)
    out = [gr.background_model()]
    for _ in range(1, K):
        m = gr.oracle.Model()
        m.cx, m.cy = rng.uniform(20, 70), rng.uniform(20, 100)
        m.total_dx, m.total_dy = rng.uniform(-0.3, 0.3, 2)
        m.total_rot, m.total_div = rng.uniform(-2e-3, 2e-3, 2)
        out.append(m)
    return out


def per_event(a):
    pr_x, pr_y, nx, ny = a.writeout_events()
    u, v = a.compute_uv()
    return dict(pr_x=pr_x, pr_y=pr_y, nx=nx, ny=ny, u=u, v=v)


def call(a, sl, gid, K, wide, warm=None, scale=3, res=(H, W), guard=GUARD, max_iter=-1, hard_cap=HARD_CAP, upload=True,
         min_events=MIN_EVENTS):
    """One bf_run_groups on a fresh upload of `sl` with the grouping `gid` and the option at `wide`: everything it leaves."""
    if upload:
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_groups(gid, K)
    if wide is not None:
        a.set_option("groups_wide", wide)
    m, i, q = a.run_groups(K, scale, res, guard, min_events, warm=warm, max_iter=max_iter, hard_iter_cap=hard_cap)
    out = per_event(a)
    out.update(models=m, infos=i, groups=q, wide=a.get_stat("groups_wide"))
    return out


def second_context(accel_mod, cap_n, sl, idx, warm=None, scale=3, res=(H, W), guard=GUARD, max_iter=-1, hard_cap=HARD_CAP,
                   min_events=MIN_EVENTS):
    """The definition's four steps on E_g = the events `idx` (upload order) of `sl`, on a separate Accel of the same capacity."""
    b = make_acc(accel_mod, cap_n, scale, res)
    try:
        b.upload_events(sl["fr_x"][idx], sl["fr_y"][idx], sl["t"][idx])
        b.set_cloud(scale, res[0], res[1])
        if warm is not None:
            b.set_model(warm)
        o = b.default_opts()
        o.max_iter, o.min_events, o.res_x, o.res_y, o.hard_iter_cap = max_iter, min_events, guard[0], guard[1], hard_cap
        m, info = accel_mod.Model(), accel_mod.RunInfo()
        rc = b.L.bf_run(b.h, C.byref(o), C.byref(m), C.byref(info))
        assert rc in (accel_mod.BF_OK, accel_mod.BF_ERR_NOCONV), (rc, b.L.bf_last_error(b.h))
        assert rc == info.rc
        out = per_event(b)
        out.update(model=m, info=info)
        return out
    finally:
        b.close()


def assert_group_is(got, g, idx, want, what):
    """Group g of the call `got` (its events: idx) carries the second context's bytes."""
    assert fields(got["models"][g]) == fields(want["model"]), (what, g, "model")
    assert outcome(got["infos"][g]) == outcome(want["info"]), (what, g, outcome(got["infos"][g]), outcome(want["info"]))
    for k in PER_EVENT:
        assert got[k][idx].tobytes() == want[k].tobytes(), (what, g, k, np.abs(got[k][idx] - want[k]).max())


def assert_same_call(got, ref, groups, rest, what):
    """The groups `groups` and the events `rest` (a mask) of `got` carry the bytes of the call `ref`."""
    for g in groups:
        assert fields(got["models"][g]) == fields(ref["models"][g]) and fields(got["infos"][g]) == fields(ref["infos"][g]), (what, g)
    for k in PER_EVENT:
        assert got[k][rest].tobytes() == ref[k][rest].tobytes(), (what, k)


def whole_call(r):
    """Every byte a call leaves, the groups' boxes included (of a wide group's bf_run_info what the definition fixes: its
    launches and polls are the inner run's diagnostics and vary with the host's timing)."""
    infos = [b"".join(bytes(str(x), "ascii") if isinstance(x, int) else x for x in outcome(i)) if q.reserved else fields(i)
             for i, q in zip(r["infos"], r["groups"])]
    return b"".join(fields(x) for x in r["models"] + r["groups"]) + b"".join(infos) + b"".join(r[k].tobytes() for k in PER_EVENT)


@pytest.fixture(scope="module")
def sc():
    return scene.make()


def scene_three_groups(sc):
    """Patch = group 0, background = group 1, 50 background events = group 2 (test_capacity_and_guards_in_one_call's)."""
    bg = np.flatnonzero(~sc["is_patch"])
    gid = np.where(sc["is_patch"], 0, 1).astype(np.int32)
    gid[bg[:50]] = 2
    return gid


# ---- 1. the scene: three groups, three legs; the option back to 0 ----

@pytest.mark.parametrize("leg", ["cold", "shared", "each"])
def test_scene_background_is_solved_wide(accel_mod, sc, leg):
    gid = scene_three_groups(sc)
    n = len(gid)
    warm = {"cold": None, "shared": gr.background_model(), "each": seeded_models(3)}[leg]
    aw = to_accel(accel_mod, warm)
    a = make_acc(accel_mod, n)
    never = make_acc(accel_mod, n)   # a context that never sets the option
    try:
        base = call(never, sc, gid, 3, None, warm=aw)
        off = call(a, sc, gid, 3, 0, warm=aw)
        on = call(a, sc, gid, 3, 1, warm=aw)
        back = call(a, sc, gid, 3, 0, warm=aw)
    finally:
        a.close()
        never.close()
    q = on["groups"][1]
    assert q.rows * q.cols * 16 > 156 * 1024 and (q.rows, q.cols) == (216, 309), (q.rows, q.cols)
    assert off["infos"][1].rc == accel_mod.BF_ERR_CAPACITY and off["wide"] == 0 and [x.reserved for x in off["groups"]] == [0, 0, 0]
    assert on["infos"][1].rc == 0 and on["infos"][1].iterations > 0
    assert [x.reserved for x in on["groups"]] == [0, 1, 0] and on["wide"] == 1
    idx = np.flatnonzero(gid == 1)
    w1 = None if warm is None else (aw[1] if isinstance(aw, list) else aw)
    want = second_context(accel_mod, n, sc, idx, warm=w1)
    print("%s: background %d events, wide rc %d, %d iterations" % (leg, len(idx), on["infos"][1].rc, on["infos"][1].iterations))
    assert_group_is(on, 1, idx, want, leg)
    assert np.abs(on["u"][idx]).max() > 0.0
    # the patch, the guarded group and the events of none: the same call without the option
    assert on["infos"][0].rc == 0 and on["infos"][2].rc == accel_mod.BF_SKIPPED
    assert_same_call(on, off, (0, 2), gid != 1, leg)
    for x, y in zip(on["groups"], off["groups"]):
        assert fields(x)[:-8] == fields(y)[:-8]   # (all but `reserved`)
    # the option back to 0: the bytes of a context that never set it
    assert whole_call(back) == whole_call(base) == whole_call(off), leg
    assert back["wide"] == 0 and back["infos"][1].rc == accel_mod.BF_ERR_CAPACITY


# ---- 2. two wide groups and eight LDS groups in one call; storage order and numbering ----

def halves_and_tiles(sl):
    """Left / right sensor halves of the upper two thirds: groups 0 and 1 (wide at scale 3); a 2 x 4 tile grid over the lower
    third: groups 2 .. 9; every 17th event in no group."""
    x, y = sl["fr_x"].astype(np.int64), sl["fr_y"].astype(np.int64)
    upper = x < 2 * H // 3
    tile = 2 + np.minimum((x - 2 * H // 3) * 2 // (H - 2 * H // 3), 1) * 4 + np.minimum(y * 4 // W, 3)
    gid = np.where(upper, (y >= W // 2).astype(np.int64), tile).astype(np.int32)
    gid[::17] = -1
    return gid


@pytest.fixture(scope="module")
def big():
    return synth.make_slice(60000, H, W, 0.030, seed=1)


def test_two_wide_groups_and_many_lds_groups(accel_mod, big):
    gid = halves_and_tiles(big)
    n, K = len(gid), 10
    a = make_acc(accel_mod, n)
    try:
        off = call(a, big, gid, K, 0)
        on = call(a, big, gid, K, 1)
        # the same call again, on the storage the first one left sorted
        again = call(a, big, gid, K, 1, upload=False)
        # another numbering of the groups
        perm = np.random.default_rng(3).permutation(K).astype(np.int32)
        renum = call(a, big, np.where(gid < 0, -1, perm[np.maximum(gid, 0)]).astype(np.int32), K, 1)
    finally:
        a.close()
    assert on["wide"] == 2 and [x.reserved for x in on["groups"]] == [1, 1] + [0] * 8
    assert [x.rc for x in off["infos"][:2]] == [accel_mod.BF_ERR_CAPACITY] * 2 and off["wide"] == 0
    assert all(x.rc == 0 for x in on["infos"]), [x.rc for x in on["infos"]]
    for g in (0, 1):
        idx = np.flatnonzero(gid == g)
        want = second_context(accel_mod, n, big, idx)
        print("wide group %d: %d events, %d x %d, %d iterations" % (g, len(idx), on["groups"][g].rows, on["groups"][g].cols, on["infos"][g].iterations))
        assert_group_is(on, g, idx, want, "halves")
    assert_same_call(on, off, range(2, K), (gid >= 2) | (gid < 0), "tiles and the events of none")
    assert not on["u"][gid < 0].any() and not on["nx"][gid < 0].any()
    assert whole_call(again) == whole_call(on) and again["wide"] == 2
    for g in range(K):
        assert fields(renum["models"][perm[g]]) == fields(on["models"][g]), g
        assert outcome(renum["infos"][perm[g]]) == outcome(on["infos"][g]), g
    for k in PER_EVENT:
        assert renum[k].tobytes() == on[k].tobytes(), k
    assert renum["wide"] == 2


# ---- 3. the LDS boundary at scale 1 ----

def test_lds_boundary_at_scale_one(accel_mod):
    RES = (130, 140)   # (synth's scene points start 10 pixels inside the sensor: the boxes below lie inside what they cover)
    sl = synth.make_slice(30000, RES[0], RES[1], 0.030, seed=4)
    n = len(sl["t"])
    x, y = sl["fr_x"], sl["fr_y"]
    a = make_acc(accel_mod, n, 1, RES)
    kw = dict(scale=1, res=RES)
    try:
        for rows, expect_wide in ((96, 0), (97, 1)):
            gid = np.where((x >= 14) & (x < 14 + rows) & (y >= 16) & (y < 16 + 104), 0, -1).astype(np.int32)
            off = call(a, sl, gid, 1, 0, **kw)
            on = call(a, sl, gid, 1, 1, **kw)
            q = on["groups"][0]
            assert (q.rows, q.cols) == (rows, 104), (q.rows, q.cols)
            assert on["wide"] == expect_wide and q.reserved == expect_wide
            idx = np.flatnonzero(gid == 0)
            want = second_context(accel_mod, n, sl, idx, **kw)
            if not expect_wide:   # exactly 156 KiB: the LDS path, the bytes of the option-off call
                assert on["infos"][0].rc == 0 and whole_call(on) == whole_call(off)
                # (recorded in DESIGN section 21, not asserted: the one-work-group result next to the chip-wide loop's)
                print("96 x 104 on the LDS path: %d iterations, second-context bf_run %d; worst flow difference %.3e px/s" % (
                    on["infos"][0].iterations, want["info"].iterations,
                    max(np.abs(on["u"][idx] - want["u"]).max(), np.abs(on["v"][idx] - want["v"]).max())))
            else:
                assert off["infos"][0].rc == accel_mod.BF_ERR_CAPACITY and on["infos"][0].rc == 0
                assert_group_is(on, 0, idx, want, "97 x 104")
                assert_same_call(on, off, (), gid < 0, "97 x 104")
    finally:
        a.close()


# ---- 4. loop outcomes: the iteration cap and max_iter ----

@pytest.mark.parametrize("kw,rc_name", [(dict(hard_cap=3), "BF_ERR_NOCONV"), (dict(max_iter=2), "BF_OK")])
def test_loop_outcomes_are_the_groups_own(accel_mod, sc, kw, rc_name):
    gid = scene_three_groups(sc)
    n = len(gid)
    a = make_acc(accel_mod, n)
    try:
        on = call(a, sc, gid, 3, 1, **kw)   # (the call itself returned BF_OK: Accel.run_groups raises otherwise)
    finally:
        a.close()
    idx = np.flatnonzero(gid == 1)
    want = second_context(accel_mod, n, sc, idx, **kw)
    print("%s: wide rc %d after %d iterations (second context: %d after %d)" % (kw, on["infos"][1].rc, on["infos"][1].iterations,
                                                                              want["info"].rc, want["info"].iterations))
    assert on["infos"][1].rc == getattr(accel_mod, rc_name) and on["wide"] == 1
    assert_group_is(on, 1, idx, want, str(kw))


# ---- 5. the context's image capacity; the option on without a wide group ----

def test_a_group_beyond_the_image_capacity_keeps_capacity(accel_mod, sc):
    gid = scene_three_groups(sc)
    a = make_acc(accel_mod, len(gid), max_rows=200)   # the background's window has 216 rows
    try:
        off = call(a, sc, gid, 3, 0)
        on = call(a, sc, gid, 3, 1)
    finally:
        a.close()
    assert on["groups"][1].rows == 216 and on["infos"][1].rc == accel_mod.BF_ERR_CAPACITY and on["infos"][0].rc == 0
    assert on["wide"] == 0 and whole_call(on) == whole_call(off)


def test_option_on_without_a_wide_group(accel_mod, big):
    GR, GC = 6, 8
    tid = (np.minimum(big["fr_x"].astype(np.int64) * GR // H, GR - 1) * GC +
           np.minimum(big["fr_y"].astype(np.int64) * GC // W, GC - 1)).astype(np.int32)
    kw = dict(guard=(H // GR, W // GC), min_events=256)
    a = make_acc(accel_mod, len(tid))
    try:
        off = call(a, big, tid, GR * GC, 0, **kw)
        on = call(a, big, tid, GR * GC, 1, **kw)
    finally:
        a.close()
    assert sum(1 for i in on["infos"] if i.rc == 0) >= GR * GC // 2
    assert on["wide"] == 0 and whole_call(on) == whole_call(off)


# ---- 6. arguments and trivial cases ----

def test_arguments_and_trivial_cases(accel_mod):
    sl = synth.make_slice(3000, H, W, 0.030, seed=2)
    n = len(sl["t"])
    a = make_acc(accel_mod, n)
    try:
        assert a.get_stat("groups_wide") == 0   # before any call
        for bad in (2, -1):
            with pytest.raises(accel_mod.BfError) as e:
                a.set_option("groups_wide", bad)
            assert e.value.code == accel_mod.BF_ERR_ARG
        a.set_option("groups_wide", 1)
        assert a.get_stat("groups_wide") == 0
        run = lambda K: a.run_groups(K, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)
        # a noise mask
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise=np.zeros(n, dtype=np.uint8))
        a.set_groups(np.zeros(n, dtype=np.int32), 1)
        with pytest.raises(accel_mod.BfError) as e:
            run(1)
        assert e.value.code == accel_mod.BF_ERR_ARG
        # K == 0
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_groups(np.full(n, -1, dtype=np.int32), 0)
        m, i, q = run(0)
        u, v = a.compute_uv()
        assert m == [] and i == [] and not u.any() and not v.any() and a.get_stat("groups_wide") == 0
        # the whole slice as one group goes wide; then a call without one: the statistic is the LAST call's
        a.set_groups(np.zeros(n, dtype=np.int32), 1)
        m, i, q = run(1)
        assert i[0].rc == 0 and q[0].reserved == 1 and a.get_stat("groups_wide") == 1
        a.set_groups(np.full(n, -1, dtype=np.int32), 1)
        m, i, q = run(1)
        assert i[0].rc == accel_mod.BF_SKIPPED and q[0].reserved == 0 and a.get_stat("groups_wide") == 0
        # zero events
        none = np.zeros(0, dtype=np.int32)
        a.upload_events(none, none, none)
        a.set_groups(none, 2)
        m, i, q = run(2)
        assert [x.rc for x in i] == [accel_mod.BF_SKIPPED] * 2 and [x.events for x in q] == [0, 0]
        assert [x.reserved for x in q] == [0, 0] and a.get_stat("groups_wide") == 0
    finally:
        a.close()


# ---- 7. the readers of addresses and times after a wide call ----

def test_readers_after_a_wide_call(accel_mod, sc):
    """bf_assign_groups, bf_project_groups, bf_merge_scores, bf_hold_groups with its readers and bf_track_keep / bf_track_overlap
    read addresses and times only: after a wide call they give the bytes they give after the option-off call; the held flow and
    the kept plane from before the call, the held grouping and the kept tracks are untouched by it."""
    gid = np.where(sc["is_patch"], 0, 1).astype(np.int32)
    n = len(gid)
    truth = to_accel(accel_mod, [gr.warm_from_flow(*scene.flow_of(vel)) for vel in (scene.V_PATCH, scene.V_BACKGROUND)])
    step = int(round(scene.DURATION_S * 1e9))

    def everything(wide):
        a = make_acc(accel_mod, n)
        try:
            a.upload_events(sc["fr_x"], sc["fr_y"], sc["t"])
            a.set_groups(gid, 2)
            a.global_set_window(3, 15)
            a.hold_groups(truth)
            plane, tinfo = a.track_keep(truth, 3, (H, W))
            held_before = b"".join(v.tobytes() for v in a.global_get_flow().values())
            r = call(a, sc, gid, 2, wide, warm=truth, upload=False)
            assert r["wide"] == wide and r["infos"][1].rc == (0 if wide else accel_mod.BF_ERR_CAPACITY)
            assert a.get_stat("groups_held") == 2 and a.tracks_held == 2
            out = [b"".join(v.tobytes() for v in a.global_get_flow().values())]
            assert out[0] == held_before
            out += [x.tobytes() for x in a.group_flow_medians()]
            ov, inside, oinfo = a.track_overlap(truth, step, 3, (H, W))
            out += [ov.tobytes(), inside.tobytes(), raw(oinfo)]
            img, scores, pinfo = a.project_groups(truth, 3, (H, W))
            out += [img[k].tobytes() for k in ("count", "label", "bgr")] + [raw(s) for s in scores] + [raw(pinfo)]
            gain, ins, ev, minfo = a.merge_scores(truth, 3, (H, W))
            out += [gain.tobytes(), ins.tobytes(), ev.tobytes(), raw(minfo)]
            a.hold_groups(truth)
            out += [v.tobytes() for v in a.global_get_flow().values()] + [x.tobytes() for x in a.group_flow_medians()]
            plane2, tinfo2 = a.track_keep(truth, 3, (H, W))
            out += [plane.tobytes(), plane2.tobytes(), raw(tinfo), raw(tinfo2)]
            g2, score, counts, ainfo = a.assign_groups(truth, 3, (H, W), install=True)
            out += [g2.tobytes(), score.tobytes(), counts.tobytes(), raw(ainfo)]
            assert a.get_stat("groups_held") == 2 and a.tracks_held == 2
            return out
        finally:
            a.close()

    off, on = everything(0), everything(1)
    assert len(off) == len(on)
    for k, (x, y) in enumerate(zip(off, on)):
        assert x == y, k


# ---- 8. the inner context is not a context of its own for the persistent form ----

def test_the_inner_context_is_not_counted(accel_mod, sc):
    gid = scene_three_groups(sc)
    small = synth.make_slice(20000, 180, 240, 0.05, seed=3)

    def persistent(go_wide):
        a = accel_mod.Accel(device=0, max_events=max(len(gid), len(small["t"])), max_rows=3 * 180 + 3, max_cols=3 * 240 + 3)
        try:
            r = call(a, sc, gid, 3, 1 if go_wide else 0)
            assert r["wide"] == (1 if go_wide else 0)
            a.upload_events(small["fr_x"], small["fr_y"], small["t"])
            a.set_cloud(3, 180, 240)
            a.set_model(accel_mod.Model())
            return a.get_stat("persistent"), a.get_stat("one_kernel")
        finally:
            a.close()

    # (one outer context alive at a time: each closes before the next is created)
    plain, wide = persistent(False), persistent(True)
    print("persistent / one_kernel for the warm slice: never wide %s, after a wide group %s" % (plain, wide))
    assert wide == plain
