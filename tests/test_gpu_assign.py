"""bf_assign_groups on the MI355X (csrc/bf_assign.hip: k_assign_vote, k_assign_box, k_assign_pick) against tests/assign_ref.py,
the numpy restatement.

Bar.  After an event's pixel the operator is integer counts, maxima and smallest indices, and the pixel is the scatter
kernel's own expression on np_ref.warp's arithmetic with the host's sine and cosine: every comparison with the restatement is
EQUALITY of gid, score, counts and info, no tolerance.  The alternation with bf_run_groups is teacher-forced: the device's own
models go into the restatement, so the ids of every round have one right answer; its end is held to the semantic bars of
tests/test_assign_cpu.py (recall >= 0.99, group 1's median flow within 5 px/s of the patch's velocity)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import segment_scene as scene
from test_gpu_groups import fields, seeded_models, to_accel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = scene.H, scene.W
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000
INFO_KEYS = ("models", "rows", "cols", "assigned", "unassigned", "changed", "max_score")


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def acc(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    yield a
    a.close()


def upload(a, sl):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


def two_models():
    return [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity((300.0, -200.0))]


def info_dict(info):
    return {k: getattr(info, k) for k in INFO_KEYS}


def same(dev, ref, what):
    gid, score, counts, info = dev
    rgid, rscore, rcounts, rinfo = ref
    print("%s: counts %s, info %s" % (what, counts.tolist(), info_dict(info)))
    assert info_dict(info) == rinfo, (what, info_dict(info), rinfo)
    assert counts.tolist() == rcounts.tolist(), what
    bad = np.flatnonzero((gid != rgid) | (score != rscore))
    assert bad.size == 0, (what, bad[:8], gid[bad[:8]], rgid[bad[:8]], score[bad[:8]], rscore[bad[:8]])
    assert gid.dtype == np.int32 and score.dtype == np.int32
    assert gid.tobytes() == rgid.tobytes() and score.tobytes() == rscore.tobytes(), what


def dev_bytes(r):
    return r[0].tobytes() + r[1].tobytes() + r[2].tobytes() + bytes(r[3])


_REF = {}


def ref_assign(sc, name, models, scale, margin=0, min_score=1, prior=None):
    """The restatement of one call, computed once per name and never changed."""
    if name not in _REF:
        r = ar.assign(sc, models, scale, (H, W), margin, min_score, prior)
        for a in r[:3]:
            a.setflags(write=False)
        _REF[name] = r
    return _REF[name]


# ---- 1. scales, margins, with and without a prior ----

@pytest.mark.parametrize("margin", [0, 6])
@pytest.mark.parametrize("scale", [1, 3, 5])
def test_two_models_first_round_and_round_with_a_prior(accel_mod, sc, scale, margin):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=scale * H + scale, max_cols=scale * W + scale)
    try:
        upload(a, sc)
        ms = two_models()
        r1 = ref_assign(sc, ("first", scale, margin), ms, scale, margin)
        d1 = a.assign_groups(to_accel(accel_mod, ms), scale, (H, W), margin=margin)
        same(d1, r1, "first round")
        assert r1[3]["rows"] == scale * (H - 1 + 2 * margin) + scale
        # the result was installed: it is the prior of the second round
        r2 = ref_assign(sc, ("second", scale, margin), ms, scale, margin, prior=r1[0])
        d2 = a.assign_groups(to_accel(accel_mod, ms), scale, (H, W), margin=margin, use_prior=True)
        same(d2, r2, "round with a prior")
        assert 0 < r2[3]["changed"] < r1[3]["changed"]
    finally:
        a.close()


# ---- 2. model counts ----

def test_one_model(accel_mod, sc, acc):
    upload(acc, sc)
    ms = two_models()[:1]
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W)), ref_assign(sc, "one", ms, 3), "K = 1")


def test_sixty_four_models_with_rotation_and_divergence(accel_mod, sc, acc):
    upload(acc, sc)
    ms = seeded_models(64)
    r = ref_assign(sc, "k64", ms, 3)
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W)), r, "K = 64")
    assert len(set(r[0].tolist())) > 8, "the seeded models must compete"
    r2 = ref_assign(sc, "k64 prior", ms, 3, prior=r[0])
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W), use_prior=True), r2, "K = 64 with a prior")


# ---- 3. priors with -1, thresholds, models that leave the window ----

def test_prior_holding_minus_ones(accel_mod, sc, acc):
    upload(acc, sc)
    ms = two_models()
    prior = (np.arange(len(sc["t"])) % 3 - 1).astype(np.int32)   # -1, 0, 1, -1, ...
    acc.set_groups(prior, 2)
    r = ref_assign(sc, "minus ones", ms, 3, prior=prior)
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W), use_prior=True), r, "prior with -1s")


def test_min_score_above_some_best_scores(accel_mod, sc, acc):
    upload(acc, sc)
    ms = two_models()
    r = ref_assign(sc, "min score", ms, 3, min_score=12)
    assert 0.05 * len(r[0]) < r[3]["unassigned"] < 0.95 * len(r[0]), r[3]
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W), min_score=12), r, "min_score 12")


def test_a_model_that_sends_most_events_outside(accel_mod, sc, acc):
    upload(acc, sc)
    ms = [ar.model_of_velocity((4000.0, -3000.0)), ar.model_of_velocity(scene.V_BACKGROUND)]
    w = ar.window(3, (H, W), 0)
    inside, _, _ = ar.pixels(sc, ms[0], w, 3)
    assert 0 < inside.sum() < 0.5 * len(inside)
    same(acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W)), ref_assign(sc, "far", ms, 3), "far model")
    alone = ms[:1]
    r = ref_assign(sc, "far alone", alone, 3)
    assert r[3]["unassigned"] >= int((~inside).sum())
    same(acc.assign_groups(to_accel(accel_mod, alone), 3, (H, W)), r, "far model alone")


def test_a_pile_beyond_sixteen_bits(accel_mod):
    n = 70000
    sl = dict(fr_x=np.full(n, 7, np.int32), fr_y=np.full(n, 9, np.int32), t=(np.arange(n) * 400).astype(np.int64))
    sl["fr_x"][-3:] = (0, 11, 7)
    sl["fr_y"][-3:] = (0, 3, 10)
    ms = [gr.oracle.Model(), ar.model_of_velocity((500.0, 0.0))]
    a = accel_mod.Accel(device=0, max_events=n, max_rows=64, max_cols=64)
    try:
        upload(a, sl)
        for scale in (1, 3):
            r = ar.assign(sl, ms, scale, (12, 16))
            assert r[3]["max_score"] >= n - 4 > 65535
            same(a.assign_groups(to_accel(accel_mod, ms), scale, (12, 16)), r, "pile at scale %d" % scale)
    finally:
        a.close()


@pytest.mark.parametrize("scale,margin", [(9, 1), (1, 0)])
def test_a_small_odd_sensor_at_the_largest_scale(accel_mod, scale, margin):
    """The smallest shape with the largest halo of k_assign_box (scale 9: 4 words), tiles cut on both axes of the 315 x 603 window
    (9 x 32 + 27 rows, 9 x 64 + 27 columns) and a last wave of 44 events; scale 1 is the same slice without the box sum."""
    res, n = (33, 65), 300
    rng = np.random.default_rng(11)
    sl = dict(fr_x=rng.integers(0, res[0], n).astype(np.int32), fr_y=rng.integers(0, res[1], n).astype(np.int32),
              t=np.sort(rng.integers(0, 30_000_000, n)).astype(np.int64))
    ms = [gr.oracle.Model(), ar.model_of_velocity((150.0, -80.0)), ar.model_of_velocity((-90.0, 40.0))]
    a = accel_mod.Accel(device=0, max_events=n, max_rows=640, max_cols=640)
    try:
        upload(a, sl)
        r1 = ar.assign(sl, ms, scale, res, margin)
        assert (r1[3]["rows"], r1[3]["cols"]) == (scale * (res[0] - 1 + 2 * margin) + scale, scale * (res[1] - 1 + 2 * margin) + scale)
        assert len(set(r1[0].tolist())) > 1, "the models must compete"
        same(a.assign_groups(to_accel(accel_mod, ms), scale, res, margin=margin), r1, "first round")
        r2 = ar.assign(sl, ms, scale, res, margin, prior=r1[0])
        same(a.assign_groups(to_accel(accel_mod, ms), scale, res, margin=margin, use_prior=True), r2, "round with a prior")
    finally:
        a.close()


# ---- 4. storage order, repeatability, state ----

def test_sorted_storage_gives_the_same_bytes_and_two_runs_agree(accel_mod, sc, acc):
    ms2, ms64 = to_accel(accel_mod, two_models()), to_accel(accel_mod, seeded_models(64))
    prior = (np.arange(len(sc["t"])) % 3 - 1).astype(np.int32)

    def calls():
        out = [acc.assign_groups(ms2, 3, (H, W), install=False), acc.assign_groups(ms2, 3, (H, W), install=False),
               acc.assign_groups(ms64, 5, (H, W), margin=6, install=False)]
        acc.set_groups(prior, 2)
        out.append(acc.assign_groups(ms2, 1, (H, W), use_prior=True, install=False))
        return [dev_bytes(r) for r in out]

    upload(acc, sc)
    plain = calls()
    assert plain[0] == plain[1], "two runs of one call"
    upload(acc, sc)
    acc.set_groups(gr.scene_groups(sc), 4)
    acc.run_groups(4, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)   # (the events are now stored sorted, with a permutation)
    assert calls() == plain
    same(acc.assign_groups(ms2, 3, (H, W), install=False), ref_assign(sc, ("first", 3, 0), two_models(), 3), "sorted storage")


def test_install_feeds_run_groups_and_no_install_leaves_the_grouping(accel_mod, sc, acc):
    ms = to_accel(accel_mod, two_models())
    warm = to_accel(accel_mod, two_models())

    def solve():
        m, i, q = acc.run_groups(2, 3, (H, W), (30, 40), MIN_EVENTS, warm=warm, hard_iter_cap=HARD_CAP)
        return b"".join(fields(x) for x in m) + b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    upload(acc, sc)
    gid, _, counts, _ = acc.assign_groups(ms, 3, (H, W), install=True)
    installed = solve()
    upload(acc, sc)
    acc.set_groups(gid, 2)
    by_hand = solve()
    assert installed == by_hand
    # install = 0: the grouping set by hand stays (other models, so that the result differs from it)
    upload(acc, sc)
    acc.set_groups(gid, 2)
    other, _, _, _ = acc.assign_groups(ms[::-1], 3, (H, W), install=False)
    assert (other != gid).any()
    assert solve() == by_hand
    # ... and before any grouping is held, install = 0 leaves none
    upload(acc, sc)
    acc.assign_groups(ms, 3, (H, W), install=False)
    with pytest.raises(accel_mod.BfError) as e:
        acc.run_groups(2, 3, (H, W), GUARD, MIN_EVENTS)
    assert e.value.code == accel_mod.BF_ERR_STATE


def test_the_slices_state_is_untouched(accel_mod, sc, acc):
    upload(acc, sc)
    acc.set_cloud(scene.SCALE, H, W)
    nx, ny = scene.flow_of(scene.V_BACKGROUND)
    acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    acc.segment(**scene.OPTS)

    def state():
        lab, comps, cl = acc.segment_get()
        return lab.tobytes() + comps.tobytes() + cl.tobytes() + b"".join(x.tobytes() for x in acc.writeout_events())

    before = state()
    acc.assign_groups(to_accel(accel_mod, two_models()), 3, (H, W), margin=6)
    acc.assign_groups(to_accel(accel_mod, two_models()), 1, (H, W), use_prior=True)
    assert state() == before


# ---- 5. errors ----

def test_every_error_code(accel_mod, sc):
    A = accel_mod
    a = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    ms = to_accel(A, two_models())

    def code(fn):
        with pytest.raises(A.BfError) as e:
            fn()
        return e.value.code

    try:
        assert code(lambda: a.assign_groups(ms, 3, (H, W))) == A.BF_ERR_STATE                     # before an upload
        upload(a, sc)
        assert code(lambda: a.assign_groups(ms, 3, (H, W), use_prior=True)) == A.BF_ERR_STATE     # no grouping held
        for kw in (dict(scale=2), dict(scale=11), dict(margin=-1), dict(min_score=0)):
            args = dict(scale=3, sensor_res=(H, W))
            args.update(kw)
            assert code(lambda: a.assign_groups(ms, **args)) == A.BF_ERR_ARG, kw
        assert code(lambda: a.assign_groups([], 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.assign_groups([ms[0]] * 65, 3, (H, W))) == A.BF_ERR_ARG
        a.set_groups(np.zeros(len(sc["t"]), np.int32), 3)
        assert code(lambda: a.assign_groups(ms, 3, (H, W), use_prior=True)) == A.BF_ERR_ARG       # a prior with K = 3, two models
        o = A.AssignOpts(3, H, W, 0, 1, 0, 0, 0)
        assert a.L.bf_assign_groups(a.h, ctypes.byref(o), None, 2, None, None, None, None) == A.BF_ERR_ARG   # NULL models
        assert code(lambda: a.assign_groups([ms[0]] * 64, 9, (1000, 1000))) == A.BF_ERR_CAPACITY   # 64 x 9000 x 9000 words
        a.upload_events(sc["fr_x"], sc["fr_y"], sc["t"], noise=np.zeros(len(sc["t"]), np.uint8))
        assert code(lambda: a.assign_groups(ms, 3, (H, W))) == A.BF_ERR_ARG                       # a noise mask
        # zero events: BF_OK, everything zero
        a.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        gid, score, counts, info = a.assign_groups(ms, 3, (H, W))
        assert len(gid) == 0 and len(score) == 0 and not counts.any() and not any(info_dict(info).values())
    finally:
        a.close()


# ---- 6. alternation with bf_run_groups ----

def refit(A, a, helper, sc, gid, models):
    """Every group from its current model: bf_run_groups, and a group whose window exceeds the LDS one after the other on a
    helper context.  -> (models, iterations, median flows)."""
    K = len(models)
    m, infos, _ = a.run_groups(K, 3, (H, W), GUARD, MIN_EVENTS, warm=models, hard_iter_cap=HARD_CAP)
    u, v = a.compute_uv()
    out, its, flows = list(models), [], []
    for g in range(K):
        idx = np.flatnonzero(gid == g)
        rc, it, mg, ug, vg = infos[g].rc, infos[g].iterations, m[g], u[idx], v[idx]
        if rc == A.BF_ERR_CAPACITY:
            helper.upload_events(sc["fr_x"][idx], sc["fr_y"][idx], sc["t"][idx])
            helper.set_cloud(3, H, W)
            helper.set_model(models[g])
            o = helper.default_opts()
            o.res_x, o.res_y, o.min_events, o.hard_iter_cap = GUARD[0], GUARD[1], MIN_EVENTS, HARD_CAP
            rc, mg, info = helper.run(o)
            it = info.iterations
            ug, vg = helper.compute_uv()
        if rc == A.BF_OK:
            out[g] = mg
        its.append(it)
        flows.append((float(np.median(ug)), float(np.median(vg))) if len(idx) else (0.0, 0.0))
    return out, its, flows


@pytest.fixture(scope="module")
def device_alternation(accel_mod, sc, acc):
    """Five alternations (two rounds + refit) from the failed seed through Accel, every round teacher-forced against the
    restatement: (models, gid, records [changed, counts, iterations], flows of the last refit)."""
    A = accel_mod
    helper = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        models = to_accel(A, [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity((11.0, -45.0))])
        upload(acc, sc)
        prior, flows, records = None, None, []
        for alt in range(5):
            changed = None
            for _ in range(2):
                dev = acc.assign_groups(models, 3, (H, W), use_prior=prior is not None)
                same(dev, ar.assign(sc, models, 3, (H, W), prior=prior), "alternation %d" % alt)   # teacher-forced
                changed = dev[3].changed if changed is None else changed
                prior = dev[0]
            models, its, flows = refit(A, acc, helper, sc, prior, models)
            records.append([changed] + dev[2].tolist() + its)
            rec, pur = ar.recall_purity(sc, prior)
            print("alternation %d: recall %.4f purity %.4f iterations %s flows %s" % (alt + 1, rec, pur, its, flows))
        return models, prior, records, flows
    finally:
        helper.close()


def test_alternation_from_the_failed_seed(sc, device_alternation):
    _, gid, _, flows = device_alternation
    rec, _ = ar.recall_purity(sc, gid)
    assert rec >= 0.99
    assert abs(flows[1][0] - scene.V_PATCH[0]) <= 5.0 and abs(flows[1][1] - scene.V_PATCH[1]) <= 5.0, flows


def test_motion_assigner_device_paths(accel_mod, sc, device_alternation, tmp_path):
    """tests/cpp/test_motion_assign.cpp linked against the product library: assign() equals the restatement, alternate() -- the
    grouped refit, the background group through the helper context -- equals the alternation through Accel above
    (tests/test_assign_cpu.py holds the host paths to the restatement)."""
    import test_assign_cpu as cpu
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_motion_assign")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_motion_assign.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ev, mf, prefix = str(tmp_path / "events.txt"), str(tmp_path / "models.bin"), str(tmp_path / "out_")
    with open(ev, "w") as f:
        for a, b, c in zip(sc["fr_x"].tolist(), sc["fr_y"].tolist(), sc["t"].tolist()):
            f.write("%d %d %d\n" % (a, b, c))
    cand = [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity((11.0, -45.0))]
    with open(mf, "wb") as f:
        for m in to_accel(accel_mod, cand):
            f.write(bytes(m))
    r = subprocess.run([exe, ev, mf, "2", "3", str(H), str(W), "0", "1", str(GUARD[0]), str(GUARD[1]), str(MIN_EVENTS), str(HARD_CAP),
                        "2", "5", prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode().splitlines()[0] == "path device"
    first = ar.assign(sc, cand, 3, (H, W))
    second = ar.assign(sc, cand, 3, (H, W), prior=first[0])
    assert np.fromfile(prefix + "first.i32", dtype=np.int32).tobytes() == cpu.flat(first).tobytes()
    assert np.fromfile(prefix + "second.i32", dtype=np.int32).tobytes() == cpu.flat(second).tobytes()
    models, gid, records, _ = device_alternation
    assert np.fromfile(prefix + "records.i32", dtype=np.int32).reshape(-1, 6).tolist() == records
    assert np.fromfile(prefix + "gid.i32", dtype=np.int32).tobytes() == gid.tobytes()
    raw = open(prefix + "models.bin", "rb").read()
    sz = ctypes.sizeof(accel_mod.Model)
    for k in range(2):
        assert fields(accel_mod.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz])) == fields(models[k]), k
