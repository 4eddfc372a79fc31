"""bf_project_groups on the MI355X (csrc/bf_project.hip: k_project_vote, k_project_compose; the box sum of bf_assign.hip) against
tests/project_groups_ref.py, the numpy restatement.

Bar.  After an event's pixel the operator is integer counts, sums, maxima and smallest indices, and the pixel is
bf_assign_groups' own (tests/test_gpu_assign.py holds it to the restatement): every comparison is EQUALITY of the three images,
the per-group scores and the info, no tolerance.  The end-to-end case is teacher-forced -- the device's own ids and models go
into the restatement -- and its score is held to the bar of tests/test_project_groups_cpu.py: the two-model grouping reaches
1.5 x the contrast of the slice under one model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import project_groups_ref as pr
import segment_scene as scene
from test_gpu_groups import fields, seeded_models, to_accel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = scene.H, scene.W
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def truth(sc):
    ids, ms = pr.scene_truth(sc)
    ids.setflags(write=False)
    return ids, ms


@pytest.fixture(scope="module")
def acc(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    yield a
    a.close()


def upload(a, sl):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


def info_dict(info):
    return {k: getattr(info, k) for k in pr.INFO_FIELDS}


def score_rows(scores):
    return [[getattr(s, f) for f in pr.SCORE_FIELDS] for s in scores]


def same(dev, ref, what):
    img, scores, info = dev
    print("%s: info %s" % (what, info_dict(info)))
    assert info_dict(info) == ref["info"], (what, info_dict(info), ref["info"])
    assert score_rows(scores) == [[s[f] for f in pr.SCORE_FIELDS] for s in ref["scores"]], what
    for k, dt in (("count", np.uint32), ("label", np.int32), ("bgr", np.uint8)):
        assert img[k].dtype == dt and img[k].shape == ref[k].shape, (what, k, img[k].shape, ref[k].shape)
        bad = np.argwhere(img[k] != ref[k])
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist(), [(img[k][tuple(b)], ref[k][tuple(b)]) for b in bad[:4]])
        assert img[k].tobytes() == ref[k].tobytes(), (what, k)


def dev_bytes(r):
    img, scores, info = r
    return img["count"].tobytes() + img["label"].tobytes() + img["bgr"].tobytes() + b"".join(bytes(s) for s in scores) + bytes(info)


_REF = {}


def ref_project(sl, name, ids, models, scale, sensor_res=(H, W), margin=0, gain=8):
    """The restatement of one call, computed once per name and never changed."""
    if name not in _REF:
        r = pr.project(sl, ids, models, scale, sensor_res, margin, gain)
        for k in ("count", "label", "bgr"):
            r[k].setflags(write=False)
        _REF[name] = r
    return _REF[name]


# ---- 1. the scene under its true grouping: scales, margins ----

@pytest.mark.parametrize("margin", [0, 6])
@pytest.mark.parametrize("scale", [1, 3, 5])
def test_scene_truth_grouping(accel_mod, sc, truth, scale, margin):
    ids, ms = truth
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=scale * H + scale, max_cols=scale * W + scale)
    try:
        upload(a, sc)
        a.set_groups(ids, 2)
        r = ref_project(sc, ("truth", scale, margin), ids, ms, scale, margin=margin)
        same(a.project_groups(to_accel(accel_mod, ms), scale, (H, W), margin=margin), r, "truth")
        assert r["info"]["rows"] == scale * (H + 2 * margin) and r["info"]["unassigned"] == 0
        if margin == 0 and scale in (1, 3):   # the table of DESIGN section 17
            assert r["info"]["sum_sq"] == {1: 647362, 3: 5837588}[scale]
    finally:
        a.close()


# ---- 2. group counts, ids of -1, empty groups, outside ----

def test_one_group(accel_mod, sc, acc):
    upload(acc, sc)
    ids = np.zeros(len(sc["t"]), np.int32)
    ms = [ar.model_of_velocity(scene.V_BACKGROUND)]
    acc.set_groups(ids, 1)
    r = ref_project(sc, "one", ids, ms, 3)
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W)), r, "K = 1")
    assert r["info"]["sum_sq"] == 3135808


def ids64(n):
    """Ids -1 .. 63 spread over the slice, groups 5 and 40 empty."""
    ids = ((np.arange(n) * 7) % 65 - 1).astype(np.int32)
    ids[(ids == 5) | (ids == 40)] = -1
    return ids


def test_sixty_four_groups_with_rotation_and_divergence(accel_mod, sc, acc):
    upload(acc, sc)
    ids, ms = ids64(len(sc["t"])), seeded_models(64)
    acc.set_groups(ids, 64)
    r = ref_project(sc, "k64", ids, ms, 3)
    assert r["info"]["unassigned"] > 0 and r["scores"][5]["events"] == 0 == r["scores"][40]["events"]
    assert len(set(r["label"].ravel().tolist())) > 32 and r["scores"][13]["pixels_owned"] > 0   # (colours beyond the palette's 12)
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W), gain=40), ref_project(sc, "k64 gain", ids, ms, 3, gain=40), "K = 64")
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W)), r, "K = 64, default gain")


def test_a_model_that_sends_three_quarters_of_a_group_outside(accel_mod, sc, truth, acc):
    upload(acc, sc)
    ids = truth[0]
    ms = [ar.model_of_velocity((5400.0, -4050.0)), ar.model_of_velocity(scene.V_PATCH)]
    acc.set_groups(ids, 2)
    r = ref_project(sc, "far", ids, ms, 3)
    g0 = r["scores"][0]
    assert 0.2 * g0["events"] <= g0["inside"] <= 0.25 * g0["events"] and r["info"]["outside"] == g0["events"] - g0["inside"], g0
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W)), r, "far model")


# ---- 3. windows that are no multiple of the box kernel's 32 x 64 tile ----

def random_slice(n, rows, cols, seed, duration_ns=30_000_000):
    rng = np.random.default_rng(seed)
    return dict(fr_x=rng.integers(0, rows, n).astype(np.int32), fr_y=rng.integers(0, cols, n).astype(np.int32),
                t=np.sort(rng.integers(0, duration_ns, n)).astype(np.int64))


@pytest.mark.parametrize("res", [(1, 1), (33, 65)])
def test_small_and_odd_sensors(accel_mod, res):
    sl = random_slice(2000, res[0], res[1], seed=3)
    ids = (np.arange(2000) % 4 - 1).astype(np.int32)
    ms = [gr.oracle.Model(), ar.model_of_velocity((150.0, -80.0)), ar.model_of_velocity((-90.0, 40.0))]
    a = accel_mod.Accel(device=0, max_events=2000, max_rows=512, max_cols=512)
    try:
        upload(a, sl)
        a.set_groups(ids, 3)
        for scale, margin in ((1, 0), (3, 0), (3, 2), (9, 1)):
            r = pr.project(sl, ids, ms, scale, res, margin)
            # (a sensor of one pixel has wsx = 0: without a margin the window test rejects every event)
            assert (r["info"]["pixels"] > 0) == (res != (1, 1) or margin > 0) and r["info"]["outside"] > 0
            same(a.project_groups(to_accel(accel_mod, ms), scale, res, margin=margin), r, "%s at scale %d, margin %d" % (res, scale, margin))
    finally:
        a.close()


# ---- 4. contention, squares beyond 32 bits, many groups on one row ----

def test_a_pile_of_70000_events_on_one_pixel(accel_mod):
    n = 70000
    sl = dict(fr_x=np.full(n, 7, np.int32), fr_y=np.full(n, 9, np.int32), t=(np.arange(n) * 400).astype(np.int64))
    ids = np.zeros(n, np.int32)
    ms = [gr.oracle.Model()]
    a = accel_mod.Accel(device=0, max_events=n, max_rows=64, max_cols=64)
    try:
        upload(a, sl)
        a.set_groups(ids, 1)
        for scale in (1, 3):
            r = pr.project(sl, ids, ms, scale, (12, 16))
            assert r["scores"][0]["max"] == n and r["info"]["sum_sq"] == scale * scale * n * n > 1 << 32
            same(a.project_groups(to_accel(accel_mod, ms), scale, (12, 16)), r, "pile at scale %d" % scale)
    finally:
        a.close()


def test_3000_events_of_64_groups_on_one_pixel_row(accel_mod):
    n = 3000
    rng = np.random.default_rng(9)
    sl = dict(fr_x=np.full(n, 5, np.int32), fr_y=rng.integers(0, 40, n).astype(np.int32), t=np.sort(rng.integers(0, 1000, n)).astype(np.int64))
    ids = rng.integers(0, 64, n).astype(np.int32)
    ms = [gr.oracle.Model()] * 64   # (t < 1 us: no model moves an event; every group lands on the row)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=64, max_cols=128)
    try:
        upload(a, sl)
        a.set_groups(ids, 64)
        for scale in (1, 3):
            r = pr.project(sl, ids, ms, scale, (12, 40))
            assert r["info"]["pixels"] == (39 if scale == 1 else 3 * 117) and all(s["pixels_hit"] > 0 for s in r["scores"])
            same(a.project_groups(to_accel(accel_mod, ms), scale, (12, 40)), r, "one row at scale %d" % scale)
    finally:
        a.close()


# ---- 5. storage order, repeatability, the assignment's buffers, state ----

def test_three_storage_orders_give_the_same_bytes_and_two_runs_agree(accel_mod, sc, truth, acc):
    ids, ms = truth
    ms2, ms64, i64 = to_accel(accel_mod, ms), to_accel(accel_mod, seeded_models(64)), ids64(len(sc["t"]))

    def calls():
        acc.set_groups(ids, 2)
        out = [acc.project_groups(ms2, 3, (H, W)), acc.project_groups(ms2, 3, (H, W)), acc.project_groups(ms2, 1, (H, W), margin=6)]
        acc.set_groups(i64, 64)
        out.append(acc.project_groups(ms64, 5, (H, W)))
        return [dev_bytes(r) for r in out]

    upload(acc, sc)
    plain = calls()
    assert plain[0] == plain[1], "two runs of one call"
    upload(acc, sc)
    acc.run_tiles(4, 4, 3, (H, W), (30, 40), MIN_EVENTS)   # (the events are now stored sorted by tile, with a permutation)
    assert calls() == plain
    upload(acc, sc)
    acc.set_groups(gr.scene_groups(sc), 4)
    acc.run_groups(4, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)   # (... sorted by group)
    assert calls() == plain
    acc.set_groups(ids, 2)
    same(acc.project_groups(ms2, 3, (H, W)), ref_project(sc, ("truth", 3, 0), ids, ms, 3), "sorted storage")


def test_alternating_with_assign_groups_on_one_context(accel_mod, sc, truth, acc):
    ids, ms = truth
    ms2 = to_accel(accel_mod, ms)
    assign_bytes = lambda r: r[0].tobytes() + r[1].tobytes() + r[2].tobytes() + bytes(r[3])
    upload(acc, sc)
    acc.set_groups(ids, 2)
    p_alone = [dev_bytes(acc.project_groups(ms2, s, (H, W))) for s in (3, 1)]
    upload(acc, sc)
    acc.set_groups(ids, 2)
    a_alone = [assign_bytes(acc.assign_groups(ms2, s, (H, W), use_prior=True, install=False)) for s in (3, 1)]
    upload(acc, sc)
    acc.set_groups(ids, 2)
    for _ in range(2):
        for i, s in enumerate((3, 1)):
            assert assign_bytes(acc.assign_groups(ms2, s, (H, W), use_prior=True, install=False)) == a_alone[i]
            assert dev_bytes(acc.project_groups(ms2, s, (H, W))) == p_alone[i]


def test_after_an_installed_assignment(accel_mod, sc, truth, acc):
    ms = truth[1]
    upload(acc, sc)
    gid, _, _, _ = acc.assign_groups(to_accel(accel_mod, ms), 3, (H, W), install=True)
    assert (gid == -1).any()
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W)), pr.project(sc, gid, ms, 3, (H, W)), "installed")


def test_the_slices_state_is_untouched(accel_mod, sc, truth, acc):
    ids, ms = truth
    lattice = accel_mod.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)

    def sequence(project):
        upload(acc, sc)
        acc.set_cloud(scene.SCALE, H, W)
        nx, ny = scene.flow_of(scene.V_BACKGROUND)
        acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
        acc.segment(**scene.OPTS)
        acc.set_groups(gr.scene_groups(sc), 4)
        acc.global_set_window(1, 5)
        acc.global_search(lattice, want_surface=False)
        acc.global_hold_best()

        def state():
            lab, comps, cl = acc.segment_get()
            return lab.tobytes() + comps.tobytes() + cl.tobytes() + b"".join(x.tobytes() for x in acc.writeout_events()) + \
                b"".join(v.tobytes() for v in acc.global_get_events().values()) + \
                b"".join(v.tobytes() for v in acc.global_get_flow().values()) + b"".join(x.tobytes() for x in acc.get_time_img())

        before = state()
        if project:
            four = to_accel(accel_mod, [ms[1], ms[0], ms[0], ms[0]])
            acc.project_groups(four, 3, (H, W), margin=6)
            acc.project_groups(four, 1, (H, W), want=())
            assert state() == before
        # the held grouping: the grouped solve gives what it gives without the projection
        m, i, q = acc.run_groups(4, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
        return before + b"".join(fields(x) for x in m) + b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    assert sequence(True) == sequence(False)


# ---- 6. errors, zero events ----

def test_every_error_code(accel_mod, sc, truth):
    A = accel_mod
    ids, ms = truth
    a = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    ms = to_accel(A, ms)

    def code(fn):
        with pytest.raises(A.BfError) as e:
            fn()
        return e.value.code

    try:
        assert code(lambda: a.project_groups(ms, 3, (H, W))) == A.BF_ERR_STATE                     # before an upload
        upload(a, sc)
        assert code(lambda: a.project_groups(ms, 3, (H, W))) == A.BF_ERR_STATE                     # no grouping held
        a.set_groups(ids, 2)
        for kw in (dict(scale=2), dict(scale=11), dict(margin=-1), dict(margin=65537), dict(gain=0), dict(sensor_res=(0, W)),
                   dict(sensor_res=(H, 65537))):
            args = dict(scale=3, sensor_res=(H, W), want=())
            args.update(kw)
            assert code(lambda: a.project_groups(ms, **args)) == A.BF_ERR_ARG, kw
        assert code(lambda: a.project_groups([], 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.project_groups([ms[0]] * 65, 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.project_groups([ms[0]] * 3, 3, (H, W))) == A.BF_ERR_ARG              # the grouping has K = 2
        o = A.ProjectOpts(3, H, W, 0, 8)
        assert a.L.bf_project_groups(a.h, ctypes.byref(o), None, 2, None, None, None, None, None) == A.BF_ERR_ARG   # NULL models
        assert a.L.bf_project_groups(a.h, None, (A.Model * 2)(*ms), 2, None, None, None, None, None) == A.BF_ERR_ARG   # NULL opts
        assert a.L.bf_project_groups(None, None, None, 0, None, None, None, None, None) == A.BF_ERR_ARG
        a.set_groups(np.zeros(len(sc["t"]), np.int32), 64)
        assert code(lambda: a.project_groups([ms[0]] * 64, 9, (1000, 1000), want=())) == A.BF_ERR_CAPACITY   # 64 x 9000 x 9000 words
        # every output NULL is a valid call
        a.set_groups(ids, 2)
        assert a.L.bf_project_groups(a.h, ctypes.byref(o), (A.Model * 2)(*ms), 2, None, None, None, None, None) == A.BF_OK
        a.upload_events(sc["fr_x"], sc["fr_y"], sc["t"], noise=np.zeros(len(sc["t"]), np.uint8))
        a.set_groups(ids, 2)
        assert code(lambda: a.project_groups(ms, 3, (H, W))) == A.BF_ERR_ARG                       # a noise mask
    finally:
        a.close()


def test_zero_events(accel_mod, truth):
    a = accel_mod.Accel(device=0, max_events=16, max_rows=64, max_cols=64)
    try:
        a.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        a.set_groups(np.zeros(0, np.int32), 2)
        dev = a.project_groups(to_accel(accel_mod, truth[1]), 3, (12, 16))
        same(dev, pr.project(dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64)),
                             np.zeros(0, np.int32), truth[1], 3, (12, 16)), "zero events")
        assert not dev[0]["count"].any() and not dev[0]["bgr"].any() and (dev[0]["label"] == -1).all()
        assert not any(info_dict(dev[2]).values()) and not np.array(score_rows(dev[1])).any()
    finally:
        a.close()


# ---- 7. end to end: search, proposals, alternation, projection ----

@pytest.fixture(scope="module")
def device_objects(accel_mod, sc, acc):
    """search + propose_models(max_models=2) + the alternation of DESIGN section 15: (models, ids) as the device leaves them."""
    from test_gpu_assign import refit
    A = accel_mod
    helper = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(acc, sc)
        acc.global_set_window(1, 5)
        o = A.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)
        acc.global_search(o, want_surface=False)
        models, _, _ = acc.propose_models(o, max_models=2)
        assert len(models) == 2
        upload(acc, sc)
        prior = None
        for alt in range(5):
            changed = None
            for _ in range(2):
                dev = acc.assign_groups(models, 3, (H, W), use_prior=prior is not None)
                changed = dev[3].changed if changed is None else changed
                prior = dev[0]
            if alt > 0 and changed == 0:
                break
            models, _, _ = refit(A, acc, helper, sc, prior, models)
        return models, prior
    finally:
        helper.close()


def test_end_to_end_projection_of_the_found_objects(accel_mod, sc, acc, device_objects):
    models, gid = device_objects
    upload(acc, sc)
    acc.set_groups(gid, 2)
    dev = acc.project_groups(models, 3, (H, W))
    same(dev, pr.project(sc, gid, models, 3, (H, W)), "found objects")   # teacher-forced: the device's own ids and models
    acc.set_groups(np.zeros(len(gid), np.int32), 1)
    _, _, single = acc.project_groups(models[:1], 3, (H, W), want=())
    print("sum N^2: two objects %d, one group under the first model %d" % (dev[2].sum_sq, single.sum_sq))
    assert dev[2].sum_sq >= 1.5 * single.sum_sq


# ---- 8. bf::ObjectRenderer and the command line ----

def test_object_renderer_on_the_device_equals_accel(accel_mod, sc, truth, acc, tmp_path):
    """tests/cpp/test_object_render.cpp linked against the product library: render() takes bf_project_groups, and what it leaves
    and writes equals the restatement (tests/test_project_groups_cpu.py holds the host path to it) and Accel.project_groups."""
    import test_project_groups_cpu as cpu
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_object_render")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_object_render.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ids, ms = truth
    ref = cpu.program_case(exe, tmp_path, "scene", sc, ids, ms, 3, (H, W), margin=6, gain=5, expect_path="device")
    upload(acc, sc)
    acc.set_groups(ids, 2)
    same(acc.project_groups(to_accel(accel_mod, ms), 3, (H, W), margin=6, gain=5), ref, "Accel")
    cpu.program_case(exe, tmp_path, "k64", sc, ids64(len(sc["t"])), seeded_models(64), 1, (H, W), expect_path="device")
    empty = dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64))
    cpu.program_case(exe, tmp_path, "zero", empty, np.zeros(0, np.int32), ms, 3, (12, 16), expect_path="device")


def test_cli_objects_img_on_the_scene(sc, tmp_path):
    """bf_motion_compensator --objects=2 --objects-img on the scene written as an event file: the three files of the one slice,
    consistent with each other and with objects_0.txt, which has the bytes of a run without the flag; the score reaches the bar
    of the end-to-end case."""
    from better_flow_amd import synth
    exe = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")
    txt = str(tmp_path / "scene.txt")
    synth.write_txt(txt, sc)

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([exe, "--objects=2"] + extra + ["--res-x=%d" % H, "--res-y=%d" % W, "--quiet", "--img-prefix", str(out), txt],
                           cwd=str(out), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return out

    plain, img = run("plain", []), run("img", ["--objects-img", "--objects-img-gain=5"])
    assert sorted(os.listdir(str(plain))) == ["objects_0.txt"]
    assert sorted(os.listdir(str(img))) == ["objects_0.pgm", "objects_0.ppm", "objects_0.score.txt", "objects_0.txt"]
    assert open(str(img / "objects_0.txt"), "rb").read() == open(str(plain / "objects_0.txt"), "rb").read()
    R, C = 3 * H, 3 * W
    pgm = open(str(img / "objects_0.pgm"), "rb").read()
    head = b"P5\n%d %d\n65535\n" % (C, R)
    assert pgm.startswith(head) and len(pgm) == len(head) + 2 * R * C
    label = np.frombuffer(pgm[len(head):], dtype=">u2").astype(np.int32).reshape(R, C) - 1
    ppm = open(str(img / "objects_0.ppm"), "rb").read()
    head = b"P6\n%d %d\n255\n" % (C, R)
    assert ppm.startswith(head) and len(ppm) == len(head) + 3 * R * C
    rgb = np.frombuffer(ppm[len(head):], dtype=np.uint8).reshape(R, C, 3)
    lines = [ln.split() for ln in open(str(img / "objects_0.score.txt")).read().splitlines()]
    groups = [[int(v) for v in ln] for ln in lines[:-1]]
    info = dict(zip(pr.INFO_FIELDS, (int(v) for v in lines[-1][1:])))
    print(groups, info)
    table = [ln.split() for ln in open(str(img / "objects_0.txt")).read().splitlines()]
    assert len(groups) == 2 and lines[-1][0] == "info" and (info["models"], info["rows"], info["cols"]) == (2, R, C)
    # the score file, the label image and the colour image describe one projection
    assert [g[1] for g in groups] == [int(t[1]) for t in table[:2]] and info["unassigned"] == int(table[2][1])
    assert [g[4] for g in groups] == [int((label == k).sum()) for k in range(2)] and info["pixels"] == int((label >= 0).sum())
    assert ((rgb.max(axis=2) > 0) == (label >= 0)).all()
    assert (rgb[label == 1][:, 1:] == 0).all() and (rgb[label == 1][:, 0] > 0).all()   # group 1 is the palette's red
    assert sum(g[2] for g in groups) + info["outside"] + info["unassigned"] == len(sc["t"]) and info["sum"] <= 9 * sum(g[2] for g in groups)
    assert all(g[3] >= g[4] > 0 and g[5] > 0 for g in groups)
    # (the events' ids are not among the command line's outputs, so the projection cannot be formed a second time here: that the
    # writer's PGM is label_out + 1 and its PPM bgr_out, on the device, is test_object_renderer_on_the_device_equals_accel's)
    assert info["sum_sq"] >= 1.5 * 3135808   # (the slice under the background's model alone)
