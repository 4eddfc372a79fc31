"""Event groups on the CPU: the ABI of the new structs and symbols, the claims of DESIGN section 14 as conditions on the
restatement (tests/groups_ref.py over the CPU oracle) -- grouping by the truth recovers both motions of the two-motion scene,
the groups are order-stable in the reference, the segmentation's own cl_id is not a fitting membership --, and
bf::ObjectTasks' host path (host/better_flow/object_tasks.h) through the oracle-backed C-ABI stand-in, also as a stand-alone
ASan / UBSan program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import groups_ref as gr
import oracle
import segment_ref
import segment_scene as scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RES, GUARD, MIN_EVENTS, HARD_CAP = (scene.H, scene.W), (90, 120), 100, 20000


# ---- ABI ----

def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    from better_flow_amd import accel
    mirrors = {"bf_group_opts": accel.GroupOpts, "bf_group_info": accel.GroupInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bf_accel.h"', 'int main(void) {']
    for cname, m in mirrors.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in m._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0; }"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, m in mirrors.items():
        assert int(got[cname]) == ctypes.sizeof(m), cname
        for f, _ in m._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(m, f).offset, (cname, f)
    assert (ctypes.sizeof(accel.GroupOpts), ctypes.sizeof(accel.GroupInfo)) == (32, 32)


def test_symbols_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    for name in ("bf_set_groups", "bf_set_groups_from_segments", "bf_run_groups"):
        assert name in accel.EXPORTS and hasattr(lib, name), name
    for m in ("set_groups", "set_groups_from_segments", "run_groups"):
        assert callable(getattr(accel.Accel, m))


# ---- the scene's four groups on the restatement ----

@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def gid(sc):
    return gr.scene_groups(sc)


def both_orders(sc, gid, warm):
    f = gr.solve(sc, gid, 4, 3, RES, GUARD, MIN_EVENTS, warm=warm, hard_cap=HARD_CAP)
    r = gr.solve(sc, gid, 4, 3, RES, GUARD, MIN_EVENTS, warm=warm, hard_cap=HARD_CAP, reverse=True)
    for a, b in zip(f[0], r[0]):
        assert a.rc == b.rc == 0 and a.iterations == b.iterations, (a.iterations, b.iterations)
    worst = max(np.abs(f[3] - r[3]).max(), np.abs(f[4] - r[4]).max())   # (solve scatters back to upload order)
    print("forward / reversed: flows differ by at most %.3e px/s" % worst)
    assert worst <= 1e-4
    return f


def test_grouping_by_the_truth_recovers_both_motions_cold(sc, gid):
    res, _, _, u, v = both_orders(sc, gid, None)
    assert [r.events for r in res] == [9600, 501, 627, 341]
    assert [r.pixels for r in res] == [5382, 5400, 5022, 4158]
    assert [r.iterations for r in res] == [56, 21, 26, 14]
    mu = gr.median_flow(u, v, res[0].idx)
    print("patch: median flow (%.2f, %.2f) px/s" % mu)
    assert max(abs(mu[0] - scene.V_PATCH[0]), abs(mu[1] - scene.V_PATCH[1])) < 1.0
    for r in res[1:]:
        mu = gr.median_flow(u, v, r.idx)
        print("background box: median flow (%.2f, %.2f) px/s" % mu)
        assert max(abs(mu[0] - scene.V_BACKGROUND[0]), abs(mu[1] - scene.V_BACKGROUND[1])) < 6.0
    rest = gid < 0
    assert not u[rest].any() and not v[rest].any()


def test_warm_from_the_background_model(sc, gid):
    res, _, _, u, v = both_orders(sc, gid, gr.background_model())
    assert [r.iterations for r in res] == [83, 15, 11, 29]
    mu = gr.median_flow(u, v, res[0].idx)
    assert max(abs(mu[0] - scene.V_PATCH[0]), abs(mu[1] - scene.V_PATCH[1])) < 1.0


def test_the_segmentations_component_is_not_a_fitting_membership(sc):
    """The thresholded component keeps the patch's late leading edge only: fewer than 5 % of the patch's events, and a cold
    fit on them at scale 1 ends after one iteration with zero flow."""
    oc = oracle.Cloud(sc["fr_x"], sc["fr_y"], sc["t"])
    ow = oc.set_cloud(scene.SCALE, scene.H, scene.W)
    nx, ny = scene.flow_of(scene.V_BACKGROUND)
    oc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    T, cnt = oc.get_time_img(ow)
    seg = segment_ref.segment(T, cnt.astype(np.uint32), oc.pr_x, oc.pr_y, ow, **scene.OPTS)
    cl = np.asarray(seg["cl_id"] if isinstance(seg, dict) else seg.cl_id)
    K = int(cl.max()) + 1
    assert K == 1
    members = np.flatnonzero(cl == 0)
    assert sc["is_patch"][members].all()
    assert 0 < len(members) < 0.05 * int(sc["is_patch"].sum())
    res, _, _, u, v = gr.solve(sc, cl, 1, scene.SCALE, RES, GUARD, MIN_EVENTS, hard_cap=HARD_CAP)
    print("component: %d events, window %d x %d, %d iteration(s)" % (len(members), res[0].window.scale_img_x, res[0].window.scale_img_y,
                                                                       res[0].iterations))
    assert res[0].rc == 0 and res[0].iterations == 1 and not u.any() and not v.any()


# ---- bf::ObjectTasks' host path against the restatement ----

def build_tasks_program(out_dir, sanitize):
    exe = os.path.join(out_dir, "test_object_tasks" + ("_san" if sanitize else ""))
    extra = SAN if sanitize else []
    obj = exe + "_oracle.o"
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-ffp-contract=off"] + extra + ["-c", os.path.join(ROOT, "oracle", "bf_oracle.c"),
                                                                                    "-o", obj])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra"] + extra + [
        "-I" + os.path.join(ROOT, "better_flow_amd", "host"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
        os.path.join(ROOT, "tests", "cpp", "test_object_tasks.cpp"), os.path.join(ROOT, "tests", "shim", "bf_accel_oracle_shim.cpp"), obj,
        "-lm", "-o", exe])
    return exe


def write_events(path, sc, gid):
    with open(path, "w") as f:
        for a, b, c, g in zip(sc["fr_x"].tolist(), sc["fr_y"].tolist(), sc["t"].tolist(), gid.tolist()):
            f.write("%d %d %d %d\n" % (a, b, c, g))


def write_models(path, models):
    from better_flow_amd import accel
    with open(path, "wb") as f:
        for m in models:
            f.write(bytes(accel.Model(**{k: getattr(m, k) for k, _ in oracle.Model._fields_})))


def read_outputs(prefix, K, n):
    from better_flow_amd import accel
    raw = open(prefix + "models.bin", "rb").read()
    sz = ctypes.sizeof(accel.Model)
    models = [accel.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz]) for k in range(K)]
    infos = np.fromfile(prefix + "infos.i32", dtype=np.int32).reshape(K, 2)
    nxny = np.fromfile(prefix + "nxny.f64", dtype=np.float64)
    return models, infos, nxny[:n], nxny[n:]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_object_tasks_host_path_equals_the_restatement(sc, gid, tmp_path, sanitize):
    exe = build_tasks_program(str(tmp_path), sanitize)
    ev = str(tmp_path / "events.txt")
    write_events(ev, sc, gid)
    warm_file = str(tmp_path / "warm.bin")
    bgm = gr.background_model()
    write_models(warm_file, [bgm] * 4)
    n = len(gid)
    for warm, arg in ((None, "-"), (bgm, warm_file)):
        prefix = str(tmp_path / ("out_%s_" % ("warm" if warm else "cold")))
        r = subprocess.run([exe, ev, "4", "3", str(scene.H), str(scene.W), str(GUARD[0]), str(GUARD[1]), str(MIN_EVENTS), str(HARD_CAP),
                            arg, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert r.stdout.decode().splitlines()[0] == "path host"
        models, infos, nx, ny = read_outputs(prefix, 4, n)
        res, onx, ony, _, _ = gr.solve(sc, gid, 4, 3, RES, GUARD, MIN_EVENTS, warm=warm, hard_cap=HARD_CAP)
        for k, g in enumerate(res):
            assert (int(infos[k, 0]), int(infos[k, 1])) == (g.rc, g.iterations), k
            for f, _ in oracle.Model._fields_:
                a, b = getattr(models[k], f), getattr(g.model, f)
                assert np.array(a).tobytes() == np.array(b).tobytes() or a == b, (k, f, a, b)
        assert nx.tobytes() == onx.tobytes() and ny.tobytes() == ony.tobytes()
