"""The call-sequence table (scripts/ctx_sequence_table.py, tests/test_gpu_ctx_sequences.py): what every C-ABI entry that reads the
context's slice state returns after every ordered pair of the entries that change it.

One case = one fresh context: upload + bf_set_cloud, two MOVERS, then the fixed list of READERS.  One line per call --
    <case id> <call> <return code> <first 16 hex digits of the SHA-256 of the call's output bytes, "-" for a refused call>
-- so a mover that leaves one flag of the context other than it used to (stale flow, a stale segmentation, outputs in the wrong
order) shows as a changed code or digest of some reader behind it.  The slice is one fixed two-motion scene on a 48 x 64 sensor:
3000 events, scale 3, every run capped at 5 iterations."""
import hashlib

import numpy as np

from better_flow_amd import accel, synth

H, W, SCALE, ITER, N = 48, 64, 3, 5, 3000
V_A, V_B = (-40.0, 80.0), (300.0, -250.0)    # (row, column) px / s of the two motions


def flow_of(v):
    """(nx, ny) of Event::apply_project for an image velocity in px / s (tests/segment_scene.py)."""
    return v[0] * 1.27e-3, v[1] * 1.27e-3


def make_slice():
    """Exactly N events in ascending time: about two thirds moving with V_A, the rest with V_B."""
    a = synth.make_slice(2600, H, W, 0.030, seed=21, velocity=V_A)
    b = synth.make_slice(1400, H, W, 0.030, seed=22, velocity=V_B)
    cat = {k: np.concatenate([a[k], b[k]]) for k in ("fr_x", "fr_y", "t")}
    order = np.argsort(cat["t"], kind="stable")
    assert len(order) >= N
    idx = order[np.linspace(0, len(order) - 1, N).astype(np.int64)]
    return {k: np.ascontiguousarray(cat[k][idx]) for k in cat}


def model_of(v):
    nx, ny = flow_of(v)
    return accel.Model(cx=SCALE * H / 2.0, cy=SCALE * W / 2.0, total_dx=nx, total_dy=ny)


MODELS = (model_of(V_A), model_of(V_B))
GROUP_HALVES = lambda sl: (sl["fr_y"] >= W // 2).astype(np.int32)   # ids by column half


def _model_bytes(m):
    d = m.as_dict()
    return b"".join(np.float64(d[k]).tobytes() for k in sorted(d))


def _infos(infos):
    return np.array([(i.rc, i.iterations) for i in infos], dtype=np.int32).tobytes()


def _run(a, want_uv):
    o = a.default_opts()
    o.res_x, o.res_y, o.max_iter, o.min_events, o.want_uv = H, W, ITER, 50, want_uv
    rc, m, info = a.run(o)
    return np.int32([rc, info.iterations]).tobytes() + _model_bytes(m)


def _window(w):
    return np.int32([w.scale_img_x, w.scale_img_y]).tobytes() + np.float64([w.x_shift, w.y_shift]).tobytes()


def _run_tiles(a):
    models, infos = a.run_tiles(2, 2, SCALE, (H, W), (H // 2, W // 2), 64, max_iter=ITER)
    return b"".join(_model_bytes(m) for m in models) + _infos(infos)


def _local_run_tiles(a):
    st, rcs = a.local_run_tiles(2, 2, SCALE, 12, (H, W), (H // 2, W // 2), max_evaluations=40)
    return b"".join(bytes(s) for s in st) + np.int32(rcs).tobytes()


def _segment_groups(a):
    info = a.segment(above_s=0.35 * 0.030, min_count=2, min_pixels=4)
    return bytes(info) + np.int32([a.set_groups_from_segments()]).tobytes()


def _groups_run(a, sl):
    a.set_groups(GROUP_HALVES(sl), 2)
    models, infos, ginfo = a.run_groups(2, SCALE, (H, W), (H // 2, W // 2), 64, max_iter=ITER)
    return b"".join(_model_bytes(m) for m in models) + _infos(infos) + b"".join(bytes(g) for g in ginfo)


def _assign(a):
    gid, score, counts, info = a.assign_groups(MODELS, SCALE, (H, W), install=True)
    return gid.tobytes() + score.tobytes() + counts.tobytes() + bytes(info)


def _none(call):
    call()
    return b""


# name -> f(accel, slice) -> output bytes
MOVERS = (
    ("upload", lambda a, sl: _none(lambda: a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"]))),
    ("set_cloud", lambda a, sl: _window(a.set_cloud(SCALE, H, W))),
    ("project_reinit", lambda a, sl: _none(lambda: a.project_4param_reinit(0.2, -0.1, 70.0, 90.0, 1e-5, 2e-5))),
    ("project", lambda a, sl: _none(lambda: a.project_4param(-0.1, 0.15, 60.0, 100.0, -1e-5, 1e-5))),
    ("set_model", lambda a, sl: _none(lambda: a.set_model(MODELS[0]))),
    ("run", lambda a, sl: _run(a, 0)),
    ("run_uv", lambda a, sl: _run(a, 1)),
    ("run_tiles", lambda a, sl: _run_tiles(a)),
    ("local_run_tiles", lambda a, sl: _local_run_tiles(a)),
    ("segment_groups", lambda a, sl: _segment_groups(a)),
    ("groups_run", _groups_run),
    ("assign_install", lambda a, sl: _assign(a)),
)


def _project_groups(a):
    img, scores, info = a.project_groups(MODELS, SCALE, (H, W))
    return b"".join(img[k].tobytes() for k in ("count", "label", "bgr")) + b"".join(bytes(s) for s in scores) + bytes(info)


def _merge_scores(a):
    gain, inside, events, info = a.merge_scores(MODELS, SCALE, (H, W))
    return gain.tobytes() + inside.tobytes() + events.tobytes() + bytes(info)


def _segment_get(a):
    labels, comps, cl = a.segment_get(comps_cap=16)
    return labels.tobytes() + comps.tobytes() + cl.tobytes()


READERS = (
    ("compute_uv", lambda a: b"".join(x.tobytes() for x in a.compute_uv())),
    ("writeout_events", lambda a: b"".join(x.tobytes() for x in a.writeout_events())),
    ("get_time_img", lambda a: b"".join(x.tobytes() for x in a.get_time_img())),
    ("segment_get", _segment_get),
    ("set_groups_from_segments", lambda a: np.int32([a.set_groups_from_segments()]).tobytes()),
    ("project_groups", _project_groups),
    ("merge_scores", _merge_scores),
    ("projection_img_0", lambda a: a.projection_img(SCALE, H, W, show_final=False).tobytes()),
    ("projection_img_1", lambda a: a.projection_img(SCALE, H, W, show_final=True).tobytes()),
    ("color_time_img", lambda a: a.color_time_img(SCALE, H, W, show_final=True).tobytes()),
    ("local_iteration_step", lambda a: np.float64(a.local_iteration_step(0.1, -0.2)).tobytes()),
    ("stat_loop_form", lambda a: np.int64(a.get_stat("loop_form")).tobytes()),
    ("stat_one_kernel", lambda a: np.int64(a.get_stat("one_kernel")).tobytes()),
)

# Call kinds whose digest differed between two recordings of the parent's table: their return code is held, their digest is not.
NO_DIGEST = ()

CASES = [(m1, m2) for m1 in MOVERS for m2 in MOVERS]


def _line(cid, name, call):
    try:
        out = call()
        rc, digest = 0, "-" if name in NO_DIGEST else hashlib.sha256(out).hexdigest()[:16]
    except accel.BfError as e:
        rc, digest = e.code, "-"
    return "%s %s %d %s" % (cid, name, rc, digest)


def case_lines(accel_mod, sl, case, lib=None):
    """Runs one case on a fresh context and returns its lines: the two movers, then every reader."""
    (n1, f1), (n2, f2) = case
    cid = "%s+%s" % (n1, n2)
    kw = dict(max_events=N, max_rows=SCALE * H + SCALE, max_cols=SCALE * W + SCALE)
    if lib:
        kw["lib"] = lib
    a = accel_mod.Accel(**kw)
    try:
        a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        a.set_cloud(SCALE, H, W)
        lines = [_line(cid, "1:" + n1, lambda: f1(a, sl)), _line(cid, "2:" + n2, lambda: f2(a, sl))]
        lines += [_line(cid, name, lambda: f(a)) for name, f in READERS]
        return lines
    finally:
        a.close()


def table(accel_mod, lib=None):
    sl = make_slice()
    return [ln for case in CASES for ln in case_lines(accel_mod, sl, case, lib)]
