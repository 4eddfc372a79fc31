"""--flow-img / --flow-field and the per-pixel flow rule on the CPU.

* tests/flowimg_ref.py, the numpy restatement of the rule in include/bf_accel.h ("per-pixel flow"), against hand-computed
  cases: ownership under both rules, the truncation of the position, the x86 double -> uchar conversion of the saturation.
* The command line linked against the oracle-backed test shim, which has none of the bf_flow_* entries: the host builds the
  field from bf_writeout_events + bf_compute_uv (flow_field.h) and composes with frame_writer.h.  Every flow_N.ppm / flow_N.flo
  must equal the restatement fed with that slice's positions and flow from an oracle run of the same slices; the two engines
  must write the same bytes; and -o / frame_N.* must not change.
* better_flow_amd.flowio reads back what the command line wrote."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flowimg_ref as ref  # noqa: E402
from better_flow_amd import flowio, synth  # noqa: E402

H, W = 180, 240


# ---- 1. the restatement against hand-computed cases ----

def test_ownership_both_rules():
    pr_x, pr_y = np.array([3.2, 3.9, 7.0]), np.array([5.5, 5.1, 1.0])
    u, v = np.array([10.0, 20.0, 30.0]), np.array([1.0, 2.0, 3.0])
    o, U, V = ref.flow_field(pr_x, pr_y, u, v, None, 10, 12, ref.LAST_UPLOADED)
    assert o[3, 5] == 1 and U[3, 5] == 20.0 and V[3, 5] == 2.0
    o, U, V = ref.flow_field(pr_x, pr_y, u, v, None, 10, 12, ref.FIRST_UPLOADED)
    assert o[3, 5] == 0 and U[3, 5] == 10.0 and V[3, 5] == 1.0
    assert o[7, 1] == 2 and (o >= 0).sum() == 2 and U[0, 0] == 0.0
    # reversing the upload order with the opposite rule names the same events
    a, Ua, Va = ref.flow_field(pr_x[::-1], pr_y[::-1], u[::-1], v[::-1], None, 10, 12, ref.LAST_UPLOADED)
    assert np.array_equal(np.where(a >= 0, 2 - a, -1), o) and np.array_equal(Ua, U) and np.array_equal(Va, V)


def test_pixel_truncation_and_bounds():
    RX, RY = 9, 7
    pr_x = np.array([-0.7, -1.0, RX - 0.5, float(RX), np.nan, 1e300, 2.0])
    pr_y = np.array([0.0, 0.0, 1.0, 2.0, 3.0, 4.0, -0.999])
    one = np.ones(7)
    o, _, _ = ref.flow_field(pr_x, pr_y, one, one, None, RX, RY, ref.LAST_UPLOADED)
    assert o[0, 0] == 0                       # -0.7 truncates toward zero: inside
    assert o[RX - 1, 1] == 2                  # RES_X - 0.5 -> RES_X - 1
    assert o[2, 0] == 6                       # -0.999 -> 0
    assert sorted(o[o >= 0].tolist()) == [0, 2, 6]   # -1.0, RES_X, NaN, 1e300: outside


def test_saturation_and_hue_bytes():
    speeds = np.array([0.0, 0.5, 1.0, 1.04, 500.0, 1e6])
    a2, ls = ref.hs_values(speeds, np.zeros(6))           # flow along +u: atan2(0, u) = 0
    assert ref.to_uchar(ls).tolist() == [0, 228, 0, 1, 251, 255]
    assert ls[0] == -np.inf and abs(ls[1] + 28.07) < 0.01 and ls[5] == 255.0
    # (0 + 3.1416) * 180 / 3.1416 is 179.99999999999997 in double: half of it truncates to 89, not 90
    assert (0.0 + 3.1416) * 180 / 3.1416 < 180.0 and ref.to_uchar(a2).tolist() == [0, 89, 89, 89, 89, 89]
    assert ref.to_uchar(np.array([-3.0, np.nan, -np.inf, 300.0, 255.9])).tolist() == [253, 0, 0, 44, 255]
    # a NaN flow: H from NaN -> INT_MIN -> 0, S from std::min(255.0, NaN) = 255
    a2, ls = ref.hs_values(np.array([np.nan]), np.array([1.0]))
    assert ref.to_uchar(a2).tolist() == [0] and ref.to_uchar(ls).tolist() == [255]
    # 1.025 is not an integer boundary of log(speed) / log(1.025): 0.99999... or 1.00000...1 both truncate as stated
    import math
    assert ref.LOG_1025 == math.log(1.025)
    # directions: -u -> pi, +v -> pi / 2
    a2, _ = ref.hs_values(np.array([-5.0, 0.0]), np.array([0.0, 5.0]))
    assert ref.to_uchar(a2).tolist() == [int((math.pi + 3.1416) * 180 / 3.1416 / 2), int((math.pi / 2 + 3.1416) * 180 / 3.1416 / 2)]


def test_noise_and_empty_slice():
    pr = np.array([1.0, 1.0])
    o, U, V = ref.flow_field(pr, pr, np.array([4.0, 8.0]), np.array([0.0, 0.0]), np.array([0, 1], np.uint8), 4, 4, ref.LAST_UPLOADED)
    assert o[1, 1] == 0 and U[1, 1] == 4.0     # the flagged event does not own the pixel
    e = np.zeros(0)
    o, U, V = ref.flow_field(e, e, e, e, None, 4, 5, ref.FIRST_UPLOADED)
    bgr, hs = ref.color_flow(o, U, V)
    assert (o == -1).all() and (bgr == 255).all() and (hs == 0).all()      # all white
    assert (ref.flo_payload(o, U, V) == np.float32(1e9)).all()
    # colour: a saturated +u flow is H 89, S 255; the conversion's primaries
    o, U, V = ref.flow_field(np.array([0.0]), np.array([0.0]), np.array([1e4]), np.array([0.0]), None, 1, 1, ref.LAST_UPLOADED)
    bgr, hs = ref.color_flow(o, U, V)
    assert hs[0, 0].tolist() == [89, 255] and bgr[0, 0].tolist() == ref.hsv_to_bgr([89], [255], [255])[0].tolist()
    assert ref.hsv_to_bgr([0, 60, 120, 7], [255, 255, 255, 0], [255] * 4).tolist() == [[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255]]


# ---- 2. the command line through the stand-in library ----

@pytest.fixture(scope="module")
def oracle_cli():
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import build as shim_build
    return shim_build.build()


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = tmp_path_factory.mktemp("flowframes")
    sl = synth.make_slice(10000, H, W, 0.1, seed=5)
    txt, binary = str(d / "ev10k.txt"), str(d / "ev10k.bin")
    synth.write_txt(txt, sl)
    synth.write_bin(binary, sl)
    # a stream whose first slice trips the small-window guard (as in tests/test_stream_frames_cpu.py)
    rng = np.random.default_rng(7)
    k = 1500
    patch = {"fr_x": (50 + rng.integers(0, 4, k)).astype(np.int32), "fr_y": (60 + rng.integers(0, 4, k)).astype(np.int32),
             "t": np.sort(rng.integers(0, 40_000_000, k)).astype(np.int64)}
    rest = synth.make_slice(8000, H, W, 0.15, seed=9, t0_ns=40_000_000)
    guard = {key: np.concatenate([patch[key], rest[key]]) for key in ("fr_x", "fr_y", "t")}
    guard_txt = str(d / "guard.txt")
    synth.write_txt(guard_txt, guard)
    return {"txt": txt, "bin": binary, "guard": guard_txt}


def run_cli(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode()


def flow_run(exe, args, inp, out_dir, extra=("--flow-img", "--flow-field")):
    os.makedirs(out_dir)
    run_cli(exe, list(args) + list(extra) + ["--quiet", "--img-prefix", out_dir, "--video-name", os.path.join(out_dir, "out.avi"), inp], out_dir)
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def read_events_bin(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"BFEVSOA1"
    n = int(np.frombuffer(raw, "<u8", 1, 8)[0])
    t = np.frombuffer(raw, "<u8", n, 16).astype(np.int64)
    col = np.frombuffer(raw, "<u2", n, 16 + 8 * n).astype(np.int32)
    row = np.frombuffer(raw, "<u2", n, 16 + 10 * n).astype(np.int32)
    return t, row, col


def oracle_slices(path, stm=True):
    """The reference ring's slices of a recording that never fills or outlives the ring (DVS_flow::add_event / recompute,
    dvs_flow.h:164-231), solved by the oracle: per slice, the events in the ring's iteration order (newest -> oldest) with
    their final positions, flow, and the two scale-1 projection images."""
    import oracle
    t, row, col = read_events_bin(path)
    assert len(t) < 50000 and t[-1] < 200_000_000
    ends, last, diff = [], 0, 0
    for i in range(len(t)):
        diff += 1
        if diff >= 20000 or t[i] - last >= 33_000_000:
            ends.append(i + 1)
            last, diff = t[i], 0
    ends.append(len(t))                                   # the final recompute()
    out, last_model = [], oracle.Model()
    for e in ends:
        c = oracle.Cloud(row[:e][::-1], col[:e][::-1], t[:e][::-1])   # slice origin 0: the ring spans less than SPAN
        w = c.set_cloud(3, H, W)
        m = c.set_model(last_model) if stm else oracle.Model()
        c.run(w, m, res_x=H, res_y=W)
        last_model = m
        u, v = c.compute_uv()
        out.append({"pr_x": c.pr_x.copy(), "pr_y": c.pr_y.copy(), "u": u, "v": v,
                    "comp": c.projection_img(1, H, W, False), "raw": c.projection_img(1, H, W, True)})
    return out


def ppm_payload_of(data, rows, cols):
    head = b"P6\n%d %d\n255\n" % (cols, rows)
    assert data.startswith(head) and len(data) == len(head) + rows * cols * 3
    return np.frombuffer(data, np.uint8, rows * cols * 3, len(head)).reshape(rows, cols, 3)


@pytest.mark.parametrize("stm", [True, False])
def test_cli_flow_files_equal_restatement(oracle_cli, fixtures, tmp_path, stm):
    files = flow_run(oracle_cli, ["--engine=ring"] + ([] if stm else ["--stm-disable"]), fixtures["bin"], str(tmp_path / "ring"))
    slices = oracle_slices(fixtures["bin"], stm)
    assert len(slices) == 4 and sorted(files) == sorted(["flow_%d.%s" % (k, e) for k in range(4) for e in ("ppm", "flo")])
    for k, s in enumerate(slices):
        # the ring uploads in iteration order, which is the order the reference walks: the last uploaded event owns
        owner, U, V = ref.flow_field(s["pr_x"], s["pr_y"], s["u"], s["v"], None, H, W, ref.LAST_UPLOADED)
        assert (owner >= 0).sum() > 1000
        assert files["flow_%d.flo" % k] == ref.flo_file(owner, U, V), k
        bgr, _ = ref.color_flow(owner, U, V)
        want = ref.ppm_payload(ref.flow_frame(s["comp"], bgr, s["raw"]))
        got = ppm_payload_of(files["flow_%d.ppm" % k], H, 3 * W)
        assert np.array_equal(got, want), (k, int((got != want).any(axis=2).sum()))
        # the owner of a pixel is the OLDEST event on it: the largest index of the newest -> oldest order
        px = ref.trunc_x86(s["pr_x"]) * W + ref.trunc_x86(s["pr_y"])
        inside = (ref.trunc_x86(s["pr_x"]) >= 0) & (ref.trunc_x86(s["pr_x"]) < H) & (ref.trunc_x86(s["pr_y"]) >= 0) & (ref.trunc_x86(s["pr_y"]) < W)
        j = np.nonzero(inside)[0][-1]
        assert owner.ravel()[px[j]] == j


@pytest.mark.parametrize("inp, ring, stream", [
    ("txt", [], []),
    ("bin", [], []),
    ("txt", ["--stm-disable"], ["--stm-disable", "--contexts=3"]),
    ("guard", [], []),
    ("guard", ["--stm-disable"], ["--stm-disable", "--contexts=3"]),
])
def test_cli_stream_flow_files_equal_ring(oracle_cli, fixtures, tmp_path, inp, ring, stream):
    extra = ("--flow-img", "--flow-field", "--video")
    a = flow_run(oracle_cli, ["--engine=ring"] + ring, fixtures[inp], str(tmp_path / "ring"), extra)
    b = flow_run(oracle_cli, ["--engine=stream"] + stream, fixtures[inp], str(tmp_path / "stream"), extra)
    assert sum(f.endswith(".flo") for f in a) >= 3 and "out_flow.avi" in a and "out.avi" in a
    assert sorted(a) == sorted(b)
    assert [f for f in a if a[f] != b[f]] == []
    # the video holds the flow frames: bottom-up B G R rows
    first = ppm_payload_of(a["flow_0.ppm"], H, 3 * W)
    avi = a["out_flow.avi"]
    at = avi.index(b"movi") + 4 + 8
    frame = np.frombuffer(avi, np.uint8, H * 3 * W * 3, at).reshape(H, 3 * W, 3)
    assert np.array_equal(frame[::-1, :, ::-1], first)


def test_cli_other_outputs_unchanged(oracle_cli, fixtures, tmp_path):
    """-o and frame_N.* next to the new flags are byte-identical to a run without them -- on both engines, and each flag
    alone writes only its own files."""
    for engine in ("ring", "stream"):
        base = ["--engine=" + engine, "--img"]
        plain = flow_run(oracle_cli, base + ["-o", str(tmp_path / (engine + "_p.txt"))], fixtures["txt"], str(tmp_path / (engine + "_p")), ())
        both = flow_run(oracle_cli, base + ["-o", str(tmp_path / (engine + "_f.txt"))], fixtures["txt"], str(tmp_path / (engine + "_f")))
        assert open(str(tmp_path / (engine + "_p.txt")), "rb").read() == open(str(tmp_path / (engine + "_f.txt")), "rb").read()
        assert sorted(plain) == sorted(f for f in both if f.startswith("frame_")) and len(plain) == 8
        assert all(plain[f] == both[f] for f in plain)
        only_img = flow_run(oracle_cli, ["--engine=" + engine], fixtures["txt"], str(tmp_path / (engine + "_i")), ("--flow-img",))
        only_flo = flow_run(oracle_cli, ["--engine=" + engine], fixtures["txt"], str(tmp_path / (engine + "_o")), ("--flow-field",))
        assert sorted(only_img) == ["flow_%d.ppm" % k for k in range(4)] and sorted(only_flo) == ["flow_%d.flo" % k for k in range(4)]
        assert all(only_img[f] == both[f] for f in only_img) and all(only_flo[f] == both[f] for f in only_flo)


def test_cli_help_and_defaults(oracle_cli, fixtures, tmp_path):
    out = run_cli(oracle_cli, ["--help"], str(tmp_path))
    assert "--flow-img" in out and "--flow-field" in out
    # without --engine the new flags keep the reference ring, like --img
    r = subprocess.run([oracle_cli, "--flow-field", "--img-prefix", str(tmp_path), "--timing", "--quiet", fixtures["txt"]],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b'"engine": "stream"' not in r.stderr and os.path.exists(str(tmp_path / "flow_0.flo"))


# ---- 3. flowio ----

def test_flowio_reads_cli_field(oracle_cli, fixtures, tmp_path):
    files = flow_run(oracle_cli, ["--engine=stream"], fixtures["txt"], str(tmp_path / "s"), ("--flow-field",))
    u, v, valid = flowio.read_flo(str(tmp_path / "s" / "flow_3.flo"))
    assert u.shape == (H, W) and valid.sum() > 1000 and u.dtype == np.float32
    vr, vc = synth.default_velocity(H, W)
    assert abs(float(u[valid].mean()) - vr) < 0.05 * abs(vr) and abs(float(v[valid].mean()) - vc) < 0.05 * abs(vc)
    assert (u[~valid] == np.float32(1e9)).all() and (v[~valid] == np.float32(1e9)).all()
    back = str(tmp_path / "back.flo")
    flowio.write_flo(back, u, v, valid)
    assert open(back, "rb").read() == files["flow_3.flo"]
    assert hashlib.sha256(files["flow_3.flo"]).hexdigest() != hashlib.sha256(files["flow_0.flo"]).hexdigest()
    bad = str(tmp_path / "bad.flo")
    open(bad, "wb").write(files["flow_3.flo"][:-4])
    with pytest.raises(ValueError):
        flowio.read_flo(bad)
