"""The per-pixel flow field, EventFile::color_flow_img and the flow frame on the MI355X (bf_flow_field, bf_color_flow_img,
bf_flow_frame_*, bf_render_flow_frame; csrc/bf_flowimg.hip), against tests/flowimg_ref.py -- the numpy restatement of the rule
stated in include/bf_accel.h -- and host/better_flow/frame_writer.h's compose_flow_frame.

* bf_flow_field: the owner plane equals the restatement EXACTLY under both ownership rules (it is computed from the positions
  bf_writeout_events returns, which are bit-exact against the oracle); u / v equal bf_compute_uv's values at the owner as
  bits; reversing the upload order with the opposite rule gives the identical planes.
* bf_color_flow_img: H / S bytes and B, G, R equal the restatement applied to the device's own field.  Device atan2 / log /
  hypot may differ from the host's in the last place, which can only show where angle / 2 or log_spd lies within 1e-9
  (relative) of an integer: the inputs have no such pixel (asserted), so the comparison is exact.
* bf_render_flow_frame and the ticketed calls: the payloads equal compose_flow_frame of the three tiles' synchronous results.
* The product command line: --engine=stream writes the files --engine=ring writes."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flowimg_ref as ref  # noqa: E402
from better_flow_amd import accel, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GEOMETRIES = [(240, 180), (346, 260), (640, 480), (1280, 720), (67, 101)]
RULES = (accel.BF_FLOW_LAST_UPLOADED, accel.BF_FLOW_FIRST_UPLOADED)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_field(acc, H, W, noise, what):
    """Both rules against the restatement; returns the LAST_UPLOADED planes."""
    pr_x, pr_y, _, _ = acc.writeout_events() if acc.n else (np.zeros(0),) * 4
    u, v = acc.compute_uv() if acc.n else (np.zeros(0), np.zeros(0))
    out = None
    for rule in RULES:
        owner, U, V = acc.flow_field(H, W, rule)
        ro, rU, rV = ref.flow_field(pr_x, pr_y, u, v, noise, H, W, rule)
        assert np.array_equal(owner, ro), (what, rule, int((owner != ro).sum()))
        assert np.array_equal(bits(U), bits(rU)) and np.array_equal(bits(V), bits(rV)), (what, rule)
        # optional outputs: the owner plane alone
        o2 = np.empty((H, W), dtype=np.int32)
        acc._chk(acc.L.bf_flow_field(acc.h, H, W, rule, o2.ctypes.data_as(C.c_void_p), None, None))
        assert np.array_equal(o2, owner)
        if rule == accel.BF_FLOW_LAST_UPLOADED:
            out = (owner, U, V)
    return out


def check_colour(acc, H, W, what, moving):
    for rule in RULES:
        owner, U, V = acc.flow_field(H, W, rule)
        bgr, hs = acc.color_flow_img(H, W, rule, want_hs=True)
        live = (owner >= 0) & ((U != 0) | (V != 0))
        near = live & ref.at_risk(U, V)
        print("%s rule %d: covered %d, moving %d, within 1e-9 of an integer %d" % (what, rule, (owner >= 0).sum(), live.sum(), near.sum()))
        assert near.sum() == 0, (what, rule, int(near.sum()))       # the inputs keep clear of the boundaries
        assert (live.sum() > 0) == moving
        rb, rhs = ref.color_flow(owner, U, V)
        dh = int((hs != rhs).any(axis=2).sum())
        print("%s rule %d: H / S bytes differing %d" % (what, rule, dh))
        assert dh == 0, (what, rule, dh)
        assert np.array_equal(bgr, rb), (what, rule)
        assert np.array_equal(acc.color_flow_img(H, W, rule), bgr)  # without the H / S output
        assert (bgr[owner < 0] == 255).all()


@pytest.mark.parametrize("W, H", GEOMETRIES)
def test_flow_field_and_colour(W, H):
    sl = synth.make_slice(min(20000, 40 * W), H, W, 0.05, seed=W + H)
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n + 16, max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        acc.set_cloud(3, H, W)
        check_field(acc, H, W, None, "raw")                         # Event::reset: pr = fr, zero flow
        check_colour(acc, H, W, "raw", False)
        # a warp with divergence and rotation: (nx, ny) differ from event to event, so ownership decides the pixel's flow
        acc.project_4param_reinit(-0.013, 0.021, H / 2.0, W / 2.0, 0.00011, 0.00007)
        owner, U, V = check_field(acc, H, W, None, "warped")
        check_colour(acc, H, W, "warped", True)
        shared = np.bincount(ref.trunc_x86(acc.writeout_events()[0]).clip(0, H - 1) * W + ref.trunc_x86(acc.writeout_events()[1]).clip(0, W - 1))
        assert (shared > 1).sum() > 10                              # pixels with several events exist
        # order independence: the same events uploaded in reverse, the opposite rule
        acc.upload_events(sl["fr_x"][::-1], sl["fr_y"][::-1], sl["t"][::-1])
        acc.set_cloud(3, H, W)
        acc.project_4param_reinit(-0.013, 0.021, H / 2.0, W / 2.0, 0.00011, 0.00007)
        o2, U2, V2 = acc.flow_field(H, W, accel.BF_FLOW_FIRST_UPLOADED)
        assert np.array_equal(np.where(o2 >= 0, n - 1 - o2, -1), owner)
        assert np.array_equal(bits(U2), bits(U)) and np.array_equal(bits(V2), bits(V))
        # a converged run (re-binned events: ownership stays on the upload index)
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        acc.set_cloud(3, H, W)
        rc, _, _ = acc.run()
        assert rc == 0
        check_field(acc, H, W, None, "converged")
        check_colour(acc, H, W, "converged", True)
        # a noise mask
        noise = (np.arange(n) % 3 == 0).astype(np.uint8)
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise=noise)
        acc.set_cloud(3, H, W)
        acc.project_4param_reinit(0.02, -0.01, H / 2.0, W / 2.0, -0.00009, 0.00005)
        o3, _, _ = check_field(acc, H, W, noise, "noise")
        assert (o3[o3 >= 0] % 3 != 0).all()
        # one event, none
        acc.upload_events(sl["fr_x"][:1], sl["fr_y"][:1], sl["t"][:1])
        acc.set_cloud(3, H, W)
        o4, _, _ = check_field(acc, H, W, None, "one event")
        assert (o4 >= 0).sum() == 1 and o4[sl["fr_x"][0], sl["fr_y"][0]] == 0
        acc.upload_events(sl["fr_x"][:0], sl["fr_y"][:0], sl["t"][:0])
        o5, U5, _ = acc.flow_field(H, W)
        assert (o5 == -1).all() and (U5 == 0).all() and (acc.color_flow_img(H, W) == 255).all()
    finally:
        acc.close()


def test_flow_field_refusals():
    H, W = 180, 240
    acc = accel.Accel(device=0, max_events=1024, max_rows=H, max_cols=W)
    try:
        o = np.empty((H, W), dtype=np.int32)
        p = o.ctypes.data_as(C.c_void_p)
        assert acc.L.bf_flow_field(acc.h, H, W, 0, p, None, None) == accel.BF_ERR_STATE          # before an upload
        z = np.zeros(4, dtype=np.int32)
        acc.upload_events(z, z, z.astype(np.int64))
        assert acc.L.bf_flow_field(acc.h, H, W, 2, p, None, None) == accel.BF_ERR_ARG            # unknown rule
        assert acc.L.bf_flow_field(acc.h, H + 1, W, 0, p, None, None) == accel.BF_ERR_ARG        # beyond the capacity
        assert acc.L.bf_color_flow_img(acc.h, H, W, 0, None, None) == accel.BF_ERR_ARG
        assert acc.L.bf_flow_field(acc.h, H, W, 0, p, None, None) == accel.BF_OK
    finally:
        acc.close()


COMPOSE = r'''
#include <better_flow/frame_writer.h>
#include <cstdio>
// tiles in (gray_comp, flow_bgr, gray_raw) -> PPM payload, AVI payload
int main(int argc, char **argv) {
    const int R = atoi(argv[1]), C = atoi(argv[2]);
    const size_t g = (size_t)R * C;
    std::vector<uint8_t> in(5 * g);
    FILE *f = std::fopen(argv[3], "rb");
    if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) return 1;
    std::fclose(f);
    const bf::FrameBGR fr = bf::compose_flow_frame(in.data(), in.data() + g, in.data() + 4 * g, R, C);
    std::vector<uint8_t> ppm(fr.px.size()), avi(bf::avi_stride(fr.cols) * fr.rows);
    bf::ppm_payload(fr, ppm.data());
    bf::avi_payload(fr, avi.data());
    f = std::fopen(argv[4], "wb"); std::fwrite(ppm.data(), 1, ppm.size(), f); std::fclose(f);
    f = std::fopen(argv[5], "wb"); std::fwrite(avi.data(), 1, avi.size(), f); std::fclose(f);
    return 0;
}
'''


@pytest.fixture(scope="module")
def composer(tmp_path_factory):
    d = tmp_path_factory.mktemp("compose_flow")
    src = d / "compose.cpp"
    src.write_text(COMPOSE)
    exe = str(d / "compose")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "better_flow_amd", "host"),
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    return exe, d


def host_flow_frame(composer, acc, H, W, rule):
    """compose_flow_frame (frame_writer.h) of the three tiles the synchronous calls return, and the .flo payload of the field."""
    exe, d = composer
    tiles = [acc.projection_img(1, H, W, False), acc.color_flow_img(H, W, rule), acc.projection_img(1, H, W, True)]
    inp, ppm, avi = str(d / "tiles.bin"), str(d / "ppm.bin"), str(d / "avi.bin")
    with open(inp, "wb") as f:
        for t in tiles:
            f.write(np.ascontiguousarray(t).tobytes())
    subprocess.check_call([exe, str(H), str(W), inp, ppm, avi])
    # the numpy composition is the same bytes (tests/test_flow_frames_cpu.py holds it to the command line's files)
    fr = ref.flow_frame(*tiles)
    assert ref.ppm_payload(fr).tobytes() == open(ppm, "rb").read() and ref.avi_payload(fr).tobytes() == open(avi, "rb").read()
    return open(ppm, "rb").read(), open(avi, "rb").read(), ref.flo_payload(*acc.flow_field(H, W, rule)).tobytes()


def check_flow_frame(composer, acc, H, W, what):
    for rule in RULES:
        p, a, f = acc.render_flow_frame(H, W, rule)
        hp, ha, hf = host_flow_frame(composer, acc, H, W, rule)
        assert p.shape == (H, 3 * W, 3) and a.shape == (H, (9 * W + 3) & ~3) and f.shape == (H, W, 2)
        assert p.tobytes() == hp, (what, rule, "PPM payload differs")
        assert a.tobytes() == ha, (what, rule, "AVI payload differs")
        assert f.tobytes() == hf, (what, rule, ".flo payload differs")
    p1, a1, f1 = acc.render_flow_frame(H, W, RULES[1], avi=False, flo=False)   # one layout alone gives the same bytes
    assert a1 is None and f1 is None and p1.tobytes() == hp
    _, _, f2 = acc.render_flow_frame(H, W, RULES[1], ppm=False, avi=False)
    assert f2.tobytes() == hf


@pytest.mark.parametrize("W, H", GEOMETRIES)
def test_render_flow_frame_equals_host_composition(composer, W, H):
    sl = synth.make_slice(min(20000, 40 * W), H, W, 0.05, seed=W + H)
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n + 16, max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        acc.set_cloud(3, H, W)
        check_flow_frame(composer, acc, H, W, "cold")
        acc.run()
        check_flow_frame(composer, acc, H, W, "converged")
        noise = (np.arange(n) % 3 == 0).astype(np.uint8)
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise=noise)
        acc.set_cloud(3, H, W)
        acc.project_4param_reinit(0.02, -0.01, H / 2.0, W / 2.0, -0.00009, 0.00005)
        check_flow_frame(composer, acc, H, W, "noise")
        if (W, H) == (240, 180):
            acc.upload_events(sl["fr_x"][:0], sl["fr_y"][:0], sl["t"][:0])
            check_flow_frame(composer, acc, H, W, "no event")
    finally:
        acc.close()


def test_flow_frame_tickets():
    H, W = 180, 240
    a_sl = synth.make_slice(20000, H, W, 0.03, seed=1)
    b_sl = synth.make_slice(20000, H, W, 0.03, seed=2, velocity=(100.0, -50.0))
    acc = accel.Accel(device=0, max_events=25000, max_rows=3 * H + 3, max_cols=3 * W + 3)
    L, f = acc.L, C.c_void_p()
    rule = accel.BF_FLOW_FIRST_UPLOADED

    def render():
        t = C.c_int64(-1)
        return L.bf_flow_frame_render(acc.h, f, rule, C.byref(t)), t.value

    def wait(t):
        p, a, fl = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_float)()
        return L.bf_flow_frame_wait(acc.h, f, t, C.byref(p), C.byref(a), C.byref(fl)), p, a, fl
    try:
        layouts = accel.BF_FRAME_PPM | accel.BF_FRAME_AVI | accel.BF_FLOW_FRAME_FLO
        assert L.bf_flow_frame_create(acc.h, H, W, 2, layouts, C.byref(f)) == accel.BF_OK
        acc.upload_events(a_sl["fr_x"], a_sl["fr_y"], a_sl["t"])
        acc.set_cloud(3, H, W)
        acc.run()
        want_p, want_a, want_f = acc.render_flow_frame(H, W, rule)
        rc, t0 = render()
        assert rc == accel.BF_OK and t0 == 0
        # the next slice on the same context, before waiting: frame 0 must not change
        acc.upload_events(b_sl["fr_x"], b_sl["fr_y"], b_sl["t"])
        acc.set_cloud(3, H, W)
        acc.run()
        other_p, _, other_f = acc.render_flow_frame(H, W, rule)
        assert not np.array_equal(other_p, want_p)
        rc, p, a, fl = wait(t0)
        assert rc == accel.BF_OK
        assert C.string_at(p, want_p.size) == want_p.tobytes() and C.string_at(a, want_a.size) == want_a.tobytes()
        assert C.string_at(fl, want_f.size * 4) == want_f.tobytes()
        rc, t1 = render()
        assert rc == accel.BF_OK and t1 == 1
        rc, t = render()
        assert rc == accel.BF_ERR_CAPACITY and t == -1             # both slots taken: refused, no ticket used up
        assert L.bf_flow_frame_release(f, t0) == accel.BF_OK
        assert wait(t0)[0] == accel.BF_ERR_ARG                      # released
        assert wait(99)[0] == accel.BF_ERR_ARG                      # never issued
        assert L.bf_flow_frame_release(f, t0) == accel.BF_ERR_ARG
        rc, t2 = render()
        assert rc == accel.BF_OK and t2 == 2
        rc, p, _, fl = wait(t2)
        assert rc == accel.BF_OK and C.string_at(p, other_p.size) == other_p.tobytes() and C.string_at(fl, other_f.size * 4) == other_f.tobytes()
        rc, p, _, _ = wait(t1)
        assert rc == accel.BF_OK and C.string_at(p, other_p.size) == other_p.tobytes()
        t = C.c_int64(-1)
        assert L.bf_flow_frame_render(acc.h, f, 7, C.byref(t)) == accel.BF_ERR_ARG   # unknown rule
        # destroyed with a render in flight
        assert L.bf_flow_frame_release(f, t1) == accel.BF_OK
        assert render()[0] == accel.BF_OK
        assert L.bf_flow_frame_destroy(f) == accel.BF_OK
        f = None
    finally:
        if f:
            L.bf_flow_frame_destroy(f)
        acc.close()


# ---- the product command line ----

GPU_CLI = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")


def run_cli(args, cwd):
    r = subprocess.run([GPU_CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode(), r.stderr.decode()


def flow_files(args, inp, out_dir, extra):
    os.makedirs(out_dir)
    _, err = run_cli(args + list(extra) + ["--img-prefix", out_dir, "--video-name", os.path.join(out_dir, "out.avi"), "--quiet", inp], out_dir)
    files = {f: hashlib.sha256(open(os.path.join(out_dir, f), "rb").read()).hexdigest() for f in os.listdir(out_dir)}
    shutil.rmtree(out_dir)
    return files, err


def compare(ring, stream, inp, tmp_path, tag, extra, min_frames=3):
    import json
    a, _ = flow_files(["--engine=ring"] + ring, inp, str(tmp_path / (tag + "_r")), extra)
    b, err = flow_files(["--engine=stream", "--timing"] + stream, inp, str(tmp_path / (tag + "_s")), extra)
    # both engines pick the device entries through weak symbols: had they not resolved, both would compose on the host from
    # read-backs and still agree -- the stream engine says which path it took
    timing = json.loads([l for l in err.splitlines() if l.startswith("{")][-1])
    assert timing["flow_frames_device"] == 1 and timing["frames"] == timing["slices"] >= min_frames, timing
    assert sum(f.endswith(".flo") for f in a) >= min_frames and sum(f.startswith("flow_") and f.endswith(".ppm") for f in a) >= min_frames
    assert sorted(a) == sorted(b)
    assert [f for f in a if a[f] != b[f]] == [], tag
    return a


@pytest.fixture(scope="module")
def events(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_flow_frames")
    txt = str(d / "ev10k.txt")
    synth.write_txt(txt, synth.make_slice(10000, 180, 240, 0.1, seed=5))
    big = str(d / "ev500k.bin")
    n = synth.write_stream_bin(big, 25, 20000, 180, 240)
    assert n >= 500000
    return txt, big


def test_cli_stream_flow_files_equal_ring(events, tmp_path):
    assert os.path.exists(GPU_CLI), "build() must have produced the product CLI"
    txt, big = events
    full = ("--flow-img", "--flow-field", "--img", "--video")
    a = compare([], [], txt, tmp_path, "txt", full)
    assert "out_flow.avi" in a and "out.avi" in a and "frame_0.ppm" in a
    compare(["--stm-disable"], ["--stm-disable", "--devices=0,0", "--contexts=2"], txt, tmp_path, "farm", full)
    # 25 slices against 4 frame slots per pool: both slot pools, the one writer thread and both videos under back-pressure
    for ring, stream, tag in (([], [], "big"), (["--stm-disable"], ["--stm-disable", "--devices=0,0", "--contexts=2"], "bigfarm")):
        a = compare(ring, stream, big, tmp_path, tag, full, min_frames=20)
        assert "out_flow.avi" in a and "out.avi" in a and sum(f.startswith("frame_") and f.endswith(".ppm") for f in a) >= 20


def test_cli_flow_files_leave_flow_tables_alone(events, tmp_path):
    """-o and --outfile-bin next to the flow frames equal those of a run without frames."""
    txt, _ = events
    assert all(hasattr(C.CDLL(accel.LIB_PATH), s) for s in ("bf_flow_field", "bf_color_flow_img", "bf_flow_frame_render"))
    run_cli(["-o", str(tmp_path / "a.txt"), "--outfile-bin=" + str(tmp_path / "a.bin"), "--quiet", txt], str(tmp_path))
    compare([], ["-o", str(tmp_path / "b.txt"), "--outfile-bin=" + str(tmp_path / "b.bin")], txt, tmp_path, "tables", ("--flow-img", "--flow-field", "--img"))
    assert open(str(tmp_path / "a.txt"), "rb").read() == open(str(tmp_path / "b.txt"), "rb").read()
    assert open(str(tmp_path / "a.bin"), "rb").read() == open(str(tmp_path / "b.bin"), "rb").read()
