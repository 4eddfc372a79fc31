"""--img / --video frames composed on the device (bf_frame_*, bf_render_frame; csrc/bf_frame.hip) on the MI355X.

* The C-ABI against frame_writer.h: bf_render_frame's PPM and AVI payloads equal, byte for byte, frame_writer.h's composition
  (compose_frame, ppm_payload, avi_payload -- compiled here from the header) of the four tiles bf_projection_img and
  bf_color_time_img return, on five geometries, cold and converged slices, noise flags, empty and one-event slices.
* Tickets: a frame sees the slice it was rendered from; full slots refuse without enqueueing; released / unknown tickets are
  errors; destroying with renders in flight is clean.
* The product command line: --engine=stream --img --video writes the files --engine=ring writes."""
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
from better_flow_amd import accel, synth  # noqa: E402

pytestmark = pytest.mark.gpu

COMPOSE = r'''
#include <better_flow/frame_writer.h>
#include <cstdio>
// tiles in (gray_comp, colour_comp, gray_raw, colour_raw) -> PPM payload, AVI payload
int main(int argc, char **argv) {
    const int R = atoi(argv[1]), C = atoi(argv[2]);
    const size_t g = (size_t)R * C, c = (size_t)(R + 3) * (C + 3) * 3;
    std::vector<uint8_t> in(2 * g + 2 * c);
    FILE *f = std::fopen(argv[3], "rb");
    if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) return 1;
    std::fclose(f);
    const bf::FrameBGR fr = bf::compose_frame(in.data(), in.data() + g, in.data() + g + c, in.data() + 2 * g + c, R, C);
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
    d = tmp_path_factory.mktemp("compose")
    src = d / "compose.cpp"
    src.write_text(COMPOSE)
    exe = str(d / "compose")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I" + os.path.join(ROOT, "better_flow_amd", "host"), str(src), "-o", exe])
    return exe, d


def host_frame(composer, acc, H, W):
    """frame_writer.h's composition of the four tiles the synchronous renderers return."""
    exe, d = composer
    tiles = [acc.projection_img(3, H, W, True), acc.color_time_img(3, H, W, True),
             acc.projection_img(3, H, W, False), acc.color_time_img(3, H, W, False)]
    inp, ppm, avi = str(d / "tiles.bin"), str(d / "ppm.bin"), str(d / "avi.bin")
    with open(inp, "wb") as f:
        for t in tiles:
            f.write(np.ascontiguousarray(t).tobytes())
    subprocess.check_call([exe, str(3 * H), str(3 * W), inp, ppm, avi])
    return open(ppm, "rb").read(), open(avi, "rb").read()


def check_frame(composer, acc, H, W, what):
    p, a = acc.render_frame(H, W)
    hp, ha = host_frame(composer, acc, H, W)
    assert p.shape == (6 * H, 6 * W, 3) and a.shape == (6 * H, (18 * W + 3) & ~3)
    assert p.tobytes() == hp, (what, "PPM payload differs")
    assert a.tobytes() == ha, (what, "AVI payload differs")
    # either layout alone gives the same bytes
    p1, a1 = acc.render_frame(H, W, avi=False)
    assert a1 is None and p1.tobytes() == hp
    return p


@pytest.mark.parametrize("W, H", [(240, 180), (346, 260), (640, 480), (1280, 720), (67, 101)])
def test_render_frame_equals_host_composition(composer, W, H):
    sl = synth.make_slice(min(20000, 40 * W), H, W, 0.05, seed=W + H)
    n = len(sl["t"])
    acc = accel.Accel(device=0, max_events=n + 16, max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        acc.set_cloud(3, H, W)
        cold = check_frame(composer, acc, H, W, "cold")
        acc.run()
        warm = check_frame(composer, acc, H, W, "converged")
        assert not np.array_equal(cold, warm)            # the compensated tiles moved
        noise = (np.arange(n) % 3 == 0).astype(np.uint8)  # a third of the events flagged
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise=noise)
        acc.set_cloud(3, H, W)
        check_frame(composer, acc, H, W, "noise")
        if (W, H) == (240, 180):
            acc.upload_events(sl["fr_x"][:1], sl["fr_y"][:1], sl["t"][:1])
            check_frame(composer, acc, H, W, "one event")
            acc.upload_events(sl["fr_x"][:0], sl["fr_y"][:0], sl["t"][:0])
            check_frame(composer, acc, H, W, "no event")
    finally:
        acc.close()


def _frame_calls(acc):
    L = acc.L
    f = C.c_void_p()

    def render():
        t = C.c_int64(-1)
        rc = L.bf_frame_render(acc.h, f, C.byref(t))
        return rc, t.value

    def wait(t):
        p, a = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
        rc = L.bf_frame_wait(acc.h, f, t, C.byref(p), C.byref(a))
        return rc, p, a
    return L, f, render, wait


def test_frame_tickets():
    H, W = 180, 240
    a_sl = synth.make_slice(20000, H, W, 0.03, seed=1)
    b_sl = synth.make_slice(20000, H, W, 0.03, seed=2, velocity=(100.0, -50.0))
    acc = accel.Accel(device=0, max_events=25000, max_rows=3 * H + 3, max_cols=3 * W + 3)
    L, f, render, wait = _frame_calls(acc)
    try:
        assert L.bf_frame_create(acc.h, H, W, 2, accel.BF_FRAME_PPM | accel.BF_FRAME_AVI, C.byref(f)) == accel.BF_OK
        nbytes = 36 * H * W * 3
        acc.upload_events(a_sl["fr_x"], a_sl["fr_y"], a_sl["t"])
        acc.set_cloud(3, H, W)
        acc.run()
        want_p, want_a = acc.render_frame(H, W)
        rc, t0 = render()
        assert rc == accel.BF_OK and t0 == 0
        # the next slice on the same context, before waiting: frame 0 must not change
        acc.upload_events(b_sl["fr_x"], b_sl["fr_y"], b_sl["t"])
        acc.set_cloud(3, H, W)
        acc.run()
        other_p, _ = acc.render_frame(H, W)
        assert not np.array_equal(other_p, want_p)
        rc, p, a = wait(t0)
        assert rc == accel.BF_OK
        assert C.string_at(p, nbytes) == want_p.tobytes() and C.string_at(a, want_a.size) == want_a.tobytes()
        rc, t1 = render()
        assert rc == accel.BF_OK and t1 == 1
        # both slots taken: refused, nothing enqueued (no ticket used up)
        rc, t = render()
        assert rc == accel.BF_ERR_CAPACITY and t == -1
        assert L.bf_frame_release(f, t0) == accel.BF_OK
        rc, p, _ = wait(t0)
        assert rc == accel.BF_ERR_ARG                     # released
        rc, _, _ = wait(99)
        assert rc == accel.BF_ERR_ARG                     # never issued
        assert L.bf_frame_release(f, t0) == accel.BF_ERR_ARG
        rc, t2 = render()
        assert rc == accel.BF_OK and t2 == 2
        rc, p, _ = wait(t2)
        assert rc == accel.BF_OK and C.string_at(p, nbytes) == other_p.tobytes()
        rc, p, _ = wait(t1)
        assert rc == accel.BF_OK and C.string_at(p, nbytes) == other_p.tobytes()
        # destroyed with a render in flight
        assert L.bf_frame_release(f, t1) == accel.BF_OK
        rc, _ = render()
        assert rc == accel.BF_OK
        assert L.bf_frame_destroy(f) == accel.BF_OK
        f = None
        # a context without the image capacity of the scale-3 colour tile is refused
        g = C.c_void_p()
        small = accel.Accel(device=0, max_events=25000, max_rows=3 * H, max_cols=3 * W)
        try:
            small.upload_events(a_sl["fr_x"], a_sl["fr_y"], a_sl["t"])
            assert L.bf_frame_create(small.h, H, W, 1, accel.BF_FRAME_PPM, C.byref(g)) == accel.BF_OK
            t = C.c_int64(-1)
            assert L.bf_frame_render(small.h, g, C.byref(t)) == accel.BF_ERR_CAPACITY
            assert L.bf_frame_destroy(g) == accel.BF_OK
        finally:
            small.close()
    finally:
        if f:
            L.bf_frame_destroy(f)
        acc.close()


# ---- the product command line ----

GPU_CLI = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")


def run_cli(args, cwd):
    r = subprocess.run([GPU_CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode()


def frame_files(args, inp, out_dir, video=True):
    os.makedirs(out_dir)
    extra = ["--img", "--img-prefix", out_dir] + (["--video", "--video-name", os.path.join(out_dir, "out.avi")] if video else [])
    run_cli(args + extra + ["--quiet", inp], out_dir)
    files = {f: hashlib.sha256(open(os.path.join(out_dir, f), "rb").read()).hexdigest() for f in os.listdir(out_dir)}
    shutil.rmtree(out_dir)
    return files


def compare(ring, stream, inp, tmp_path, tag, video=True, min_frames=3):
    a = frame_files(["--engine=ring"] + ring, inp, str(tmp_path / (tag + "_r")), video)
    b = frame_files(["--engine=stream"] + stream, inp, str(tmp_path / (tag + "_s")), video)
    assert sum(f.endswith(".ppm") for f in a) >= min_frames and ("out.avi" in a) == video
    assert sorted(a) == sorted(b)
    assert [f for f in a if a[f] != b[f]] == [], tag


@pytest.fixture(scope="module")
def events(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_frames")
    txt = str(d / "ev10k.txt")
    synth.write_txt(txt, synth.make_slice(10000, 180, 240, 0.1, seed=5))
    big = str(d / "ev500k.bin")
    n = synth.write_stream_bin(big, 25, 20000, 180, 240)
    assert n > 450000
    return txt, big


def test_cli_stream_frames_equal_ring(events, tmp_path):
    assert os.path.exists(GPU_CLI), "build() must have produced the product CLI"
    txt, big = events
    compare([], [], txt, tmp_path, "txt")
    compare(["--stm-disable"], ["--stm-disable", "--devices=0,0", "--contexts=2"], txt, tmp_path, "farm")
    compare([], [], big, tmp_path, "big", video=False, min_frames=20)


def test_cli_stream_frames_with_flow_files(events, tmp_path):
    """-o and --outfile-bin next to the frames: the flow files equal those of a run without frames."""
    txt, _ = events
    run_cli(["-o", str(tmp_path / "a.txt"), "--outfile-bin=" + str(tmp_path / "a.bin"), "--quiet", txt], str(tmp_path))
    compare([], ["-o", str(tmp_path / "b.txt"), "--outfile-bin=" + str(tmp_path / "b.bin")], txt, tmp_path, "flow")
    assert open(str(tmp_path / "a.txt"), "rb").read() == open(str(tmp_path / "b.txt"), "rb").read()
    assert open(str(tmp_path / "a.bin"), "rb").read() == open(str(tmp_path / "b.bin"), "rb").read()
