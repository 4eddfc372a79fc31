"""The -o table accumulated on the device (bf_emit_slice, StreamEngine::set_accumulate_device) and the binary flow file
(bf_motion_compensator --outfile-bin, better_flow_amd/flowio.py).

CPU: the binary writer against the Python reader, the CLI's option handling, and the two numpy restatements of the marking
rule (tests/emit_ref.py: the host's chain walk and the device's covered plane + sorted runs + tail) against each other and
against StreamEngine::get_accumulated on the CPU stand-in of the C-ABI.  GPU: the device table against the host table,
element for element, u / v as bits; the CLI's text and binary outputs; the C-ABI entry's edge cases."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from better_flow_amd import flowio, synth  # noqa: E402
import emit_ref  # noqa: E402

HOST = os.path.join(ROOT, "better_flow_amd", "host")
INC = os.path.join(ROOT, "include")
CLI = os.path.join(HOST, "bf_motion_compensator")
GPU_TIMEOUT = 600


def _gxx(src, exe, gpu):
    base = ["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + HOST, "-I" + INC, src]
    if gpu:
        lib = os.path.join(ROOT, "better_flow_amd")
        subprocess.check_call(base + ["-L" + lib, "-lbf_accel", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    else:
        obj = exe + ".oracle.o"
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "bf_oracle.c"), "-o", obj])
        subprocess.check_call(base + [os.path.join(ROOT, "tests", "shim", "bf_accel_oracle_shim.cpp"), obj, "-lm", "-o", exe])
    return exe


def write_events_bin(path, t_ns, row, col):
    """BFEVSOA1 (event_reader.h): u64 t, u16 x = column, u16 y = row, u8 p."""
    t_ns = np.asarray(t_ns, dtype="<u8")
    with open(path, "wb") as f:
        f.write(b"BFEVSOA1")
        f.write(np.uint64(len(t_ns)).astype("<u8").tobytes())
        f.write(t_ns.tobytes())
        f.write(np.asarray(col).astype("<u2").tobytes())
        f.write(np.asarray(row).astype("<u2").tobytes())
        f.write(np.ones(len(t_ns), dtype=np.uint8).tobytes())


def clause_stream(n_blocks, seed, pixels=6, base=1_000_000_000):
    """Events on a few pixels (rows 3.., columns 5..) built from blocks that hit every clause of the marking rule: pairs at
    one pixel 99 999 ns and 100 000 ns apart, twins and triplets at one instant, and filler on the other pixels; sorted
    by time (stable).  Returns (t, row, col)."""
    rng = np.random.default_rng(seed)
    ev = []
    t = base
    for _ in range(n_blocks):
        p = int(rng.integers(pixels))
        kind = int(rng.integers(5))
        if kind == 0:
            ev += [(t, p), (t + 99999, p)]
        elif kind == 1:
            ev += [(t, p), (t + 100000, p)]
        elif kind == 2:
            ev += [(t, p)] * int(rng.integers(2, 4))
        elif kind == 3:
            ev += [(t + int(rng.integers(0, 150000)), int(rng.integers(pixels))) for _ in range(3)]
        else:
            ev += [(t, p), (t + 1, p), (t + 100001, p)]
        t += int(rng.choice([0, 1, 20000, 60000, 99999, 100000]))
    ev.sort(key=lambda e: e[0])
    tt = np.array([e[0] for e in ev], dtype=np.uint64)
    pp = np.array([e[1] for e in ev])
    return tt, 3 + pp // 3, 5 + pp % 3


# ---------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_flow_bin_writer_reader_round_trip(tmp_path, n):
    exe = _gxx(os.path.join(ROOT, "tests", "cpp", "test_flow_bin.cpp"), str(tmp_path / "test_flow_bin"), gpu=False)
    path = str(tmp_path / "f.bin")
    subprocess.check_call([exe, path, str(n)])
    assert os.path.getsize(path) == 16 + 28 * n
    got = flowio.read_flow_bin(path)
    i = np.arange(n, dtype=np.float64)
    k = np.arange(n, dtype=np.uint64)
    assert got["t"].dtype == np.uint64 and np.array_equal(got["t"], 1000000000 + 37 * k)
    assert got["row"].dtype == np.uint16 and np.array_equal(got["row"], (k % 65536).astype(np.uint16))
    assert np.array_equal(got["col"], ((7 * k) % 65536).astype(np.uint16))
    assert np.array_equal(got["u"].view(np.uint64), (i / 3 - 5.5).view(np.uint64))
    assert np.array_equal(got["v"].view(np.uint64), (-(i * 0.25) + 1e-300).view(np.uint64))
    # and the Python writer gives the same bytes
    again = str(tmp_path / "g.bin")
    flowio.write_flow_bin(again, got["t"], got["row"], got["col"], got["u"], got["v"])
    assert open(again, "rb").read() == open(path, "rb").read()


def test_read_flow_bin_rejects_other_files(tmp_path):
    p = str(tmp_path / "x.bin")
    flowio.write_flow_bin(p, [1, 2], [3, 4], [5, 6], [0.5, 1.5], [2.5, 3.5])
    data = open(p, "rb").read()
    open(p, "wb").write(data[:-1])
    with pytest.raises(ValueError):
        flowio.read_flow_bin(p)
    open(p, "wb").write(b"BFEVSOA1" + data[8:])
    with pytest.raises(ValueError):
        flowio.read_flow_bin(p)


@pytest.fixture(scope="module")
def oracle_cli():
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import build as shim_build
    return shim_build.build()


@pytest.fixture(scope="module")
def small_txt(tmp_path_factory):
    d = tmp_path_factory.mktemp("flowcli")
    path = str(d / "ev.txt")
    synth.write_txt(path, synth.make_slice(3000, 180, 240, 0.05, seed=2))
    return path


def _cli_rc(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stderr.decode()


def test_cli_outfile_bin_refused_on_reference_ring(oracle_cli, small_txt, tmp_path):
    rc, err = _cli_rc(oracle_cli, [small_txt, "--engine=ring", "--outfile-bin=" + str(tmp_path / "f.bin"), "--quiet"], str(tmp_path))
    assert rc == 1 and "--outfile-bin belongs to the stream engine" in err
    assert not (tmp_path / "f.bin").exists()
    rc, err = _cli_rc(oracle_cli, [small_txt, "--img", "--outfile-bin=" + str(tmp_path / "f.bin"), "--quiet"], str(tmp_path))
    assert rc == 1 and not (tmp_path / "f.bin").exists()


def test_cli_outfile_bin_needs_a_file_name(oracle_cli, small_txt, tmp_path):
    rc, err = _cli_rc(oracle_cli, [small_txt, "--outfile-bin=", "--quiet"], str(tmp_path))
    assert rc == 1 and "--outfile-bin needs a file name" in err
    rc, err = _cli_rc(oracle_cli, [small_txt, "--outfile-bin", "--quiet"], str(tmp_path))
    assert rc == 1 and "unknown flag" in err


def test_cli_help_lists_outfile_bin(oracle_cli, tmp_path):
    r = subprocess.run([oracle_cli, "--help"], stdout=subprocess.PIPE, timeout=60)
    assert b"--outfile-bin=<file>" in r.stdout and b"BFFLSOA1" in r.stdout


def test_outfile_bin_without_device_table_fails_cleanly(oracle_cli, small_txt, tmp_path):
    """The CPU stand-in has no bf_emit_*: the stream engine says so instead of writing a wrong table."""
    rc, err = _cli_rc(oracle_cli, [small_txt, "--outfile-bin=" + str(tmp_path / "f.bin"), "--quiet"], str(tmp_path))
    assert rc != 0 and "bf_emit_create" in err, err
    assert not (tmp_path / "f.bin").exists()


def _random_slices(N, seed, max_sz):
    """A slice sequence the way the stream engine makes them: triggers at growing arrival numbers, a ring of max_sz (a full
    ring leaves its oldest element out and may lead with it), repeated triggers without new events (fully overlapping
    slices), an empty slice at the start; start_time sometimes one past the oldest timestamp (the t == -1 mark)."""
    rng = np.random.default_rng(seed)
    out, end, seen = [(0, 0, 0, 0)], 0, 0
    while end < N:
        end = min(N, end + int(rng.integers(0, 2 * max_sz)))
        if end == 0:
            continue
        size = min(end, max_sz)
        oldest = end - size
        full = size == max_sz
        first, n = (oldest + 1, size - 1) if full else (oldest, size)
        lead = int(full and oldest >= seen)
        out.append((first, n, first, lead))
        seen = end
    return out


@pytest.mark.parametrize("seed", range(6))
def test_marking_rule_pull_form_equals_push_form(seed):
    t, row, col = clause_stream(300, seed)
    pix = row * 1000 + col
    slices = _random_slices(len(t), seed, max_sz=12 + 5 * seed)
    # the t == -1 mark: some slices start one past their oldest timestamp
    slices = [(f, n, (int(t[f]) + 1 if (n and k % 3 == 1) else (int(t[f]) if n else 0)), ld) for k, (f, n, _, ld) in enumerate(slices)]
    host = emit_ref.host_rows(t, pix, slices)
    dev = emit_ref.device_rows(t, pix, slices, cap=4 * (12 + 5 * seed) + 7)
    assert dev == host
    assert len(host) > 0 and any(s[3] for s in slices)


@pytest.mark.parametrize("max_sz,on_ev", [(16, 24), (16, 5), (40, 1), (64, 64)])
def test_marking_rule_restatements_equal_stream_engine_host_walk(tmp_path, max_sz, on_ev):
    """Both restatements against StreamEngine::get_accumulated on slices cut by the engine itself (CPU stand-in): a full ring
    with a lead every slice (16, 24), overlapping slices (16, 5), fully overlapping ones (40, 1: a slice per event)."""
    exe = _gxx(os.path.join(ROOT, "tests", "cpp", "test_accumulate_dump.cpp"), str(tmp_path / "dump"), gpu=False)
    t, row, col = clause_stream(200, max_sz + on_ev)
    path = str(tmp_path / "ev.bin")
    write_events_bin(path, t, row, col)
    out = subprocess.check_output([exe, path, str(max_sz), "100000000", str(on_ev), "1000000000"], timeout=300).decode().split("\n")
    slices = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("S ")]
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.startswith("R ")]
    t = t - t[0]   # (the reader makes the timestamps relative to the first event's)
    host = emit_ref.host_rows(t, row * 1000 + col, slices)
    dev = emit_ref.device_rows(t, row * 1000 + col, slices, cap=3 * max_sz + 5)
    assert dev == host
    assert [(int(t[g]), int(row[g]), int(col[g])) for g in host] == rows
    if on_ev > max_sz:
        assert sum(s[3] for s in slices) > 0
    assert len(rows) > 0


# ---------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def emit_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("emit")
    return _gxx(os.path.join(ROOT, "tests", "cpp", "test_emit.cpp"), str(d / "test_emit"), gpu=True)


def _warm_stream(path, H, W, n, seed, twins=97):
    sl = synth.make_slice(n, H, W, 0.2, seed=seed)
    t = sl["t"].astype(np.uint64) + np.uint64(1_000_000_000)
    row, col = sl["fr_x"], sl["fr_y"]
    k = np.arange(len(t))
    dup = k[k % twins == 0]   # twins: same pixel, same instant
    t = np.concatenate([t, t[dup]]); row = np.concatenate([row, row[dup]]); col = np.concatenate([col, col[dup]])
    o = np.argsort(t, kind="stable")
    write_events_bin(path, t[o], row[o], col[o])


def _run_emit(exe, path, max_sz, span_ns, on_ev, on_time, stm_off, contexts, H, W):
    r = subprocess.run([exe, path, str(max_sz), str(span_ns), str(on_ev), str(on_time), str(int(stm_off)), str(contexts), str(H), str(W)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=GPU_TIMEOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:] + r.stderr.decode()[-2000:]
    kv = dict(x.split("=") for x in out.strip().splitlines()[-1].split())
    return {k: int(v) for k, v in kv.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,stm_off,contexts", [(260, 346, False, 1), (480, 640, False, 1), (260, 346, True, 1), (260, 346, True, 2)],
                         ids=["warm_346x260", "warm_640x480", "stm_disable", "contexts2"])
def test_device_table_equals_host_table(emit_exe, tmp_path, H, W, stm_off, contexts):
    path = str(tmp_path / "ev.bin")
    _warm_stream(path, H, W, 300000, seed=11)
    s = _run_emit(emit_exe, path, 100000, 200_000_000, 25000, 1_000_000_000, stm_off, contexts, H, W)
    assert s["diff"] == 0 and s["rows"] == s["device_rows"] > 0
    assert s["slices"] >= 10 and s["slices"] > s["skipped"]


@pytest.mark.gpu
@pytest.mark.parametrize("max_sz,on_ev,stm_off,contexts", [(16, 24, False, 1), (16, 5, False, 1), (40, 1, False, 1), (16, 24, True, 2)],
                         ids=["lead_every_slice", "overlapping", "fully_overlapping", "lead_contexts2"])
def test_device_table_equals_host_table_clause_streams(emit_exe, tmp_path, max_sz, on_ev, stm_off, contexts):
    """The hand-built clause streams (0.1 ms boundary at 99 999 / 100 000 ns, same-instant twins and triplets) through the ring:
    every slice is under the optimizer's 1000-event minimum, so every slice is a skipped one."""
    t, row, col = clause_stream(400, 7 + max_sz + on_ev)
    path = str(tmp_path / "ev.bin")
    write_events_bin(path, t, row, col)
    s = _run_emit(emit_exe, path, max_sz, 100_000_000, on_ev, 1_000_000_000, stm_off, contexts, 260, 346)
    assert s["diff"] == 0 and s["rows"] == s["device_rows"] > 0
    assert s["skipped"] == s["slices"] > 20


@pytest.mark.gpu
def test_cli_text_and_binary_from_the_device_table(tmp_path):
    sl = synth.make_slice(120000, 180, 240, 0.1, seed=4)
    path = str(tmp_path / "ev.bin")
    synth.write_bin(path, sl)
    common = [path, "--max-events=20000", "--quiet"]

    def cli(extra):
        r = subprocess.run([CLI] + common + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=GPU_TIMEOUT)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stderr.decode()

    cli(["-o", "alone.txt"])
    err = cli(["-o", "both.txt", "--outfile-bin=flow.bin", "--timing"])
    timing = json.loads([ln for ln in err.splitlines() if ln.startswith("{")][-1])
    assert timing["output_bin_s"] > 0
    alone = open(tmp_path / "alone.txt", "rb").read()
    assert open(tmp_path / "both.txt", "rb").read() == alone
    f = flowio.read_flow_bin(str(tmp_path / "flow.bin"))
    lines = alone.decode().splitlines()
    assert len(lines) == len(f["t"]) > 100000

    def fixed9(x):   # what format_fixed9 prints (test_host_cli.py: test_fixed9_formatter_matches_printf)
        return "%.9f" % x

    text = ["%s %d %d 1 %s %s" % (fixed9(float(t) / 1000000000), c, r, fixed9(v), fixed9(u))
            for t, r, c, u, v in zip(f["t"].tolist(), f["row"].tolist(), f["col"].tolist(), f["u"].tolist(), f["v"].tolist())]
    assert text == lines


def _emit(lib, ctx, st, n, first, start, lead=0, lead_t=0, lead_row=0, lead_col=0):
    """Enqueue one slice and wait for it: (rc of the enqueue, rows as five column arrays or None)."""
    ticket = C.c_int64(-2)
    rc = lib.bf_emit_slice(ctx, st, n, first, start, lead, lead_t, lead_row, lead_col, C.byref(ticket))
    if rc != 0 or ticket.value < 0:
        return rc, ticket.value, None
    first_row, rows = C.c_uint64(), C.c_int64()
    assert lib.bf_emit_wait(ctx, st, ticket.value, C.byref(first_row), C.byref(rows)) == 0
    cols = [C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint16)(), C.POINTER(C.c_uint16)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()]
    R = C.c_int64()
    assert lib.bf_emit_output(st, *[C.byref(x) for x in cols], C.byref(R)) == 0
    idx = (first_row.value + np.arange(rows.value, dtype=np.uint64)) % np.uint64(R.value)
    out = [np.ctypeslib.as_array(x, shape=(R.value,))[idx].copy() for x in cols]
    assert lib.bf_emit_release(st, first_row.value + rows.value) == 0
    return rc, ticket.value, out


@pytest.mark.gpu
def test_emit_abi_edge_cases():
    from better_flow_amd import accel
    lib = accel.load()   # (the argument types of bf_emit_* come with the library)
    H, W = 180, 240
    sl = synth.make_slice(5000, H, W, 0.01, seed=9)
    # one event at slice-local t == -1 (the reference's mark) and twins
    fr_x = np.concatenate([[10], sl["fr_x"], sl["fr_x"][:50]]).astype(np.int32)
    fr_y = np.concatenate([[20], sl["fr_y"], sl["fr_y"][:50]]).astype(np.int32)
    t_loc = np.concatenate([[-1], sl["t"], sl["t"][:50]]).astype(np.int32)
    o = np.argsort(t_loc, kind="stable")
    fr_x, fr_y, t_loc = fr_x[o], fr_y[o], t_loc[o]
    n = len(t_loc)
    acc = accel.Accel(device=0, max_events=n, max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        ctx = acc.h
        st, small = C.c_void_p(), C.c_void_p()
        assert lib.bf_emit_create(ctx, 4 * n, H, W, 2 * n + 1, C.byref(st)) == 0
        assert lib.bf_emit_create(ctx, 4 * n, H, W, n - 1, C.byref(small)) == 0
        try:
            # an empty slice: nothing to enqueue; with a lead: the lead alone, zero flow
            rc, ticket, rows = _emit(lib, ctx, st, 0, 0, 0)
            assert rc == 0 and ticket == -1 and rows is None
            rc, ticket, rows = _emit(lib, ctx, st, 0, 5, 0, lead=1, lead_t=123, lead_row=4, lead_col=6)
            assert rc == 0 and ticket == 0 and len(rows[0]) == 1
            assert rows[0][0] == 123 and rows[1][0] == 4 and rows[2][0] == 6 and rows[3][0] == 0.0 and rows[4][0] == 0.0
            assert lib.bf_emit_reset(ctx, st) == 0

            acc.upload_events(fr_x, fr_y, t_loc)
            acc.set_cloud(3, H, W)
            acc.run()
            u_ref, v_ref = acc.compute_uv()
            start = 1_000_000
            # an output ring that cannot hold the slice's rows: BF_ERR_CAPACITY, nothing enqueued, the state unchanged
            rc, ticket, _ = _emit(lib, ctx, small, n, 0, start)
            assert rc == -6 and ticket == -1
            # the slice: every event but the t == -1 one (twins of the SAME slice both stay: marks act on later slices only)
            rc, ticket, rows = _emit(lib, ctx, st, n, 0, start)
            assert rc == 0 and ticket == 0 and len(rows[0]) == n - 1
            keep = t_loc != -1
            assert np.array_equal(rows[0], (start + t_loc[keep].astype(np.int64)).astype(np.uint64))
            assert np.array_equal(rows[1], fr_x[keep].astype(np.uint16)) and np.array_equal(rows[2], fr_y[keep].astype(np.uint16))
            assert np.array_equal(rows[3].view(np.uint64), np.asarray(u_ref)[keep].view(np.uint64))
            assert np.array_equal(rows[4].view(np.uint64), np.asarray(v_ref)[keep].view(np.uint64))
            # the same slice again: every event is covered now (the marked one never emits)
            rc, ticket, rows2 = _emit(lib, ctx, st, n, 0, start)
            assert rc == 0 and len(rows2[0]) == 0
            # a reset between streams: the first emission again, bit for bit
            assert lib.bf_emit_reset(ctx, st) == 0
            rc, ticket, rows3 = _emit(lib, ctx, st, n, 0, start)
            assert rc == 0 and ticket == 0
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(rows, rows3))
            # a slice that is not the context's, a ticket out of order: refused
            t = C.c_int64()
            assert lib.bf_emit_slice(ctx, st, n - 1, 0, start, 0, 0, 0, 0, C.byref(t)) == -3
            fr, nr = C.c_uint64(), C.c_int64()
            assert lib.bf_emit_wait(ctx, st, 5, C.byref(fr), C.byref(nr)) == -1
        finally:
            lib.bf_emit_destroy(st)
            lib.bf_emit_destroy(small)
    finally:
        acc.close()
