"""The branches of the two loop kernels that fetch their arguments late (late_args, bf_device_fns.h), at the smallest shapes
that reach them.

The scatter kernel's dense lean instantiations take the four arguments of the overflow path from the argument block inside
that path, and skip dead event slots by a test of their own; the stencil kernel takes the overflow planes' addresses inside its
dirty-box path and every argument of its tail from the argument block behind the pixel loops, and keeps its per-row flags as
bits of one word.  None of this changes an arithmetic expression, so every case must give the BYTES of the global-atomics loop
(binned = 0, fused = 0) on the same slice: return code, iteration count, every trace record, model, per-event flow, time image.

Cases (the scale-3 slice is test_gpu_variants.variant_slice's, the scale-1 slice lazy_slice's -- the uniform moving scene: on
variant_slice's scale-1 slice the margin-2 loop re-bins before any event has left its tile, overflow_events == 0 --; both have
fixed seeds, and tests/test_lazy_args_cpu.py holds the oracle to running all 40 iterations on them, so no case ends early):
  * 65x67, scale 3, 20 000 events, co_schedule = 1, debug_margin = 2, 40 cold iterations: lean 512 x 1 with the plain
    <1, 0> stencil kernel.  The margin of 2 makes events outrun their bins: overflow_events > 0 and rebins >= 2 are asserted, so
    the scatter kernel's overflow path, the stencil kernel's dirty-box path and the clearing of the planes all ran;
  * the same with co_schedule = 0 (head form);
  * 65x67, scale 1, 80 000 events, co_schedule = 1, debug_margin = 2: lean 512 x 12, the headline's scatter instantiation;
  * a finished loop: max_iter = 3 with poll_interval = 8, so that five launches of each kernel behind the third iteration take
    the `done` early exit.  The C-ABI shows the state through what it returns -- the model and the iteration count (the host's
    snapshot), the trace, the flow (the final warp reads the device's state buffer) and the time image -- and these equal the
    reference's after three iterations, in either form; the two state buffers themselves are not readable from outside.
"""
import numpy as np
import pytest

from better_flow_amd import synth
from test_gpu_variants import packed, variant_slice

K = 40
S3 = (65, 67, 3, 20000)
S1 = (65, 67, 1, 80000)


def lazy_slice(key):
    """The slice of a case: S3 -> variant_slice; S1 -> exactly 80 000 events of synth.make_slice's scene, evenly over the slice."""
    if key != S1:
        return variant_slice(key)
    H, W, s, n = key
    sl = synth.make_slice(3 * n, H, W, 0.03, seed=11)
    pick = np.linspace(0, len(sl["t"]) - 1, n).astype(np.int64)
    return dict(fr_x=sl["fr_x"][pick], fr_y=sl["fr_y"][pick], t=sl["t"][pick].astype(np.int32))


def solve(a, sl, key, max_iter, poll=None):
    H, W, s, n = key
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    a.set_cloud(s, H, W)
    o = a.default_opts()
    o.res_x, o.res_y, o.want_uv, o.trace_cap, o.max_iter, o.min_events = H, W, 1, K + 2, max_iter, 10
    if poll:
        o.poll_interval = poll
    rc, m, info = a.run(o)
    trace = a.get_trace(K + 2)
    u, v = a.compute_uv()
    timg = a.get_time_img()
    return dict(rc=rc, it=info.iterations, model=packed(m), trace=[packed(t) for t in trace], flow=(u.tobytes(), v.tobytes()),
                timg=tuple(np.ascontiguousarray(x).tobytes() for x in timg)), info


@pytest.fixture(scope="module")
def references(accel_mod):
    """Per (slice, iterations), computed once: the slice and the global-atomics loop's result on it."""
    from helpers import make_accel
    slices, cache = {}, {}

    def get(key, max_iter):
        if key not in slices:
            slices[key] = lazy_slice(key)
        if (key, max_iter) not in cache:
            H, W, s, n = key
            a = make_accel(accel_mod, dict(binned=0, fused=0), max_events=n, max_rows=s * H + s, max_cols=s * W + s)
            try:
                ref, _ = solve(a, slices[key], key, max_iter)
                assert a.get_stat("k1_threads") == -1 and a.get_stat("bins") == 0
            finally:
                a.close()
            # (the loop ran to its cap: nothing converged or gave up before the iterations the cases are about)
            assert ref["rc"] == 0 and ref["it"] >= max_iter and len(ref["trace"]) >= max_iter, (key, ref["rc"], ref["it"])
            cache[(key, max_iter)] = ref
        return slices[key], cache[(key, max_iter)]
    return get


def same_bytes(name, got, ref):
    for field in ("rc", "it", "model", "flow", "timg"):
        assert got[field] == ref[field], (name, field)
    assert len(got["trace"]) == len(ref["trace"]), (name, len(got["trace"]), len(ref["trace"]))
    for k, (g_, r_) in enumerate(zip(got["trace"], ref["trace"])):
        assert g_ == r_, (name, "trace record", k)


def run_binned(accel_mod, sl, key, opts, max_iter, poll=None):
    from helpers import make_accel
    H, W, s, n = key
    a = make_accel(accel_mod, dict(binned=2, fused=0, bin_compact=0, bin_split=0, **opts), max_events=n, max_rows=s * H + s,
                   max_cols=s * W + s)
    try:
        got, info = solve(a, sl, key, max_iter, poll)
        stat = {k: a.get_stat(k) for k in ("scatter_format", "k1_head", "k1_threads", "k1_events_per_thread", "k3_half_scale",
                                           "k3_mode", "k3_capped", "bin_margin", "bins")}
    finally:
        a.close()
    return got, info, stat


@pytest.mark.gpu
@pytest.mark.parametrize("name,key,co,k1,k3", [
    ("scale3-lean", S3, 1, (0, 512, 1, 0), (1, 0, 0)),
    ("scale3-head", S3, 0, (1, 512, 1, 0), (1, 0, 0)),
    ("scale1-lean12", S1, 1, (0, 512, 12, 0), (0, 0, 0)),
])
def test_overflow_and_dirty_box_paths_same_bits(accel_mod, references, name, key, co, k1, k3):
    sl, ref = references(key, K)
    got, info, stat = run_binned(accel_mod, sl, key, dict(co_schedule=co, debug_margin=2), K)
    print("%s: ran %s, iterations %d, overflow_events %d, rebins %d" % (name, stat, info.iterations, info.overflow_events,
                                                                        info.rebins))
    assert (stat["k1_head"], stat["k1_threads"], stat["k1_events_per_thread"], stat["scatter_format"]) == k1, stat
    assert (stat["k3_half_scale"], stat["k3_mode"], stat["k3_capped"]) == k3, stat
    assert stat["bin_margin"] == 2, stat
    assert info.overflow_events > 0 and info.rebins >= 2, (info.overflow_events, info.rebins)
    same_bytes(name, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("co", [1, 0], ids=["lean", "head"])
def test_finished_loop_keeps_the_state(accel_mod, references, co):
    sl, ref = references(S3, 3)
    got, info, stat = run_binned(accel_mod, sl, S3, dict(co_schedule=co), 3, poll=8)
    print("finished-%s: ran %s, iterations %d" % ("lean" if co else "head", stat, info.iterations))
    assert stat["k1_head"] == 1 - co and stat["k3_mode"] == 0, stat
    same_bytes("finished", got, ref)
