"""The slices of tests/test_gpu_lazy_args.py, on the CPU oracle: the reference loop runs all 40 iterations on them (and all 3
of the finished-loop case), so none of that file's cases ends before the iterations it is about."""
import pytest

from test_gpu_lazy_args import K, S1, S3, lazy_slice


@pytest.mark.parametrize("key", [S3, S1], ids=["scale3", "scale1"])
def test_oracle_runs_every_iteration(oracle_lib, key):
    H, W, s, n = key
    sl = lazy_slice(key)
    o = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
    w_ = o.set_cloud(s, H, W)
    for max_iter in (K, 3):
        rc, loop, trace = o.run(w_, oracle_lib.Model(), max_iter=max_iter, res_x=H, res_y=W, trace_cap=max_iter + 2, min_events=10)
        print(key, max_iter, rc, loop.itercount, len(trace))
        assert rc == 0 and loop.itercount >= max_iter and len(trace) >= max_iter, (key, max_iter, rc, loop.itercount, len(trace))
