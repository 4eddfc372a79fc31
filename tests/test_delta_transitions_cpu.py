"""The small inputs of tests/test_gpu_delta_scatter.py really exercise every branch of the delta scatter (no GPU).

The delta-scatter kernel treats an event in one of four ways, by where its scatter pixel trunc(pr * scale + shift)
(accel_lib.h:154-158) lies before and after the warp: inside -> another pixel inside (one atomic off, one on), inside ->
outside (one off), outside -> inside (one on), unchanged (none).  Here the CPU oracle is stepped through the same runs --
iteration_step under the loop control of OptimizerRolling::run (optimizer_rolling.h:48-125), as scripts/mover_fraction.py does
it -- and every one of the four must make up at least 1 % of the event-iterations of each base input."""
import os
import sys

import numpy as np
import pytest

import delta_cases as dc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import mover_fraction as mf   # noqa: E402

NAMES = ("inside -> other pixel", "inside -> outside", "outside -> inside", "unchanged")


def shares(oracle_lib, sl, H, W, scale, warm=False, max_iter=dc.K):
    cloud = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
    w = cloud.set_cloud(scale, H, W)
    rows = []
    take = lambda it, before, after: rows.append(mf.transitions(before, after))
    if warm:   # the first run's model, overshot, as the second run's start (bf_set_model; its warp is a transition too)
        m0 = oracle_lib.Model()
        cloud.run(w, m0, max_iter=max_iter, res_x=H, res_y=W)
        cloud = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
        w = cloud.set_cloud(scale, H, W)
        before = mf.scatter_pixels(cloud, w)
        m = cloud.set_model(dc.overshoot(oracle_lib.Model, m0))
        take(0, before, mf.scatter_pixels(cloud, w))
        mf.step_run(oracle_lib, cloud, w, max_iter=max_iter, on_step=take, model=m)
    else:
        mf.step_run(oracle_lib, cloud, w, max_iter=max_iter, on_step=take)
    t = np.array(rows, np.float64)
    assert np.all(t.sum(axis=1) == cloud.n)
    return t.sum(axis=0) / t.sum(), len(rows)


@pytest.mark.parametrize("scale", dc.SCALES)
def test_every_transition_occurs_on_the_base_input(oracle_lib, scale):
    sh, iters = shares(oracle_lib, dc.small_slice(), dc.H, dc.W, scale)
    print("scale %d, %d iterations: " % (scale, iters) + ", ".join("%s %.2f %%" % (n, 100 * v) for n, v in zip(NAMES, sh)))
    assert iters >= 10
    for n, v in zip(NAMES, sh):
        assert v >= 0.01, (scale, n, v)


def test_transitions_of_the_other_inputs(oracle_lib):
    """The warm start, the capped run and the 60 x 90 slice: events move, leave and enter there too (any at all: the 1 % bar is
    the base input's)."""
    m = dc.medium_slice()
    for name, got in (("warm start", shares(oracle_lib, dc.small_slice(), dc.H, dc.W, 3, warm=True)),
                      ("max_iter 10", shares(oracle_lib, dc.small_slice(), dc.H, dc.W, 3, max_iter=10)),
                      ("60 x 90", shares(oracle_lib, m, 60, 90, 3))):
        sh, iters = got
        print("%s, %d iterations: " % (name, iters) + ", ".join("%s %.2f %%" % (n, 100 * v) for n, v in zip(NAMES, sh)))
        assert all(v > 0 for v in sh), (name, sh)
