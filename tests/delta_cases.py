"""The small slices of the delta-scatter tests (tests/test_gpu_delta_scatter.py, tests/test_delta_transitions_cpu.py).

A 33 x 65 sensor, about 20 000 events over 0.3 s of a slowly moving scene: ten times the usual slice length makes the time
image's gradients -- and with them the optimizer's first steps -- ten times as large, so the model overshoots and swings back
several times before the dividers have grown, and with every swing a band of events leaves the window and comes back."""
from better_flow_amd import synth

H, W = 33, 65
SCALES = (3, 1)
K = 40   # iterations traced


def small_slice():
    return synth.make_slice(20000, H, W, 0.3, seed=7, velocity=(-20.0 / 3.0, 50.0 / 3.0))


def medium_slice():
    """60 x 90, 50 000 events: the slice the tile-binned default is compared on."""
    return synth.make_slice(50000, 60, 90, 0.3, seed=11, velocity=(-10.0, 25.0))


def overshoot(model_cls, m):
    """A warm start that has to come back: the converged model with its accumulated flow half as large again."""
    d = m.as_dict()
    for k in ("total_dx", "total_dy", "total_rot", "total_div"):
        d[k] *= 1.5
    return model_cls(**d)
