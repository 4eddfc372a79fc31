#!/usr/bin/env python3
"""How many events change their scatter pixel from one iteration to the next (no GPU).

Steps the CPU oracle (tests/oracle.py: iteration_step under the loop control of OptimizerRolling::run,
optimizer_rolling.h:48-125) through a cold run of bench.py's config 2 slice and compares every event's scatter pixel
trunc(pr * scale + shift) (accel_lib.h:154-158) before and after each warp.  An event is a MOVER when the pixel differs or
when it enters or leaves the window; a mover costs the delta-scatter loop two atomics (one if it came from or went outside),
every other event none.

    python scripts/mover_fraction.py [seed ...]          (default: seed 1)
    python scripts/mover_fraction.py --events 20000 --height 33 --width 65 --scale 3 7
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def scatter_pixels(cloud, w):
    """Linear scatter pixel of every event from its current pr, -1 outside the window (accel_lib.h:154-158)."""
    s, hs = w.scale, w.scale // 2
    with np.errstate(invalid="ignore"):
        X = np.trunc(cloud.pr_x * s + float(int(w.x_shift)))
        Y = np.trunc(cloud.pr_y * s + float(int(w.y_shift)))
    inside = (X >= hs) & (X < w.metric_wsizex + hs) & (Y >= hs) & (Y < w.metric_wsizey + hs)   # (NaN: outside)
    k = np.full(cloud.n, -1, np.int64)
    k[inside] = X[inside].astype(np.int64) * w.scale_img_y + Y[inside].astype(np.int64)
    return k


def step_run(oracle, cloud, w, max_iter=-1, hard_cap=200000, on_step=None, model=None):
    """OptimizerRolling::run (oracle/bf_oracle.c: bfo_run) written out around iteration_step; on_step(it, before, after) gets the
    scatter pixels on either side of every warp.  `model`: a warm start (the model bfo_set_model returned).  Returns the iteration
    count."""
    m, lp = (model if model is not None else oracle.Model()), oracle.Loop()
    lp.x_divider = lp.y_divider = 1.0
    lp.rot_divider = lp.div_divider = 10000.0
    f32 = np.float32

    def step():
        before = scatter_pixels(cloud, w)
        cloud.iteration_step(w, m, lp)
        lp.itercount += 1
        if on_step:
            on_step(lp.itercount, before, scatter_pixels(cloud, w))
    step()
    while lp.x_divider < 320 or lp.y_divider < 320 or lp.rot_divider < 32000 or lp.div_divider < 32000:
        if (abs(m.dx / float(lp.x_divider)) < 1e-5 and abs(m.dy / float(lp.y_divider)) < 1e-5 and
                abs(m.rot / float(lp.rot_divider)) < 1e-4 and abs(m.div / float(lp.div_divider)) < 1e-1):
            break
        old = [float(f32(v)) for v in (m.dx, m.dy, m.rot, m.div)]
        step()
        if max_iter > 0 and lp.itercount > max_iter:
            break
        if m.dx * old[0] < 0: lp.x_divider *= 2
        if m.dy * old[1] < 0: lp.y_divider *= 2
        if m.rot * old[2] < 0: lp.rot_divider *= 2
        if m.div * old[3] < 0: lp.div_divider *= 2
        if hard_cap > 0 and lp.itercount >= hard_cap:
            break
    return int(lp.itercount)


def transitions(before, after):
    """Events per transition: (inside -> another pixel inside, inside -> outside, outside -> inside, unchanged)."""
    bi, ai = before >= 0, after >= 0
    return (int(np.count_nonzero(bi & ai & (before != after))), int(np.count_nonzero(bi & ~ai)),
            int(np.count_nonzero(~bi & ai)), int(np.count_nonzero(before == after)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("seeds", type=int, nargs="*", default=[1])
    ap.add_argument("--events", type=int, default=1000000)
    ap.add_argument("--height", type=int, default=260)
    ap.add_argument("--width", type=int, default=346)
    ap.add_argument("--scale", type=int, default=3)
    ap.add_argument("--duration", type=float, default=0.030)
    a = ap.parse_args()
    import oracle
    from better_flow_amd import synth
    oracle.build()
    for seed in a.seeds:
        sl = synth.make_slice(a.events, a.height, a.width, a.duration, seed=seed)
        cloud = oracle.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
        w = cloud.set_cloud(a.scale, a.height, a.width)
        rows = []
        step_run(oracle, cloud, w, on_step=lambda it, b, f: rows.append(transitions(b, f)))
        t = np.array(rows, np.float64)
        share = (t[:, 0] + t[:, 1] + t[:, 2]) / cloud.n
        atomics = (2 * t[:, 0] + t[:, 1] + t[:, 2])
        final = scatter_pixels(cloud, w)
        print("seed %d: %d events, %d x %d pixels, %d iterations" % (seed, cloud.n, w.scale_img_x, w.scale_img_y, len(rows)))
        print("  movers per iteration: mean %.2f %%, median %.2f %%, max %.2f %%; <= 10 %% in %.1f %% of the iterations, "
              "<= 20 %% in %.1f %%" % (100 * share.mean(), 100 * np.median(share), 100 * share.max(),
                                     100 * np.mean(share <= 0.10), 100 * np.mean(share <= 0.20)))
        print("  of all event-iterations: other pixel %.3f %%, left the window %.4f %%, entered it %.4f %%, unchanged %.3f %%" %
              tuple(100 * t[:, k].sum() / (cloud.n * len(rows)) for k in range(4)))
        print("  atomics per iteration: mean %.0f (a rebuild: %d)" % (atomics.mean(), int(np.count_nonzero(final >= 0))))
        print("  by blocks of 50 iterations: " + " ".join("%.1f" % (100 * share[k:k + 50].mean()) for k in range(0, len(share), 50)))
        print("  support of the last image: %d of %d scatter pixels" % (len(np.unique(final[final >= 0])), w.scale_img_x * w.scale_img_y))


if __name__ == "__main__":
    main()
