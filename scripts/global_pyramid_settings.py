"""Regenerates DESIGN.md's table of pyramid settings on the two-motion slice (tests/global_cells_ref.py: two 8 000-event
halves on 64 x 128, 32 x 32 cells, scale 3, window 15, the default 180 x 80 lattice), on the numpy restatement
(tests/global_pyramid_ref.py), no GPU: per (levels, factor, radius) the candidates evaluated, per level, and how many of the
eight cells answer within 2 lattice steps of their half's motion.  S(k, cell) does not depend on what else is evaluated,
so one cache serves every setting.  The cheapest setting with 8 of 8 is the one tests/test_global_pyramid_cpu.py commits.
About 20 s."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import global_cells_ref as GC  # noqa: E402
import global_pyramid_ref as P  # noqa: E402
import global_ref as G  # noqa: E402

SETTINGS = [(3, 4, 1), (3, 4, 2), (3, 4, 3), (3, 3, 1), (3, 3, 2), (3, 2, 1), (3, 2, 2), (2, 8, 2), (2, 8, 3), (2, 8, 4),
            (2, 4, 1), (2, 4, 2), (2, 4, 3)]


def main():
    ref = GC.GlobalCells(*GC.two_motion_slice(), 64, 128, 32, 32, scale=3, metric_wsize=15)
    xs, ys = G.default_grid()
    cache = {}

    def score(k):
        if k not in cache:
            cache[k] = ref.project_all_cells(xs[k // len(ys)], ys[k % len(ys)])
        return cache[k]

    tol = 2 * GC.GRID_STEP
    rows = []
    for levels, factor, radius in SETTINGS:
        out = P.search_pyramid(ref, xs, ys, levels, factor, radius, score=score)
        c, ok = out["cells"], 0
        for cx in range(2):
            for cy in range(4):
                tu, tv = GC.TWO_MOTION_TRUTH["left" if cy < 2 else "right"]
                ok += bool(abs(c["best_u"][cx, cy] - tu) <= tol and abs(c["best_v"][cx, cy] - tv) <= tol)
        rows.append((len(out["evaluated"]), (levels, factor, radius), out["level_count"], ok))
    print("| (levels, factor, radius) | evaluated (per level) | cells within 2 steps |\n|---|---|---|")
    for n, setting, counts, ok in sorted(rows):
        print("| %s | %d %s | %d of 8 |" % (setting, n, tuple(counts), ok))
    print("cheapest with 8 of 8:", min(r for r in rows if r[3] == 8)[1])


if __name__ == "__main__":
    main()
