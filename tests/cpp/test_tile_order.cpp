// Host-only sweep of bf_rules::tile_of_block (better_flow_amd/csrc/bf_plan_rules.h): which tile a work-group of the stencil launch
// takes.  For every tile count 1 .. 4096 and for the tile grids of the BASELINE geometries at scale 3:
//   * block -> tile is a bijection on [0, ntiles),
//   * the blocks of one residue class mod 8 (b, b + 8, ...: what has been observed to share an L2) take ONE contiguous run of
//     row-major tile indices, in launch order, and the runs tile [0, ntiles) in class order,
//   * the class sizes differ by at most 1,
//   * tile -> (tile row, tile column) = (t / gx, t % gx) reaches every tile of the gy x gx grid once.
// For config 2's grid (346 x 260 at scale 3) it counts the vertically adjacent tile pairs whose two tiles share a class: all but
// at most 7 tile rows' worth with this order (8 bands have 7 boundaries), none with the identity order the kernel had.
#include <cstdio>
#include <vector>

#include "../../better_flow_amd/csrc/bf_plan_rules.h"

using namespace bf_rules;

static long long failures = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (failures++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

static void check_count(int ntiles) {
    std::vector<int> owner(ntiles, -1);
    int lo[kTileClasses], hi[kTileClasses], cnt[kTileClasses];
    for (int x = 0; x < kTileClasses; ++x) { lo[x] = ntiles; hi[x] = -1; cnt[x] = 0; }
    for (int b = 0; b < ntiles; ++b) {
        const int t = tile_of_block(b, ntiles);
        CHECK(t >= 0 && t < ntiles, "ntiles %d: block %d -> tile %d out of range", ntiles, b, t);
        if (t < 0 || t >= ntiles) continue;
        CHECK(owner[t] < 0, "ntiles %d: tile %d taken by blocks %d and %d", ntiles, t, owner[t], b);
        owner[t] = b;
        const int x = b % kTileClasses;
        // in launch order a class walks its run upwards, one tile at a time
        if (cnt[x] > 0) CHECK(t == hi[x] + 1, "ntiles %d: class %d is not one run (tile %d after %d)", ntiles, x, t, hi[x]);
        if (t < lo[x]) lo[x] = t;
        if (t > hi[x]) hi[x] = t;
        ++cnt[x];
    }
    for (int t = 0; t < ntiles; ++t) CHECK(owner[t] >= 0, "ntiles %d: tile %d has no block", ntiles, t);
    int cmin = ntiles, cmax = 0, next = 0;
    for (int x = 0; x < kTileClasses; ++x) {
        if (cnt[x] < cmin) cmin = cnt[x];
        if (cnt[x] > cmax) cmax = cnt[x];
        if (cnt[x] == 0) continue;
        CHECK(hi[x] - lo[x] + 1 == cnt[x], "ntiles %d: class %d holds %d tiles over [%d, %d]", ntiles, x, cnt[x], lo[x], hi[x]);
        CHECK(lo[x] == next, "ntiles %d: class %d starts at %d, not %d", ntiles, x, lo[x], next);
        next = hi[x] + 1;
    }
    CHECK(next == ntiles, "ntiles %d: the runs end at %d", ntiles, next);
    CHECK(cmax - cmin <= 1, "ntiles %d: class sizes %d .. %d", ntiles, cmin, cmax);
}

// vertically adjacent tile pairs of a gy x gx grid whose blocks are in one class
static int shared_vertical_pairs(int gx, int gy, bool identity) {
    const int ntiles = gx * gy;
    std::vector<int> cls(ntiles);
    for (int b = 0; b < ntiles; ++b) cls[identity ? b : tile_of_block(b, ntiles)] = b % kTileClasses;
    int shared = 0;
    for (int r = 0; r + 1 < gy; ++r)
        for (int c = 0; c < gx; ++c) shared += cls[r * gx + c] == cls[(r + 1) * gx + c] ? 1 : 0;
    return shared;
}

int main() {
    for (int ntiles = 1; ntiles <= 4096; ++ntiles) check_count(ntiles);

    // BASELINE.json's sensors (rows x columns) at scale 3: R = 3 H scaled rows, C = 3 W scaled columns
    const int sensors[][2] = {{180, 240}, {260, 346}, {480, 640}, {720, 1280}};
    for (const auto& hw : sensors) {
        const int R = 3 * hw[0], C = 3 * hw[1];
        const int gx = (C + kStencilTileC - 1) / kStencilTileC, gy = (R + kStencilTileR - 1) / kStencilTileR;
        const int ntiles = (int)stencil_tiles(R, C);
        CHECK(ntiles == gx * gy, "%d x %d: %d tiles, grid %d x %d", R, C, ntiles, gy, gx);
        check_count(ntiles);
        std::vector<int> seen(ntiles, 0);
        for (int b = 0; b < ntiles; ++b) {
            const int t = tile_of_block(b, ntiles), row = t / gx, col = t % gx;
            CHECK(row >= 0 && row < gy && col >= 0 && col < gx, "%d x %d: block %d -> tile (%d, %d)", R, C, b, row, col);
            if (row >= 0 && row < gy && col >= 0 && col < gx) ++seen[row * gx + col];
        }
        for (int t = 0; t < ntiles; ++t) CHECK(seen[t] == 1, "%d x %d: tile %d taken %d times", R, C, t, seen[t]);
        const int pairs = gx * (gy - 1), banded = shared_vertical_pairs(gx, gy, false), ident = shared_vertical_pairs(gx, gy, true);
        printf("# %4d x %4d scaled pixels: %2d x %2d tiles, %4d vertical pairs: %4d share a class in band order, %d in launch order\n", R, C,
               gy, gx, pairs, banded, ident);
        CHECK(pairs - banded <= 7 * gx, "%d x %d: %d vertical pairs cross a class boundary (> 7 rows of %d)", R, C, pairs - banded, gx);
        if (hw[0] == 260) {   // config 2: 49 x 17 tiles
            CHECK(gx == 17 && gy == 49, "config 2's grid is %d x %d", gy, gx);
            CHECK(ident == 0, "config 2: %d vertical pairs share a class in launch order", ident);
        }
    }
    // the same grid transposed (13 columns of 65 tiles): the count holds for either orientation of the sensor
    CHECK(13 * 64 - shared_vertical_pairs(13, 65, false) <= 7 * 13 && shared_vertical_pairs(13, 65, true) == 0, "13 x 65 grid");

    if (failures) { printf("%lld failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
