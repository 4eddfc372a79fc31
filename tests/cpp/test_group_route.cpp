// test_group_route.cpp -- bf_rules::group_route (better_flow_amd/csrc/bf_group_rules.h) on a table of cases, on the host: where
// bf_run_groups solves one group -- skipped by the guards, one work-group with its window in LDS, the chip-wide loop
// ("groups_wide"), or BF_ERR_CAPACITY.  With the option off the rule must choose as bf_run_groups always did: the kernel's own
// guards (bf_tiles.hip: tile_optimizer_body) are restated here, independently, and swept against it.
// Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_group_route.cpp (driven by tests/test_group_route_cpu.py).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../better_flow_amd/csrc/bf_group_rules.h"

using bf_rules::GroupFacts;
using bf_rules::GroupPath;
using bf_rules::GroupRoute;

static int failures = 0;

static const char* name(GroupPath p) {
    switch (p) {
        case GroupPath::skipped: return "skipped";
        case GroupPath::lds: return "lds";
        case GroupPath::wide: return "wide";
        case GroupPath::capacity: return "capacity";
    }
    return "?";
}

// scale 3, guards of a 90 x 120 sensor, 100 events at least, the 156 KiB budget, an image capacity of 273 x 363
static GroupFacts facts(int rows, int cols, long long events, bool wide) {
    GroupFacts f;
    f.rows = rows; f.cols = cols; f.events = events; f.scale = 3;
    f.guard_res_x = 90; f.guard_res_y = 120; f.min_events = 100;
    f.lds_budget = 156 * 1024;
    f.max_rows = 273; f.max_cols = 363;
    f.wide = wide;
    return f;
}

static void expect(const char* what, const GroupFacts& f, GroupPath path, long long bytes) {
    const GroupRoute r = bf_rules::group_route(f);
    const bool ok = r.path == path && r.lds_bytes == bytes;
    printf("%-58s %-8s %8lld  %s\n", what, name(r.path), r.lds_bytes, ok ? "ok" : "FAILED");
    if (!ok) {
        printf("    expected %s %lld\n", name(path), bytes);
        ++failures;
    }
}

// What k_group_optimizer decides for a group it is given, with the host's max_px as bf_run_groups always sized it.
static GroupPath kernel_path(const GroupFacts& f) {
    if ((f.rows < f.scale * f.guard_res_x / 15) && (f.cols < f.scale * f.guard_res_y / 15)) return GroupPath::skipped;
    if (f.events < f.min_events) return GroupPath::skipped;
    if (f.rows <= 0 || f.cols <= 0 || (long long)f.rows * f.cols * 16 > f.lds_budget) return GroupPath::capacity;
    return GroupPath::lds;
}

int main() {
    for (int w = 0; w < 2; ++w) {
        const bool wide = w != 0;
        printf("---- groups_wide = %d ----\n", w);
        // the guards: both sides under scale * guard / 15 (18 x 24), or too few events -- the window's size does not matter then
        expect("17 x 23, 5000 events: the window guard", facts(17, 23, 5000, wide), GroupPath::skipped, 0);
        expect("18 x 23, 5000 events: one side reaches the guard", facts(18, 23, 5000, wide), GroupPath::lds, 18ll * 23 * 16);
        expect("17 x 24, 5000 events: the other side does", facts(17, 24, 5000, wide), GroupPath::lds, 17ll * 24 * 16);
        expect("60 x 60, 99 events: min_events", facts(60, 60, 99, wide), GroupPath::skipped, 0);
        expect("60 x 60, 100 events", facts(60, 60, 100, wide), GroupPath::lds, 60ll * 60 * 16);
        expect("216 x 309, 99 events: a skipped group is never wide", facts(216, 309, 99, wide), GroupPath::skipped, 0);
        // exactly the budget: 96 * 104 * 16 = 156 KiB
        expect("96 x 104: exactly 156 KiB stays LDS", facts(96, 104, 5000, wide), GroupPath::lds, 156ll * 1024);
        expect("97 x 104: one more row", facts(97, 104, 5000, wide), wide ? GroupPath::wide : GroupPath::capacity, 0);
        expect("96 x 105: one more column", facts(96, 105, 5000, wide), wide ? GroupPath::wide : GroupPath::capacity, 0);
        expect("216 x 309: the scene's background", facts(216, 309, 14000, wide), wide ? GroupPath::wide : GroupPath::capacity, 0);
        expect("273 x 363: the whole image capacity", facts(273, 363, 14000, wide), wide ? GroupPath::wide : GroupPath::capacity, 0);
        // beyond the context's image capacity, per axis (the pixel count alone would fit in the second and third)
        expect("274 x 363: beyond max_rows", facts(274, 363, 14000, wide), GroupPath::capacity, 0);
        expect("274 x 100: beyond max_rows, fewer pixels", facts(274, 100, 14000, wide), GroupPath::capacity, 0);
        expect("100 x 364: beyond max_cols, fewer pixels", facts(100, 364, 14000, wide), GroupPath::capacity, 0);
        // zero events: the seeded box gives a NEGATIVE window (-267 x -357 here); min_events skips it, and with every guard at
        // zero the window guard still does (both sides are below 0); a window of no pixels that passes the guards is never solved
        expect("no events, min_events 100", facts(-267, -357, 0, wide), GroupPath::skipped, 0);
        GroupFacts f = facts(-267, -357, 0, wide);
        f.min_events = 0; f.guard_res_x = 0; f.guard_res_y = 0;
        expect("no events, no guards: both sides below zero", f, GroupPath::skipped, 0);
        f = facts(-267, 40, 0, wide);
        f.min_events = 0; f.guard_res_x = 0; f.guard_res_y = 0;
        expect("-267 x 40, no guards: a window of no pixels", f, GroupPath::capacity, 0);
        f = facts(0, 40, 500, wide);
        f.guard_res_x = 0; f.guard_res_y = 0;
        expect("0 x 40, no guards", f, GroupPath::capacity, 0);
    }
    // with the option off the rule is the kernel's decision, everywhere: a sweep over windows, counts, guards and scales
    long long swept = 0, differ = 0;
    for (int scale = 1; scale <= 9; scale += 2)
        for (int rows = -30; rows <= 400; rows += 7)
            for (int cols = -30; cols <= 400; cols += 11)
                for (long long events : {0ll, 1ll, 99ll, 100ll, 5000ll})
                    for (int guard : {0, 15, 90, 260}) {
                        GroupFacts f = facts(rows, cols, events, false);
                        f.scale = scale; f.guard_res_x = guard; f.guard_res_y = guard + 30;
                        const GroupRoute off = bf_rules::group_route(f);
                        ++swept;
                        if (off.path != kernel_path(f) || (off.path == GroupPath::lds) != (off.lds_bytes > 0)) ++differ;
                        f.wide = true;
                        const GroupRoute on = bf_rules::group_route(f);
                        // the option moves capacity groups only, and only those inside the image capacity
                        const bool moved = on.path != off.path;
                        if (moved && !(off.path == GroupPath::capacity && on.path == GroupPath::wide && rows > 0 && cols > 0 &&
                                       rows <= f.max_rows && cols <= f.max_cols))
                            ++differ;
                        if (!moved && off.path == GroupPath::capacity && rows > 0 && cols > 0 && rows <= f.max_rows && cols <= f.max_cols)
                            ++differ;
                    }
    printf("sweep: %lld cases, %lld differ from the kernel's guards\n", swept, differ);
    if (differ) ++failures;
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
