// bf_group_rules.h -- where one group of bf_run_groups is solved, as a pure function of plain numbers: no bf_ctx, no HIP,
// nothing but <cstdint>.  bf_run_groups (bf_tiles_abi.cpp) asks it for every group, so the host's sizing of the launch, the
// groups it hands to the chip-wide loop and what the caller is told cannot disagree; tests/cpp/test_group_route.cpp holds it to
// a table of cases on the host.  The guards are those of OptimizerRolling::run as k_group_optimizer evaluates them
// (bf_tiles.hip: tile_optimizer_body) -- the kernel stays the authority for the groups it is given, this rule says which those are.
#pragma once
#include <cstdint>

namespace bf_rules {

enum class GroupPath : int {
    skipped,    // the guards of run() skip it (BF_SKIPPED): no planes
    lds,        // one work-group, its window in LDS (GroupRoute::lds_bytes)
    wide,       // the chip-wide loop of bf_run, inside the call ("groups_wide" = 1)
    capacity,   // BF_ERR_CAPACITY in the group's own rc: not solved
};

struct GroupRoute {
    GroupPath path;
    long long lds_bytes;   // the three planes of the window (8 + 4 + 4 bytes per pixel); 0 unless path == lds
};

struct GroupFacts {
    int rows = 0, cols = 0;            // the window: scale * (max - min) + scale per axis (negative for a group without events)
    long long events = 0;
    int scale = 1;
    int guard_res_x = 0, guard_res_y = 0, min_events = 0;   // the guards of bf_group_opts
    long long lds_budget = 0;          // bytes of dynamic LDS one work-group may take
    int max_rows = 0, max_cols = 0;    // the context's image capacity (bf_create)
    bool wide = false;                 // the option
};

inline GroupRoute group_route(const GroupFacts& f) {
    const bool small = (f.rows < f.scale * f.guard_res_x / 15) && (f.cols < f.scale * f.guard_res_y / 15);
    if (small || f.events < (long long)f.min_events) return {GroupPath::skipped, 0};
    if (f.rows <= 0 || f.cols <= 0) return {GroupPath::capacity, 0};
    const long long bytes = (long long)f.rows * (long long)f.cols * 16;
    if (bytes <= f.lds_budget) return {GroupPath::lds, bytes};
    if (f.wide && f.rows <= f.max_rows && f.cols <= f.max_cols) return {GroupPath::wide, 0};
    return {GroupPath::capacity, 0};
}

}  // namespace bf_rules
