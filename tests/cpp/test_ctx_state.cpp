// Walks every slice state (better_flow_amd/csrc/bf_ctx_state.h) that a fresh context can reach under every sequence of the
// header's transitions -- a breadth-first search over the flags' bit patterns, each transition taken only where the call sites
// that use it guarantee its precondition -- and checks two things on the way:
//   * every transition does to the flags exactly what the block it replaced did: `want` below restates those blocks field by
//     field from the C-ABI files as they were before the header existed, and the state after the header's transition must equal
//     the state after `want`, in every flag (so a line missing from a transition, or one too many, fails on the first state
//     where it matters);
//   * every reached state keeps what the readers in the C-ABI files rely on.
// "A run is going on" (between run_began and run_ended, or the run's failure) is a bit of the walker, not read off the flags
// under test: inside it only the run's own transitions are taken.  A failure prints the state and the sequence of transitions
// that led to it.
//
//   g++ -O2 -std=c++14 -Wall tests/cpp/test_ctx_state.cpp -o test_ctx_state && ./test_ctx_state
// (-DBF_CTX_STATE_HEADER='"<file>"' walks another copy of the header: tests/test_ctx_state_cpu.py feeds it broken ones.)
#include <cstdio>
#include <cstdint>
#include <functional>
#include <queue>
#include <string>
#include <vector>

#ifndef BF_CTX_STATE_HEADER
#define BF_CTX_STATE_HEADER "../../better_flow_amd/csrc/bf_ctx_state.h"
#endif
#include BF_CTX_STATE_HEADER

using bf_state::SliceState;

namespace {

#define BF_FLAGS(X)                                                                                                         \
    X(uploaded) X(stats_valid) X(all_noise) X(have_window) X(degenerate) X(pending_warp) X(p_clean) X(n_valid) X(uv_valid) \
    X(out_sorted) X(has_perm) X(use_binned) X(fused_ok) X(fused_shared) X(seg_valid) X(groups_valid) X(glob_valid) X(have_lwin)

constexpr int kInRunBit = 19;   // the walker's own bit, above the 18 flags and cs

uint32_t pack(const SliceState& s) {
    uint32_t v = 0;
    int b = 0;
#define X(f) v |= (uint32_t)(s.f ? 1u : 0u) << b++;
    BF_FLAGS(X)
#undef X
    v |= (uint32_t)(s.cs & 1) << b++;
    return v;
}

SliceState unpack(uint32_t v) {
    SliceState s;
    int b = 0;
#define X(f) s.f = ((v >> b++) & 1u) != 0;
    BF_FLAGS(X)
#undef X
    s.cs = (int)((v >> b++) & 1u);
    s.groups_K = 2;
    return s;
}

std::string show(const SliceState& s) {
    std::string out;
#define X(f) if (s.f) out += #f " ";
    BF_FLAGS(X)
#undef X
    out += s.cs ? "cs=1" : "cs=0";
    return out;
}

// The blocks the transitions replaced, as the C-ABI files wrote them.
void want_reset(SliceState& s) { s.p_clean = true; s.n_valid = false; s.uv_valid = false; s.out_sorted = false; }
void want_warped(SliceState& s) { s.p_clean = false; s.seg_valid = false; s.n_valid = true; s.uv_valid = false; s.out_sorted = false; }

enum When { outside_run, inside_run, begins_run, ends_run };

struct Step {
    const char* name;
    When when;
    std::function<bool(const SliceState&)> pre;    // what every call site of the transition guarantees
    std::function<void(SliceState&)> go;           // the header's transition
    std::function<void(SliceState&)> want;         // what the code it replaced assigned
};

// an operator on the live window behind window_op_begin (bf_operators.cpp): a usable window, bf_set_model's warp applied
bool window_op(const SliceState& s) { return s.have_window && !s.degenerate && !s.pending_warp; }
// behind a sort by sensor tile or by group, before anything else touches the context
bool sorted_outside(const SliceState& s) { return s.uploaded && s.has_perm && !s.use_binned && !s.fused_ok; }
bool always(const SliceState&) { return true; }
bool is_uploaded(const SliceState& s) { return s.uploaded; }
bool planned_grid(const SliceState& s) { return s.use_binned || s.fused_ok; }

const std::vector<Step>& steps() {
    static const std::vector<Step> all = {
        // slice_staged + after_upload (bf_upload.cpp, bf_ctx.h)
        {"slice_uploaded", outside_run, always, [](SliceState& s) { s.slice_uploaded(); },
         [](SliceState& s) {
             s.cs = 0; s.has_perm = false;
             s.p_clean = true; s.stats_valid = false; s.have_lwin = false; s.glob_valid = false; s.seg_valid = false;
             s.groups_valid = false; s.uploaded = true; s.have_window = false; s.all_noise = false; s.pending_warp = false;
             s.n_valid = false; s.uv_valid = false; s.out_sorted = false;
         }},
        // (fold_stats may run on the uploading thread while a run goes on)
        {"stats_folded", outside_run, is_uploaded, [](SliceState& s) { s.stats_folded(); }, [](SliceState& s) { s.stats_valid = true; }},
        {"stats_folded (under a run)", inside_run, is_uploaded, [](SliceState& s) { s.stats_folded(); }, [](SliceState& s) { s.stats_valid = true; }},
        // bf_run's window guard, ahead of the run proper
        {"all_noise_marked", outside_run, [](const SliceState& s) { return s.have_window; }, [](SliceState& s) { s.all_noise_marked(); },
         [](SliceState& s) { s.all_noise = true; }},
        // bf_set_cloud
        {"window_set(degenerate)", outside_run, is_uploaded, [](SliceState& s) { s.window_set(true); },
         [](SliceState& s) { s.seg_valid = false; s.have_window = true; s.degenerate = true; s.pending_warp = false; }},
        {"window_set(usable)", outside_run, is_uploaded, [](SliceState& s) { s.window_set(false); },
         [](SliceState& s) {
             s.seg_valid = false; s.degenerate = false; s.have_window = true; s.pending_warp = false; s.all_noise = false;
             want_reset(s);
         }},
        // plan_slice's decisions: bf_set_cloud, behind window_set(usable)
        {"planned_binned(1)", outside_run, window_op, [](SliceState& s) { s.planned_binned(true); }, [](SliceState& s) { s.use_binned = true; }},
        {"planned_binned(0)", outside_run, window_op, [](SliceState& s) { s.planned_binned(false); }, [](SliceState& s) { s.use_binned = false; }},
        {"planned_one_kernel(1)", outside_run, window_op, [](SliceState& s) { s.planned_one_kernel(true); }, [](SliceState& s) { s.fused_ok = true; }},
        {"planned_one_kernel(0)", outside_run, window_op, [](SliceState& s) { s.planned_one_kernel(false); }, [](SliceState& s) { s.fused_ok = false; }},
        {"planned_one_kernel_shared(1)", outside_run, window_op, [](SliceState& s) { s.planned_one_kernel_shared(true); },
         [](SliceState& s) { s.fused_shared = true; }},
        {"planned_one_kernel_shared(0)", outside_run, window_op, [](SliceState& s) { s.planned_one_kernel_shared(false); },
         [](SliceState& s) { s.fused_shared = false; }},
        {"events_reset", outside_run, is_uploaded, [](SliceState& s) { s.events_reset(); }, want_reset},
        // bf_project_4param_reinit / bf_project_4param
        {"events_warped", outside_run, window_op, [](SliceState& s) { s.events_warped(); }, want_warped},
        // bf_set_model / flush_pending
        {"warp_pending", outside_run, [](const SliceState& s) { return s.have_window && !s.degenerate; }, [](SliceState& s) { s.warp_pending(); },
         [](SliceState& s) { s.pending_warp = true; }},
        {"pending_applied", outside_run, [](const SliceState& s) { return s.pending_warp; }, [](SliceState& s) { s.pending_applied(); },
         [](SliceState& s) { s.pending_warp = false; want_warped(s); }},
        // bf_run: run_begin, then run_end (the device's choice of set first, where the loop sorts by tile), or a failure between
        {"run_began", begins_run, [](const SliceState& s) { return s.have_window; }, [](SliceState& s) { s.run_began(); },
         [](SliceState& s) { s.p_clean = false; s.seg_valid = false; s.pending_warp = false; }},
        {"sorted_by_plan(0)", inside_run, planned_grid, [](SliceState& s) { s.sorted_by_plan(0); }, [](SliceState& s) { s.cs = 0; s.has_perm = true; }},
        {"sorted_by_plan(1)", inside_run, planned_grid, [](SliceState& s) { s.sorted_by_plan(1); }, [](SliceState& s) { s.cs = 1; s.has_perm = true; }},
        {"run_ended(uv)", ends_run, always, [](SliceState& s) { s.run_ended(true); },
         [](SliceState& s) { s.n_valid = true; s.uv_valid = true; s.out_sorted = true; }},
        {"run_ended(no uv)", ends_run, always, [](SliceState& s) { s.run_ended(false); },
         [](SliceState& s) { s.n_valid = true; s.uv_valid = false; s.out_sorted = true; }},
        {"run failed", ends_run, always, [](SliceState&) {}, [](SliceState&) {}},
        // tiles_prepare / bf_run_groups, then tiles_collect or the end of bf_local_run_tiles
        {"sorted_outside_plan", outside_run, is_uploaded, [](SliceState& s) { s.sorted_outside_plan(); },
         [](SliceState& s) { s.cs ^= 1; s.has_perm = true; s.use_binned = false; s.fused_ok = false; }},
        {"tile_run_collected", outside_run, sorted_outside, [](SliceState& s) { s.tile_run_collected(); },
         [](SliceState& s) {
             want_warped(s);
             s.pending_warp = false; s.have_window = true; s.degenerate = false; s.use_binned = false; s.fused_ok = false;
         }},
        {"local_tile_run_collected", outside_run, sorted_outside, [](SliceState& s) { s.local_tile_run_collected(); },
         [](SliceState& s) { want_reset(s); s.pending_warp = false; s.use_binned = false; s.fused_ok = false; s.have_lwin = false; }},
        // materialize_outputs, ensure_uv, bf_writeout_events
        {"outputs_materialised", outside_run, [](const SliceState& s) { return s.out_sorted; }, [](SliceState& s) { s.outputs_materialised(); },
         [](SliceState& s) { s.out_sorted = false; }},
        {"uv_computed", outside_run, [](const SliceState& s) { return window_op(s) && s.n_valid && !s.out_sorted && !s.uv_valid; },
         [](SliceState& s) { s.uv_computed(); }, [](SliceState& s) { s.uv_valid = true; }},
        {"uv_buffer_reused", outside_run, [](const SliceState& s) { return window_op(s) && !s.out_sorted; }, [](SliceState& s) { s.uv_buffer_reused(); },
         [](SliceState& s) { s.uv_valid = false; }},
        // the single-flag sites
        {"segmentation_held", outside_run, window_op, [](SliceState& s) { s.segmentation_held(); }, [](SliceState& s) { s.seg_valid = true; }},
        {"segmentation_dropped", outside_run, always, [](SliceState& s) { s.segmentation_dropped(); }, [](SliceState& s) { s.seg_valid = false; }},
        {"grouping_held", outside_run, is_uploaded, [](SliceState& s) { s.grouping_held(3); }, [](SliceState& s) { s.groups_K = 3; s.groups_valid = true; }},
        {"grouping_dropped", outside_run, is_uploaded, [](SliceState& s) { s.grouping_dropped(); }, [](SliceState& s) { s.groups_valid = false; }},
        {"local_window_held", outside_run, is_uploaded, [](SliceState& s) { s.local_window_held(); }, [](SliceState& s) { s.have_lwin = true; }},
        {"local_window_dropped", outside_run, always, [](SliceState& s) { s.local_window_dropped(); }, [](SliceState& s) { s.have_lwin = false; }},
        {"global_window_held", outside_run, is_uploaded, [](SliceState& s) { s.global_window_held(); }, [](SliceState& s) { s.glob_valid = true; }},
        {"global_window_dropped", outside_run, is_uploaded, [](SliceState& s) { s.global_window_dropped(); }, [](SliceState& s) { s.glob_valid = false; }},
    };
    return all;
}

// What the readers rely on; null when the state is fine, else the broken rule.
const char* broken(const SliceState& s) {
    if (s.uv_valid && !s.n_valid) return "uv_valid implies n_valid (ensure_uv computes the flow from d_nxny)";
    if (s.out_sorted && !s.n_valid) return "out_sorted implies n_valid (materialize_outputs un-permutes d_nxny)";
    if (s.pending_warp && !(s.have_window && !s.degenerate)) return "pending_warp implies a usable window (flush_pending warps into its planes)";
    if (s.p_clean && s.n_valid) return "p_clean implies !n_valid (Event::reset state has no per-event output)";
    if (s.seg_valid && !s.have_window) return "seg_valid implies have_window (bf_segment_get sizes its copies from the window)";
    if (s.have_window && !s.uploaded) return "have_window implies uploaded (window_op_begin asks for the window alone)";
    if (!s.has_perm && s.cs != 0) return "unsorted events are in set 0 (the upload stages them there)";
    return nullptr;
}

// What must hold when a transition has just been taken, beside the invariants and the equality with `want`: the issue's own list.
const char* broken_after(const Step& st, const SliceState& s) {
    const std::string name = st.name;
    if (name == "slice_uploaded" && (s.n_valid || s.uv_valid || s.seg_valid || s.groups_valid || s.glob_valid || s.have_lwin))
        return "an upload leaves no per-event output, segmentation, grouping or window behind";
    if ((name == "events_warped" || name == "pending_applied" || name == "tile_run_collected") && s.seg_valid)
        return "a warp drops the segmentation";
    // (the whole run: run_began's writes are still in force here, nothing but the run's own transitions came between)
    if (name.compare(0, 9, "run_ended") == 0 && (s.seg_valid || s.p_clean || s.pending_warp || !s.n_valid || !s.out_sorted))
        return "a completed run leaves warped events, sorted outputs, no segmentation and no pending warp";
    return nullptr;
}

}  // namespace

int main() {
    const uint32_t kStates = 1u << (kInRunBit + 1);
    std::vector<int32_t> from(kStates, -2), by(kStates, -1);   // predecessor state (-2: not reached, -1: the start) and step
    std::queue<uint32_t> todo;
    const uint32_t start = pack(SliceState());
    from[start] = -1;
    todo.push(start);
    auto path = [&](uint32_t v) {
        std::vector<const char*> names;
        for (; from[v] >= 0; v = (uint32_t)from[v]) names.push_back(steps()[(size_t)by[v]].name);
        std::string out = "fresh";
        for (size_t i = names.size(); i-- > 0;) { out += " -> "; out += names[i]; }
        return out;
    };
    long reached = 0, taken = 0;
    int bad = 0;
    while (!todo.empty() && bad < 5) {
        const uint32_t v = todo.front();
        todo.pop();
        ++reached;
        const bool in_run = ((v >> kInRunBit) & 1u) != 0;
        const uint32_t flags = v & ((1u << kInRunBit) - 1);
        const SliceState s = unpack(flags);
        if (pack(s) != flags) { printf("pack / unpack disagree on %u\n", flags); return 1; }
        if (const char* why = broken(s)) {
            printf("INVARIANT BROKEN: %s\n  state: %s\n  path: %s\n", why, show(s).c_str(), path(v).c_str());
            ++bad;
            continue;
        }
        for (size_t k = 0; k < steps().size(); ++k) {
            const Step& st = steps()[k];
            if (in_run != (st.when == inside_run || st.when == ends_run) || !st.pre(s)) continue;
            SliceState t = s, w = s;
            st.go(t);
            st.want(w);
            ++taken;
            if (pack(t) != pack(w) || t.groups_K != w.groups_K) {
                printf("TRANSITION DIFFERS from the block it replaced: %s\n  from:  %s\n  gives: %s\n  block: %s\n  path: %s\n", st.name,
                       show(s).c_str(), show(t).c_str(), show(w).c_str(), path(v).c_str());
                ++bad;
            }
            if (const char* why = broken_after(st, t)) {
                printf("BROKEN after %s: %s\n  state: %s\n  path: %s\n", st.name, why, show(t).c_str(), path(v).c_str());
                ++bad;
            }
            const bool run_next = st.when == begins_run || st.when == inside_run;
            const uint32_t next = pack(t) | ((run_next ? 1u : 0u) << kInRunBit);
            if (from[next] == -2) { from[next] = (int32_t)v; by[next] = (int32_t)k; todo.push(next); }
        }
    }
    printf("%ld states reached, %ld transitions taken, %zu transitions\n", reached, taken, steps().size());
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
