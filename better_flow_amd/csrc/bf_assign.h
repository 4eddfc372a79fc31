// bf_assign.h -- launchers of the kernels on the K models' vote planes -- assignment (bf_assign.hip), projection of a grouping
// (bf_project.hip) and merge gains (bf_merge.hip) -- for bf_assign_abi.cpp, which sets up the planes they share once; and of the
// kernels that propose the candidate models (bf_propose.hip) for bf_propose_abi.cpp.  The definitions they implement are in
// include/bf_accel.h ("event groups: assignment", "event groups: candidate models", "event groups: projection", "event groups:
// merge gains").  Where the words of a result block sit is bf_group_blocks.h's, for the kernels and the host alike.  Every
// launcher enqueues plain launches on the given stream; no kernel waits for another work-group.  What the kernel files share on the device is in bf_device_fns.h: the box
// sum of a tile (box_sum_tile: k_assign_box, k_propose_box), the tally per distinct key of a wave (for_each_wave_key) and the
// wave reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bf_device.h"
#include "bf_group_blocks.h"

namespace bf {

constexpr int kAssignMaxModels = 64;
constexpr long long kAssignMaxWords = 1ll << 27;   // K x R x C vote words (and as many box sums when scale > 1)
// The events as stored (slot order; perm null: slot == upload index), the K warps, the window, and the prior (upload order;
// null: every event votes under every model).
struct AssignArgs {
    const uint32_t* xy; const int32_t* t; const uint32_t* perm;
    const WarpParams* wp;      // K, read on the scalar unit
    const int32_t* prior;
    long long n;
    int K, scale, x_sh, y_sh, wsx, wsy, R, C;
};

// V (K x R x C words, zero) += the votes.
void launch_assign_vote(const AssignArgs& a, uint32_t* V, hipStream_t s);
// B_k = the scale x scale box sum of V_k, every word of B written (scale > 1).
void launch_assign_box(const uint32_t* V, uint32_t* B, int K, int R, int C, int scale, hipStream_t s);
// gid / score through perm, and the result block (AssignBlock, zero on entry).  B: the box sums, or V itself at scale 1.
void launch_assign_pick(const AssignArgs& a, const uint32_t* B, int min_score, int32_t* gid, int32_t* score, uint32_t* out,
                        hipStream_t s);

// The proposal kernels (bf_propose.hip; include/bf_accel.h, "event groups: candidate models").
constexpr int kProposeMaxRadius = 8, kProposeMaxSuppress = 64, kProposeMaxModels = 64;
constexpr long long kProposeMaxBins = 1ll << 22;
constexpr size_t kProposeLdsBytes = 63 * 1024;   // the LDS form: H and the two value tables in one work-group's LDS
// The per-event best state (upload order), the lattice's value tables (n_x doubles, then n_y) and its planes.
struct ProposeArgs {
    const double *max_score, *best_nx, *best_ny;
    const double* tab;
    long long n;
    int n_x, n_y;
};
// Words of the result block: voted, unscored, off_lattice, proposals, then (index, votes, peak) per proposal.
constexpr int kProposeOutHead = 4;
inline int propose_out_words(int K) { return kProposeOutHead + 3 * K; }
inline bool propose_fits_lds(long long n_x, long long n_y) {
    return (size_t)(n_x * n_y) * sizeof(uint32_t) + (size_t)(n_x + n_y) * sizeof(double) <= kProposeLdsBytes;
}
// H (n_x * n_y words, zero) += the votes; out[0 .. 3) (zero) += the three counts.  Returns the form that ran: 1 LDS, 2 global.
int launch_propose_vote(const ProposeArgs& a, uint32_t* H, uint32_t* out, hipStream_t s);
// B = the (2 r + 1)^2 box sum of H, every word of B written.
void launch_propose_box(const uint32_t* H, uint32_t* B, int n_x, int n_y, int radius, hipStream_t s);
// The greedy pick: out[3] = the proposals, out[4 + 3 p ..] = (index, B, H) of pick p.  One work-group.
void launch_propose_pick(const uint32_t* H, const uint32_t* B, int n_x, int n_y, int suppress, int max_models, int min_votes,
                         uint32_t* out, hipStream_t s);

// The projection kernels (bf_project.hip; include/bf_accel.h, "event groups: projection").  They share the assignment's window,
// warps (AssignArgs, its prior the held grouping: here an event's ONE model) and vote planes.
// V (K x R x C words, zero) += one vote per event on its own group's plane; out (ProjectBlock, zero) += events, inside,
// unassigned.
void launch_project_vote(const AssignArgs& a, uint32_t* V, unsigned long long* out, hipStream_t s);
// Per pixel N, the owner and its colour from the K planes B (the box sums, or V itself at scale 1); out += the rest.
void launch_project_compose(const uint32_t* B, int K, int R, int C, int gain, uint32_t* count, int32_t* label, uint8_t* bgr,
                            unsigned long long* out, hipStream_t s);

// The merge-gain kernels (bf_merge.hip; include/bf_accel.h, "event groups: merge gains").  The base planes B_k are the
// projection's (launch_project_vote, launch_assign_box); a pass holds the trial planes of `targets` target models, plane
// (a_local * K + b) the events of group b under model a0 + a_local.
// The result block is MergeBlock.
// A = min(K, targets_per_pass or K, floor(2^27 / (K R C))): the target models of one pass (K R C <= 2^27, so A >= 1).
inline int merge_targets_per_pass(int K, long long plane, int targets_per_pass) {
    long long A = kAssignMaxWords / ((long long)K * plane);
    if (A > K) A = K;
    if (targets_per_pass >= 1 && A > targets_per_pass) A = targets_per_pass;
    return (int)A;
}
// N = sum_k B_k, every word written; out (zero) += sum, sum_sq.
void launch_merge_total(const uint32_t* B, int K, int R, int C, uint32_t* N, unsigned long long* out, hipStream_t s);
// T (targets x K x R x C words, zero) += one vote per event with an id other than the target's on plane (a_local, id) under
// model a0 + a_local; out += inside[id][a0 + a_local].  The diagonal stays zero: it is the base pass's.
void launch_merge_vote(const AssignArgs& a, int a0, int targets, uint32_t* T, unsigned long long* out, hipStream_t s);
// out += gain[b][a0 + a_local] from the trial planes T (box-summed when scale > 1; plane b == a read from B), the base planes B
// and N.
void launch_merge_gain(const uint32_t* T, const uint32_t* B, const uint32_t* N, int K, int a0, int targets, int R, int C,
                       unsigned long long* out, hipStream_t s);

}  // namespace bf
