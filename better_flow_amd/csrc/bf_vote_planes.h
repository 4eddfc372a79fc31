// bf_vote_planes.h -- what the entries on the K models' vote planes share on the host, defined in bf_assign_abi.cpp and used by
// it, by bf_track_abi.cpp and by bf_hold_groups (bf_global_search.cpp): the checks, the staging of the K warps, the
// projection's base pass and the decode of its shared words.  Their scratch is bf_ctx::vote.
#pragma once
#include "bf_ctx.h"

using VoteWindow = bf_ctx::VoteScratch::Window;

// The K-model vote planes of one call: the kernels' arguments, and the R x C window with its words per plane.
struct VotePlanes {
    AssignArgs a;
    int R, C;
    size_t plane;
};

// K models for the held grouping, in this order: n_models in 1 .. 64, no noise mask, and -- unless `prior` is null: the held
// grouping is not read -- a grouping is held and its K is n_models.  `who`: the entry point's name; `prior`: what the message
// says before "no grouping ... is held".
int held_grouping_check(bf_ctx* c, const char* who, int n_models, const char* prior);
// The first checks of an entry on the vote planes after those of its pointers: scale and the sensor's size.  Next the entry
// itself checks the margin (vote_margin_ok) together with its own option, in one message, then vote_planes_check.
int vote_window_check(bf_ctx* c, const VoteWindow& w);
inline bool vote_margin_ok(int margin) { return margin >= 0 && margin <= 65536; }
// The rest, in their order: held_grouping_check, then the window of the widened sensor and the capacity check.  Fills
// everything of vp but a's pointers.
int vote_planes_check(bf_ctx* c, const char* who, const VoteWindow& w, int n_models, const char* prior, VotePlanes& vp);
// The window alone, of options that have passed these checks (bf_track_overlap: the kept plane's): everything of vp but a's
// pointers, a.K = K.
void vote_planes_window(const bf_ctx* c, const VoteWindow& w, int K, VotePlanes& vp);

// (the device set) The K warps staged -- the arrays grown, set_model_warp per model, the copy enqueued -- and a's pointers: the
// events as stored, the staged warps, and the held grouping as the prior when `prior`.
int vote_warps_stage(bf_ctx* c, const bf_model* models, int K, bool prior, AssignArgs& a);
// (n > 0, the device set) vote_warps_stage, and the vote planes grown and V cleared, the box planes grown when they are used.
int vote_planes_stage(bf_ctx* c, const bf_model* models, bool prior, VotePlanes& vp);
// The planes the second kernel of an entry reads: the box sums, or V itself at scale 1.
const uint32_t* vote_planes_summed(bf_ctx* c, const VotePlanes& vp);

// (n > 0, the device set) The projection's base pass on the held grouping: vote_planes_stage, the result block cleared, the vote,
// the box sum when scale > 1, and -- unless `label` is null -- the compose under `gain` with the owner plane into `label` (R x C
// words of the caller's; N and the colour into the projection's scratch, grown here).  The copy of the block to the host is
// enqueued: project_base_decode after the stream has been waited for.  The base planes are vote_planes_summed.
int project_base_pass(bf_ctx* c, const bf_model* models, VotePlanes& vp, int gain, int32_t* label);
// The block's words every caller of the base pass reports.
struct ProjectBase {
    int32_t events[kAssignMaxModels], inside[kAssignMaxModels];   // per group: its events, and those inside the window
    int32_t unassigned, outside;                                  // outside: sum over the groups of events - inside
};
ProjectBase project_base_decode(const bf_ctx* c, int K);
