// object_tracker.h -- bf::ObjectTracker: the moving objects of a STREAM of slices.  bf::ObjectFinder treats
// every slice as if nothing came before it: a full search per slice, and group k of one slice has no relation to group k of the
// next.  The tracker carries identities from slice to slice and starts a slice from the previous slice's models:
//   1. candidates: ObjectFinder::find (search, proposals) when it must -- no live track, `research_every` slices since the last
//      search, or the previous slice left more than research_unassigned_num / _den of its events unassigned -- and otherwise WARM:
//      the live tracks' models go straight into the alternation (ObjectFinder::group_from: no bf_global_set_window,
//      bf_global_search or bf_propose_models), then the merger when it is on: the same code after the candidates on both paths;
//   2. identity, by one rule on both paths: the final grouping is put on the context (upload, bf_set_groups), bf_track_overlap
//      counts its groups against the owner plane kept from the previous slice, the events carried back by dt_ns, and match()
//      decides from that table alone;
//   3. bf_track_keep keeps this slice's owner plane for the next one; with no group left bf_track_drop runs and every track ends;
//   4. (hold_flow) bf_hold_groups and the medians, as the finder's hold_flow leaves them, after the keep.
// It needs the device library, as the finder does; against a C-ABI without the track entries next() returns BF_ERR_STATE and
// `error` names bf_track_keep.
#ifndef BF_HOST_OBJECT_TRACKER_H
#define BF_HOST_OBJECT_TRACKER_H

#include <better_flow/object_finder.h>

#include <string>
#include <vector>

// (weak, as in object_finder.h)
extern "C" {
int bf_track_keep(bf_ctx *ctx, const bf_track_opts *opts, const bf_model *models, int32_t n_models, int32_t *plane_out,
                  bf_track_info *info) __attribute__((weak));
int bf_track_overlap(bf_ctx *ctx, const bf_track_opts *opts, const bf_model *models, int32_t n_models, int64_t dt_ns,
                     int32_t *overlap_out, int32_t *inside_out, bf_track_info *info) __attribute__((weak));
int bf_track_drop(bf_ctx *ctx) __attribute__((weak));
}

namespace bf {

class ObjectTracker {
  public:
    // The configuration of every slice's search, alternation and refit (finder.refit), whether the slice ends with its flow held
    // (finder.hold_flow), and what next() leaves of the slice: finder.grouping, flow_u / flow_v, records, steps.
    ObjectFinder finder;
    int research_every = 0;   // > 0: a search every that many slices; 0: only when it must
    int64_t research_unassigned_num = 1, research_unassigned_den = 2;   // ... or when the previous slice left more than this share unassigned
    // A group continues the track that holds at least match_num / match_den of its inside events.  1/2 rests on ONE scene
    // (tests/track_scene.py): there the right track holds at least 0.83 of a group's inside events and the
    // wrong one at most 0.034; no other scene has been looked at.
    uint64_t match_num = 1, match_den = 2;

    struct Track {
        int32_t id;
        bf_model model;
        int32_t age;      // slices this track has been matched after the one it started in
        int32_t events;
    };
    std::vector<Track> tracks;           // the live tracks: tracks[k] is group k of the last slice
    std::vector<int32_t> ended;          // the ids that ended with the last slice
    std::vector<int32_t> overlap;        // the last slice's table, K x (kept + 1); empty when no plane was kept
    std::vector<int32_t> inside;         // ... and its row sums (K; empty likewise)
    std::vector<int32_t> on_track;       // per group: overlap[k][the kept group it continues], 0 for a new track
    int32_t kept = 0;                    // the groups of the plane the last slice was counted against
    bool searched = false;               // the path the last slice took
    int64_t dt_ns = 0;
    int32_t next_id = 0;
    std::string error;

    // The entry the linked C-ABI lacks, or null.
    static const char *missing_entry(bool merging = false, bool holding = false) {
        if (const char *m = ObjectFinder::missing_entry(merging, holding)) return m;
        if (!bf_track_keep || !bf_track_overlap || !bf_track_drop || !bf_set_groups) return "bf_track_keep";
        return nullptr;
    }

    // Which kept group every group continues, -1 for none: repeatedly the largest overlap[k][j] among unmatched k and j (ties:
    // the smallest k, then the smallest j), accepted while it is > 0 and overlap[k][j] * den >= inside[k] * num; the first one
    // refused ends the matching.  overlap: K x (Kp + 1), the last column (a pixel nobody owned) is not a track.
    static std::vector<int32_t> match(const std::vector<int32_t> &overlap, const std::vector<int32_t> &inside, int K, int Kp,
                                      uint64_t num, uint64_t den) {
        std::vector<int32_t> out((size_t)K, -1);
        std::vector<char> taken((size_t)Kp, 0);
        for (;;) {
            long long best = -1;
            int bk = -1, bj = -1;
            for (int k = 0; k < K; ++k) {
                if (out[(size_t)k] >= 0) continue;
                for (int j = 0; j < Kp; ++j) {
                    if (taken[(size_t)j]) continue;
                    const long long v = overlap[(size_t)k * (size_t)(Kp + 1) + (size_t)j];
                    if (v > best) { best = v; bk = k; bj = j; }   // (strictly larger: ties stay with the smaller k, then j)
                }
            }
            if (bk < 0) break;
            if (!(best > 0 && (uint64_t)best * den >= (uint64_t)inside[(size_t)bk] * num)) break;
            out[(size_t)bk] = bj;
            taken[(size_t)bj] = 1;
        }
        return out;
    }

    // Forget every track and the kept plane: the next slice starts a stream.
    int reset(bf_ctx *ctx) {
        tracks.clear(); ended.clear(); overlap.clear(); inside.clear(); on_track.clear();
        kept = 0; since_search = 0; last_events = last_unassigned = 0; have_plane = false;
        return bf_track_drop ? bf_track_drop(ctx) : BF_OK;
    }

    // dt: this slice's time origin minus the previous slice's, in ns (not read for the first slice of a stream).
    int next(bf_ctx *ctx, const Slice &s, int64_t dt) {
        error.clear();
        ended.clear(); overlap.clear(); inside.clear(); on_track.clear();
        dt_ns = dt;
        const bool merging = finder.merge_num > 0, holding = finder.hold_flow;
        if (const char *m = missing_entry(merging, holding)) {
            error = std::string("bf::ObjectTracker: the linked library has no ") + m;
            return BF_ERR_STATE;
        }
        searched = tracks.empty() || (research_every > 0 && since_search >= research_every) ||
                   last_unassigned * research_unassigned_den > last_events * research_unassigned_num;
        std::vector<bf_model> warm;
        for (const Track &t : tracks) warm.push_back(t.model);
        int rc = searched ? finder.group(ctx, s) : finder.group_from(ctx, s, warm);
        since_search = searched ? 1 : since_search + 1;
        if (rc >= 0 && !holding) rc = finder.flows(ctx, s);   // (holding: after the keep, which needs the slice uploaded again)
        if (rc < 0) { error = finder.error; return rc; }
        const Grouping &g = finder.grouping;
        last_events = (int64_t)s.n;
        last_unassigned = g.counts.empty() ? 0 : (int64_t)g.counts.back();
        const int32_t K = (int32_t)g.models.size();
        std::vector<Track> before;
        before.swap(tracks);
        kept = have_plane ? (int32_t)before.size() : 0;
        if (K == 0) {   // no group left: nothing to keep, every track ends
            for (const Track &t : before) ended.push_back(t.id);
            have_plane = false;
            rc = bf_track_drop(ctx);
            return rc < 0 ? ObjectFinder::fail(ctx, rc, error) : BF_OK;
        }
        bf_track_opts o = bf_track_opts();
        o.scale = finder.assign.scale;
        o.sensor_res_x = finder.assign.sensor_res_x; o.sensor_res_y = finder.assign.sensor_res_y;
        o.margin = finder.assign.margin;
        // the final grouping on the context, under the held flow's window when a flow is going to be held
        rc = hold_grouping(ctx, s, g.gid, g.models.size(), holding ? finder.search_scale : 0, finder.search_wsize);
        std::vector<int32_t> continues((size_t)K, -1);
        if (rc >= 0 && have_plane) {
            overlap.assign((size_t)K * (size_t)(kept + 1), 0);
            inside.assign((size_t)K, 0);
            rc = bf_track_overlap(ctx, &o, g.models.data(), K, dt, overlap.data(), inside.data(), nullptr);
            if (rc >= 0) continues = match(overlap, inside, K, kept, match_num, match_den);
        }
        if (rc >= 0) rc = bf_track_keep(ctx, &o, g.models.data(), K, nullptr, nullptr);
        if (rc < 0) { have_plane = false; return ObjectFinder::fail(ctx, rc, error); }
        have_plane = true;
        std::vector<char> continued(before.size(), 0);
        on_track.assign((size_t)K, 0);
        for (int32_t k = 0; k < K; ++k) {
            Track t;
            const int32_t j = continues[(size_t)k];
            if (j >= 0) {
                t.id = before[(size_t)j].id;
                t.age = before[(size_t)j].age + 1;
                continued[(size_t)j] = 1;
                on_track[(size_t)k] = overlap[(size_t)k * (size_t)(kept + 1) + (size_t)j];
            } else {
                t.id = next_id++;
                t.age = 0;
            }
            t.model = g.models[(size_t)k];
            t.events = g.counts[(size_t)k];
            tracks.push_back(t);
        }
        for (size_t j = 0; j < before.size(); ++j)
            if (!continued[j]) ended.push_back(before[j].id);
        if (holding) {
            rc = finder.held_flows(ctx);
            if (rc < 0) return ObjectFinder::fail(ctx, rc, error);
        }
        return BF_OK;
    }

    // objects_N.tracks.txt: the path the slice took, then per group its track, the track's age, its events, those inside under
    // its model carried back by dt and those of them on its own track's pixels, then the tracks that ended.
    bool write_tracks(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        std::fprintf(f, "searched %d dt_ns %lld\n", searched ? 1 : 0, (long long)dt_ns);
        for (size_t k = 0; k < tracks.size(); ++k)
            std::fprintf(f, "%zu %d %d %d %d %d\n", k, (int)tracks[k].id, (int)tracks[k].age, (int)tracks[k].events,
                         inside.empty() ? 0 : (int)inside[k], (int)on_track[k]);
        std::fprintf(f, "ended");
        for (int32_t id : ended) std::fprintf(f, " %d", (int)id);
        std::fprintf(f, "\n");
        return std::fclose(f) == 0;
    }

  private:
    int since_search = 0;
    int64_t last_events = 0, last_unassigned = 0;
    bool have_plane = false;
};

}  // namespace bf

#endif  // BF_HOST_OBJECT_TRACKER_H
