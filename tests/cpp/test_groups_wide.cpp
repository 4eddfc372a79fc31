// test_groups_wide.cpp -- the host classes with wide groups (bf::Refit::wide, held by every class that refits) as a
// stand-alone program linked against libbf_accel.so: everything is run two ways -- wide = true with helper = nullptr, and
// wide = false with a helper context -- and must leave the same bytes.
//
//   test_groups_wide <prefix> <models.bin> <K> <step_ns> <res_x> <res_y> <events_0.txt> [<events_1.txt> ...]
//
// events_N.txt: "fr_x fr_y t_ns" per line, slice-local times; models.bin: the bf_model structs bf::MotionAssigner::alternate
// starts from on slice 0.  Three comparisons, each "<name> same|DIFFERENT" on stdout: `alternate` (ids, models, counts and the
// records' changed, counts and iterations), `find` (bf::ObjectFinder::find on slice 0: ids, models, counts, records, flows) and
// `track` (bf::ObjectTracker::next over every slice: those of its finder, the tracks, the overlap table).  <prefix>times.txt:
// host wall clock of every call in ms, both ways (each call ends synchronised).  Exit 0 when all three are the same.
#include <better_flow/object_tracker.h>

#include "object_test_common.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: test_groups_wide prefix models.bin K step_ns res_x res_y events_0 [events_1 ...]\n");
        return 2;
    }
    const std::string prefix = argv[1];
    const int K = std::atoi(argv[3]), res_x = std::atoi(argv[5]), res_y = std::atoi(argv[6]);
    const long long step = std::atoll(argv[4]);
    std::vector<bf_model> start;
    if (FILE *f = std::fopen(argv[2], "rb")) {
        bf_model m;
        while (std::fread(&m, sizeof(m), 1, f) == 1) start.push_back(m);
        std::fclose(f);
    }
    if (start.empty()) return 2;
    std::vector<Events> slices((size_t)(argc - 7));
    size_t most = 0;
    for (int i = 7; i < argc; ++i) {
        if (!read_events(argv[i], slices[(size_t)(i - 7)])) return 2;
        most = std::max(most, slices[(size_t)(i - 7)].fx.size());
    }
    FILE *times = std::fopen((prefix + "times.txt").c_str(), "w");
    if (!times) return 1;
    const int rows = 3 * res_x + 3, cols = 3 * res_y + 3;
    std::string got[2][3];
    for (int way = 0; way < 2; ++way) {   // 0: wide groups, no helper; 1: the helper context
        const bool wide = way == 0;
        const char *name = wide ? "wide" : "helper";
        bf_ctx *ctx = nullptr, *helper = nullptr;
        if (bf_create(0, (int64_t)most + 1, rows, cols, nullptr, &ctx) != BF_OK ||
            (!wide && bf_create(0, (int64_t)most + 1, rows, cols, nullptr, &helper) != BF_OK)) {
            std::fprintf(stderr, "test_groups_wide: bf_create failed\n");
            return 1;
        }
        const Events &e0 = slices[0];
        const bf::Slice s0 = e0.slice();
        {   // the alternation from the given models
            bf::ObjectFinder cfg;
            configure(cfg, K, res_x, res_y);
            cfg.refit.wide = wide;
            cfg.refit.helper = helper;
            bf::MotionAssigner ma;
            ma.refit = cfg.refit;
            bf::Grouping g;
            for (int rep = 0; rep < 2; ++rep) {   // (the second is the warm figure: the first also loads the kernels)
                const auto t0 = std::chrono::steady_clock::now();
                g = bf::Grouping(start, s0.n);
                const int rc = ma.alternate(ctx, s0, g, cfg.assign, cfg.rounds_per_fit, cfg.max_alternations);
                std::fprintf(times, "%s alternate (run %d, %zu alternations): %.3f ms\n", name, rep, ma.records.size(), ms_since(t0));
                if (rc != BF_OK) {
                    std::fprintf(stderr, "test_groups_wide: %s alternate: %d: %s\n", name, rc, bf_last_error(ctx));
                    return 1;
                }
            }
            Bytes b;
            b.add(g.gid); b.add(g.models); b.add(g.counts); b.add(ma.records);
            got[way][0] = b.s;
        }
        {   // the finder on slice 0
            bf::ObjectFinder of;
            configure(of, K, res_x, res_y);
            of.refit.wide = wide;
            of.refit.helper = helper;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = of.find(ctx, s0);
            std::fprintf(times, "%s find slice 0: %.3f ms\n", name, ms_since(t0));
            if (rc != BF_OK) {
                std::fprintf(stderr, "test_groups_wide: %s find: %d: %s\n", name, rc, of.error.c_str());
                return 1;
            }
            Bytes b;
            b.add(of.grouping.gid); b.add(of.grouping.models); b.add(of.grouping.counts); b.add(of.records); b.add(of.flow_u); b.add(of.flow_v); b.add(of.grouping.origin);
            got[way][1] = b.s;
        }
        {   // the tracker over the slices
            bf::ObjectTracker tr;
            configure(tr.finder, K, res_x, res_y);
            tr.finder.refit.wide = wide;
            tr.finder.refit.helper = helper;
            Bytes b;
            for (size_t n = 0; n < slices.size(); ++n) {
                const Events &e = slices[n];
                const auto t0 = std::chrono::steady_clock::now();
                const int rc = tr.next(ctx, e.slice(), n ? step : 0);
                std::fprintf(times, "%s next slice %zu (searched %d): %.3f ms\n", name, n, tr.searched ? 1 : 0, ms_since(t0));
                if (rc != BF_OK) {
                    std::fprintf(stderr, "test_groups_wide: %s next (slice %zu): %d: %s\n", name, n, rc, tr.error.c_str());
                    return 1;
                }
                b.add(tr.finder.grouping.gid); b.add(tr.finder.grouping.models); b.add(tr.finder.grouping.counts); b.add(tr.finder.records);
                b.add(tr.overlap); b.add(tr.inside); b.add(tr.on_track); b.add(tr.ended);
                b.add((int64_t)tr.searched); b.add((int64_t)tr.kept);
                for (const bf::ObjectTracker::Track &t : tr.tracks) { b.add((int64_t)t.id); b.add((int64_t)t.age); b.add((int64_t)t.events); }
            }
            got[way][2] = b.s;
        }
        int64_t persistent = -1;   // would the context's own warm runs take the persistent form now?
        (void)bf_upload_events(ctx, e0.fx.data(), e0.fy.data(), e0.t.data(), nullptr, (int64_t)e0.fx.size());
        (void)bf_set_cloud(ctx, 3, res_x, res_y, nullptr);
        (void)bf_set_model(ctx, &start[0]);
        (void)bf_get_stat(ctx, "persistent", &persistent);
        std::fprintf(times, "%s persistent form for a warm run of the main context: %lld\n", name, (long long)persistent);
        if (helper) bf_destroy(helper);
        bf_destroy(ctx);
    }
    std::fclose(times);
    const char *names[3] = {"alternate", "find", "track"};
    bool same = true;
    for (int k = 0; k < 3; ++k) {
        const bool eq = !got[0][k].empty() && got[0][k] == got[1][k];
        std::printf("%s %s (%zu bytes)\n", names[k], eq ? "same" : "DIFFERENT", got[0][k].size());
        same = same && eq;
    }
    return same ? 0 : 1;
}
