// test_object_tracker.cpp -- bf::ObjectTracker (host/better_flow/object_tracker.h) as a stand-alone program linked against
// libbf_accel.so: a stream of slices, every slice through next().
//
//   test_object_tracker <prefix> <K> <research_every> <step_ns> <res_x> <res_y> <events_0.txt> <events_1.txt> ...
//
// events_N.txt: "fr_x fr_y t_ns" per line, slice-local times; consecutive slices' time origins are step_ns apart.  The finder is
// configured as tests/cpp/test_object_finder.cpp configures it.  Before the stream, bf::ObjectFinder::find runs on slice 0 on
// contexts of its own: <prefix>find_gid.i32, find_models.bin, find_counts.i32.  Per slice N: <prefix>N_gid.i32, N_models.bin,
// N_counts.i32, N_overlap.i32, N_inside.i32 and N.txt: "searched <0|1> kept <Kp> dt_ns <dt>", one line "group track age events
// on_track" per group, and "ended <ids>".  <prefix>times.txt: the host wall clock of the find() and of every next(), in ms (each
// call ends synchronised: its results are on the host).
#include <better_flow/object_tracker.h>

#include "object_test_common.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    return std::fclose(f) == 0;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: test_object_tracker prefix K research_every step_ns res_x res_y events_0 [events_1 ...]\n");
        return 2;
    }
    const std::string prefix = argv[1];
    const int K = std::atoi(argv[2]), res_x = std::atoi(argv[5]), res_y = std::atoi(argv[6]);
    const long long step = std::atoll(argv[4]);
    std::vector<Events> slices((size_t)(argc - 7));
    size_t most = 0;
    for (int i = 7; i < argc; ++i) {
        if (!read_events(argv[i], slices[(size_t)(i - 7)])) return 2;
        most = std::max(most, slices[(size_t)(i - 7)].fx.size());
    }
    bf_ctx *ctx = nullptr, *helper = nullptr, *alone = nullptr;
    const int rows = 3 * res_x + 3, cols = 3 * res_y + 3;
    if (bf_create(0, (int64_t)most + 1, rows, cols, nullptr, &ctx) != BF_OK ||
        bf_create(0, (int64_t)most + 1, rows, cols, nullptr, &helper) != BF_OK ||
        bf_create(0, (int64_t)most + 1, rows, cols, nullptr, &alone) != BF_OK) {
        std::fprintf(stderr, "test_object_tracker: bf_create failed\n");
        return 1;
    }
    bool ok = true;
    FILE *times = std::fopen((prefix + "times.txt").c_str(), "w");
    if (!times) return 1;
    {   // the finder alone on slice 0
        bf::ObjectFinder of;
        configure(of, K, res_x, res_y);
        const Events &e = slices[0];
        of.refit.helper = helper;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = of.find(alone, e.slice());
        std::fprintf(times, "find slice 0: %.3f ms\n", ms_since(t0));
        if (rc != BF_OK) {
            std::fprintf(stderr, "test_object_tracker: find: %d: %s\n", rc, of.error.c_str());
            return 1;
        }
        ok = dump(prefix + "find_gid.i32", of.grouping.gid) && dump(prefix + "find_models.bin", of.grouping.models) && dump(prefix + "find_counts.i32", of.grouping.counts);
    }
    bf::ObjectTracker tr;
    configure(tr.finder, K, res_x, res_y);
    tr.finder.refit.helper = helper;
    tr.research_every = std::atoi(argv[3]);
    for (size_t n = 0; n < slices.size() && ok; ++n) {
        const Events &e = slices[n];
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = tr.next(ctx, e.slice(), n ? step : 0);
        std::fprintf(times, "next slice %zu (searched %d): %.3f ms\n", n, tr.searched ? 1 : 0, ms_since(t0));
        if (rc != BF_OK) {
            std::fprintf(stderr, "test_object_tracker: next (slice %zu): %d: %s\n", n, rc, tr.error.c_str());
            return 1;
        }
        const std::string base = prefix + std::to_string(n);
        ok = dump(base + "_gid.i32", tr.finder.grouping.gid) && dump(base + "_models.bin", tr.finder.grouping.models) &&
             dump(base + "_counts.i32", tr.finder.grouping.counts) && dump(base + "_overlap.i32", tr.overlap) && dump(base + "_inside.i32", tr.inside);
        FILE *f = std::fopen((base + ".txt").c_str(), "w");
        if (!f) return 1;
        std::fprintf(f, "searched %d kept %d dt_ns %lld\n", tr.searched ? 1 : 0, (int)tr.kept, (long long)tr.dt_ns);
        for (size_t k = 0; k < tr.tracks.size(); ++k)
            std::fprintf(f, "%zu %d %d %d %d\n", k, (int)tr.tracks[k].id, (int)tr.tracks[k].age, (int)tr.tracks[k].events, (int)tr.on_track[k]);
        std::fprintf(f, "ended");
        for (int32_t id : tr.ended) std::fprintf(f, " %d", (int)id);
        std::fprintf(f, "\n");
        ok = (std::fclose(f) == 0) && ok;
    }
    ok = (std::fclose(times) == 0) && ok;
    bf_destroy(alone);
    bf_destroy(helper);
    bf_destroy(ctx);
    return ok ? 0 : 1;
}
