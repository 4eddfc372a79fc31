// test_object_merge.cpp -- bf::ObjectMerger (host/better_flow/object_merge.h) as a stand-alone program, linked either against
// the CPU stand-in of the C-ABI (tests/shim + the oracle: scores_host, also under ASan / UBSan) or against libbf_accel.so
// (bf_merge_scores), and bf::ObjectFinder with merging on (libbf_accel.so only).
//
//   test_object_merge scores <events.txt> <ids.i32> <models.bin> <K> <scale> <res_x> <res_y> <margin> <prefix>
//       events.txt: "fr_x fr_y t_ns" per line (may be empty).  ids.i32: one group id per event.  models.bin: K bf_model records.
//       Writes <prefix>gain.u64 (K x K), <prefix>inside.i32 (K x K), <prefix>events.i32 (K), <prefix>info.bin; prints
//       "path device|host".
//   test_object_merge pick <cases.txt>
//       cases.txt, per case: "K num den", K event counts, K x K gains (decimal, row b column a).  Prints per case
//       "found accepted b a".
//   test_object_merge find <events.txt> <K> <res_x> <res_y> <guard_x> <guard_y> <min_events> <hard_cap> <num> <den>
//                          <dissolve_below> <prefix>
//       bf::ObjectFinder as in test_object_finder.cpp, with merge_num / merge_den / dissolve_below.  Writes <prefix>gid.i32,
//       models.bin, origin.i32, counts.i32 and, through the writer, <prefix>steps.txt.
#include <better_flow/object_finder.h>
#include <better_flow/object_merge.h>

#include "object_test_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int die(const char *what, bf_ctx *ctx) {
    std::fprintf(stderr, "test_object_merge: %s: %s\n", what, ctx ? bf_last_error(ctx) : "");
    return 1;
}

template <class T>
static bool dump(const std::string &path, const T *v, size_t n) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (n) std::fwrite(v, sizeof(T), n, f);
    return std::fclose(f) == 0;
}

static int run_scores(char **argv) {
    const int K = std::atoi(argv[5]);
    if (K < 1) return die("bad model count", nullptr);
    Events e;
    if (!read_events(argv[2], e)) return die("cannot read the events", nullptr);
    const std::vector<int32_t> &fx = e.fx;
    std::vector<int32_t> ids(fx.size());
    std::vector<bf_model> models((size_t)K);
    FILE *f = std::fopen(argv[3], "rb");
    if (!f) return die("cannot read the ids", nullptr);
    const size_t got = ids.empty() ? 0 : std::fread(ids.data(), sizeof(int32_t), ids.size(), f);
    std::fclose(f);
    if (got != ids.size()) return die("short ids file", nullptr);
    f = std::fopen(argv[4], "rb");
    if (!f) return die("cannot read the models", nullptr);
    const size_t gm = std::fread(models.data(), sizeof(bf_model), (size_t)K, f);
    std::fclose(f);
    if (gm != (size_t)K) return die("short models file", nullptr);
    bf::ObjectMerger m;
    m.opts.scale = std::atoi(argv[6]);
    m.opts.sensor_res_x = std::atoi(argv[7]); m.opts.sensor_res_y = std::atoi(argv[8]);
    m.opts.margin = std::atoi(argv[9]);
    const std::string prefix = argv[10];
    bf_ctx *ctx = nullptr;
    const int s = m.opts.scale;
    if (bf_create(0, (int64_t)fx.size() + 1, s * m.opts.sensor_res_x + s, s * m.opts.sensor_res_y + s, nullptr, &ctx) != BF_OK)
        return die("bf_create", nullptr);
    const bool device = bf::ObjectMerger::device_available() && bf_set_groups;
    std::printf("path %s\n", device ? "device" : "host");
    const bf::Slice sl = e.slice();
    // refused: an id outside -1 .. K-1 (host path), a negative targets_per_pass (either path)
    if (!ids.empty()) {
        std::vector<int32_t> bad(ids);
        bad[0] = K;
        if (m.scores_host(ctx, sl, bad, models) != BF_ERR_ARG) return die("an id beyond the groups was not refused", nullptr);
    }
    m.opts.targets_per_pass = -1;
    if (m.scores_host(ctx, sl, ids, models) != BF_ERR_ARG) return die("a negative targets_per_pass was not refused", nullptr);
    m.opts.targets_per_pass = 0;
    int rc;
    if (device) {
        rc = bf::hold_grouping(ctx, sl, ids, K);
        if (rc >= 0) rc = m.scores(ctx, models);
    } else {
        rc = m.scores_host(ctx, sl, ids, models);
    }
    if (rc != BF_OK) return die("scores", ctx);
    if (!dump(prefix + "gain.u64", m.gain.data(), m.gain.size()) || !dump(prefix + "inside.i32", m.inside.data(), m.inside.size()) ||
        !dump(prefix + "events.i32", m.events.data(), m.events.size()) || !dump(prefix + "info.bin", &m.info, 1))
        return die("cannot write the outputs", nullptr);
    bf_destroy(ctx);
    return 0;
}

static int run_pick(char **argv) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) return die("cannot read the cases", nullptr);
    unsigned long long K, num, den;
    while (std::fscanf(f, "%llu %llu %llu", &K, &num, &den) == 3) {
        std::vector<int32_t> events((size_t)K);
        std::vector<uint64_t> gain((size_t)(K * K));
        for (size_t k = 0; k < K; ++k) {
            long e;
            if (std::fscanf(f, "%ld", &e) != 1) return die("short case", nullptr);
            events[k] = (int32_t)e;
        }
        for (size_t w = 0; w < K * K; ++w) {
            unsigned long long g;
            if (std::fscanf(f, "%llu", &g) != 1) return die("short case", nullptr);
            gain[w] = g;
        }
        const bf::ObjectMerger::Pick p = bf::ObjectMerger::pick(gain, events, num, den);
        std::printf("%d %d %d %d\n", p.found ? 1 : 0, p.accepted ? 1 : 0, (int)p.b, (int)p.a);
    }
    std::fclose(f);
    return 0;
}

static int run_find(char **argv) {
    Events e;
    if (!read_events(argv[2], e)) return die("cannot read the events", nullptr);
    const std::vector<int32_t> &fx = e.fx;
    bf::ObjectFinder of;
    configure(of, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8]),
              std::atoi(argv[9]));
    of.merge_num = std::strtoull(argv[10], nullptr, 10);
    of.merge_den = std::strtoull(argv[11], nullptr, 10);
    of.dissolve_below = std::atoi(argv[12]);
    const std::string prefix = argv[13];
    bf_ctx *ctx = nullptr, *helper = nullptr;
    const int rows = 3 * of.refit.fit.sensor_res_x + 3, cols = 3 * of.refit.fit.sensor_res_y + 3;
    if (bf_create(0, (int64_t)fx.size() + 1, rows, cols, nullptr, &ctx) != BF_OK ||
        bf_create(0, (int64_t)fx.size() + 1, rows, cols, nullptr, &helper) != BF_OK)
        return die("bf_create", nullptr);
    of.refit.helper = helper;
    const int rc = of.find(ctx, e.slice());
    if (rc != BF_OK) {
        std::fprintf(stderr, "test_object_merge: find: %d: %s\n", rc, of.error.c_str());
        return 1;
    }
    const bf::Grouping &g = of.grouping;
    const bool ok = dump(prefix + "gid.i32", g.gid.data(), g.gid.size()) && dump(prefix + "models.bin", g.models.data(), g.models.size()) &&
                    dump(prefix + "origin.i32", g.origin.data(), g.origin.size()) &&
                    dump(prefix + "counts.i32", g.counts.data(), g.counts.size()) &&
                    bf::ObjectMerger::write_steps(prefix + "steps.txt", of.steps, g.models.size(), of.merged_sum_sq);
    bf_destroy(helper);
    bf_destroy(ctx);
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 11 && !std::strcmp(argv[1], "scores")) return run_scores(argv);
    if (argc == 3 && !std::strcmp(argv[1], "pick")) return run_pick(argv);
    if (argc == 14 && !std::strcmp(argv[1], "find")) return run_find(argv);
    std::fprintf(stderr, "usage: test_object_merge scores events ids models K scale res_x res_y margin prefix\n"
                         "       test_object_merge pick cases\n"
                         "       test_object_merge find events K res_x res_y guard_x guard_y min_events hard_cap num den dissolve_below prefix\n");
    return 2;
}
