// test_motion_assign.cpp -- bf::MotionAssigner (host/better_flow/motion_assign.h) as a stand-alone program, linked either against
// the CPU stand-in of the C-ABI (tests/shim + the oracle: the host paths, also under ASan / UBSan) or against libbf_accel.so
// (the device paths).
//
//   test_motion_assign <events.txt> <models.bin> <K> <scale> <res_x> <res_y> <margin> <min_score> <guard_x> <guard_y>
//                      <min_events> <hard_cap> <rounds_per_fit> <max_alternations> <prefix>
//
// events.txt: "fr_x fr_y t_ns" per line.  models.bin: K bf_model records, the candidates.  Writes
//   <prefix>first.i32, <prefix>second.i32   one assignment without a prior, then one with the first as its prior: gid[n],
//                                           score[n], counts[K + 1], then the eight words of bf_assign_info
//   <prefix>models.bin, <prefix>gid.i32     what alternate() leaves
//   <prefix>records.i32                     per alternation: changed, counts[K + 1], iterations[K] (-1: no refit)
// and prints "path device|host".
#include <better_flow/motion_assign.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int die(const char *what, bf_ctx *ctx) {
    std::fprintf(stderr, "test_motion_assign: %s: %s\n", what, ctx ? bf_last_error(ctx) : "");
    return 1;
}

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    return std::fclose(f) == 0;
}

static std::vector<int32_t> flat(const bf::MotionAssigner &m) {
    std::vector<int32_t> out(m.gid);
    out.insert(out.end(), m.score.begin(), m.score.end());
    out.insert(out.end(), m.counts.begin(), m.counts.end());
    const int32_t i[8] = {m.info.models, m.info.rows, m.info.cols, m.info.assigned, m.info.unassigned, m.info.changed,
                          m.info.max_score, m.info.reserved};
    out.insert(out.end(), i, i + 8);
    return out;
}

int main(int argc, char **argv) {
    if (argc != 16) {
        std::fprintf(stderr, "usage: test_motion_assign events models K scale res_x res_y margin min_score guard_x guard_y min_events "
                             "hard_cap rounds_per_fit max_alternations prefix\n");
        return 2;
    }
    const int K = std::atoi(argv[3]);
    if (K < 1) return die("bad model count", nullptr);
    std::vector<int32_t> fx, fy, t;
    {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) return die("cannot read the events", nullptr);
        char line[256];
        while (std::fgets(line, sizeof(line), f)) {
            long a, b, c;
            if (std::sscanf(line, "%ld %ld %ld", &a, &b, &c) != 3) continue;
            fx.push_back((int32_t)a); fy.push_back((int32_t)b); t.push_back((int32_t)c);
        }
        std::fclose(f);
    }
    std::vector<bf_model> cand((size_t)K);
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) return die("cannot read the models", nullptr);
        const size_t got = std::fread(cand.data(), sizeof(bf_model), (size_t)K, f);
        std::fclose(f);
        if (got != (size_t)K) return die("short models file", nullptr);
    }
    bf_assign_opts o;
    std::memset(&o, 0, sizeof(o));
    o.scale = std::atoi(argv[4]);
    o.sensor_res_x = std::atoi(argv[5]); o.sensor_res_y = std::atoi(argv[6]);
    o.margin = std::atoi(argv[7]);
    o.min_score = std::atoi(argv[8]);
    bf::MotionAssigner ma;
    ma.refit.fit.scale = o.scale;
    ma.refit.fit.sensor_res_x = o.sensor_res_x; ma.refit.fit.sensor_res_y = o.sensor_res_y;
    ma.refit.fit.guard_res_x = std::atoi(argv[9]); ma.refit.fit.guard_res_y = std::atoi(argv[10]);
    ma.refit.fit.min_events = std::atoi(argv[11]);
    ma.refit.fit.hard_iter_cap = std::atoi(argv[12]);
    const int rounds = std::atoi(argv[13]), max_alt = std::atoi(argv[14]);
    const std::string prefix = argv[15];

    bf_ctx *ctx = nullptr, *helper = nullptr;
    const int s = o.scale;
    if (bf_create(0, (int64_t)fx.size() + 1, s * o.sensor_res_x + s, s * o.sensor_res_y + s, nullptr, &ctx) != BF_OK ||
        bf_create(0, (int64_t)fx.size() + 1, s * o.sensor_res_x + s, s * o.sensor_res_y + s, nullptr, &helper) != BF_OK)
        return die("bf_create", nullptr);
    const bf::Slice sl = {fx.data(), fy.data(), t.data(), fx.size()};
    std::printf("path %s\n", bf::MotionAssigner::device_available() ? "device" : "host");

    // a round with a prior before any grouping is held is refused on either path
    if (ma.upload(ctx, sl) != BF_OK) return die("upload", ctx);
    o.use_prior = 1;
    if (ma.assign(ctx, cand, o) != BF_ERR_STATE) return die("a prior that is not held was not refused", nullptr);
    o.use_prior = 0; o.install = 1;
    if (ma.assign(ctx, cand, o) != BF_OK) return die("assign", ctx);
    if (!dump(prefix + "first.i32", flat(ma))) return die("cannot write the outputs", nullptr);
    o.use_prior = 1;
    if (ma.assign(ctx, cand, o) != BF_OK) return die("assign with a prior", ctx);
    if (!dump(prefix + "second.i32", flat(ma))) return die("cannot write the outputs", nullptr);

    ma.refit.helper = helper;
    bf::Grouping g(cand, sl.n);
    if (ma.alternate(ctx, sl, g, o, rounds, max_alt) != BF_OK) return die("alternate", ctx);
    std::vector<int32_t> rec;
    for (const bf::MotionAssigner::Record &r : ma.records) {
        rec.push_back(r.changed);
        rec.insert(rec.end(), r.counts.begin(), r.counts.end());
        for (int k = 0; k < K; ++k) rec.push_back(r.iterations.empty() ? -1 : r.iterations[(size_t)k]);
    }
    if (!dump(prefix + "models.bin", g.models) || !dump(prefix + "gid.i32", g.gid) || !dump(prefix + "records.i32", rec))
        return die("cannot write the outputs", nullptr);
    bf_destroy(helper);
    bf_destroy(ctx);
    return 0;
}
