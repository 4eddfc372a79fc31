// test_object_finder.cpp -- bf::ObjectFinder (host/better_flow/object_finder.h) as a stand-alone program linked against
// libbf_accel.so: search, proposals, alternation on one slice.
//
//   test_object_finder <events.txt> <K> <res_x> <res_y> <guard_x> <guard_y> <min_events> <hard_cap> <prefix>
//
// events.txt: "fr_x fr_y t_ns" per line.  The search runs at scale 1 with a 5-pixel window over the lattice -0.72 .. 0.72 in
// steps of 0.04 on both axes, the proposal with radius 1 and suppress 2, the alternation at scale 3 with two rounds per fit and
// at most five alternations.  Writes <prefix>gid.i32, models.bin, proposals.bin, flows.f64 (u then v per group) and
// records.i32 (per alternation: changed, counts[K + 1], iterations[K], -1: no refit).
#include <better_flow/object_finder.h>

#include <cstdio>
#include <cstdlib>

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    return std::fclose(f) == 0;
}

int main(int argc, char **argv) {
    if (argc != 10) {
        std::fprintf(stderr, "usage: test_object_finder events K res_x res_y guard_x guard_y min_events hard_cap prefix\n");
        return 2;
    }
    std::vector<int32_t> fx, fy, t;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char line[256];
    while (std::fgets(line, sizeof(line), f)) {
        long a, b, c;
        if (std::sscanf(line, "%ld %ld %ld", &a, &b, &c) != 3) continue;
        fx.push_back((int32_t)a); fy.push_back((int32_t)b); t.push_back((int32_t)c);
    }
    std::fclose(f);
    bf::ObjectFinder of;
    of.lattice.x_low = of.lattice.y_low = -0.72;
    of.lattice.x_hi = of.lattice.y_hi = 0.72;
    of.lattice.x_step = of.lattice.y_step = 0.04;
    of.propose.max_models = std::atoi(argv[2]);
    of.assign.sensor_res_x = of.refit.fit.sensor_res_x = std::atoi(argv[3]);
    of.assign.sensor_res_y = of.refit.fit.sensor_res_y = std::atoi(argv[4]);
    of.refit.fit.guard_res_x = std::atoi(argv[5]); of.refit.fit.guard_res_y = std::atoi(argv[6]);
    of.refit.fit.min_events = std::atoi(argv[7]);
    of.refit.fit.hard_iter_cap = std::atoi(argv[8]);
    const std::string prefix = argv[9];
    bf_ctx *ctx = nullptr, *helper = nullptr;
    const int rows = 3 * of.refit.fit.sensor_res_x + 3, cols = 3 * of.refit.fit.sensor_res_y + 3;
    if (bf_create(0, (int64_t)fx.size() + 1, rows, cols, nullptr, &ctx) != BF_OK ||
        bf_create(0, (int64_t)fx.size() + 1, rows, cols, nullptr, &helper) != BF_OK) {
        std::fprintf(stderr, "test_object_finder: bf_create failed\n");
        return 1;
    }
    const bf::Slice sl = {fx.data(), fy.data(), t.data(), fx.size()};
    of.refit.helper = helper;
    const int rc = of.find(ctx, sl);
    if (rc != BF_OK) {
        std::fprintf(stderr, "test_object_finder: find: %d: %s\n", rc, of.error.c_str());
        return 1;
    }
    const size_t K = of.grouping.models.size();
    std::vector<int32_t> rec;
    for (const bf::MotionAssigner::Record &r : of.records) {
        rec.push_back(r.changed);
        rec.insert(rec.end(), r.counts.begin(), r.counts.end());
        for (size_t k = 0; k < K; ++k) rec.push_back(r.iterations.empty() ? -1 : r.iterations[k]);
    }
    std::vector<double> flows(of.flow_u);
    flows.insert(flows.end(), of.flow_v.begin(), of.flow_v.end());
    const bool ok = dump(prefix + "gid.i32", of.grouping.gid) && dump(prefix + "models.bin", of.grouping.models) &&
                    dump(prefix + "proposals.bin", of.proposals) && dump(prefix + "flows.f64", flows) && dump(prefix + "records.i32", rec);
    bf_destroy(helper);
    bf_destroy(ctx);
    return ok ? 0 : 1;
}
