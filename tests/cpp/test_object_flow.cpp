// test_object_flow.cpp -- bf::ObjectFinder with hold_flow (host/better_flow/object_finder.h) as a stand-alone program linked
// against libbf_accel.so: the same slice found twice, once with the per-group uploads (hold_flow = false) and once with the held
// flow (hold_flow = true).
//
//   test_object_flow find <events.txt> <K> <res_x> <res_y> <guard_x> <guard_y> <min_events> <hard_cap> <prefix>
//                         [<merge_num> <merge_den> <dissolve_below>]
//       events.txt: "fr_x fr_y t_ns" per line.  With the last three, both runs merge (bf::ObjectMerger::reduce).  The program
//       itself requires the two runs to leave the same gid, models and counts (exit 3 otherwise) and the second to leave the
//       context holding a flow for the slice (exit 4).  Writes <prefix>gid.i32, models.bin, counts.i32, flow_host.f64 (K u then
//       K v: hold_flow = false), flow_held.f64 (the same with hold_flow = true), held_u.f64 / held_v.f64 (per event, read back
//       from the context the second run left) and frame.ppm.u8 / frame.flo.f32 (bf_global_render_flow_frame on that context,
//       BF_FLOW_LAST_UPLOADED).
//       A dissolve_below above the slice's size leaves no group: both runs must then return BF_OK with no model and no flow
//       figure, and the second must leave NO held flow (exit 5 when a reader does not return BF_ERR_STATE); only gid.i32 and
//       counts.i32 are written.
//   test_object_flow missing
//       prints what bf::ObjectFinder::missing_entry names without and with hold_flow, one per line ("-": nothing).
#include <better_flow/object_finder.h>

#include "object_test_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

template <class T>
static bool dump(const std::string &path, const T *v, size_t n) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (n) std::fwrite(v, sizeof(T), n, f);
    return std::fclose(f) == 0;
}

static void configure_merge(bf::ObjectFinder &of, char **argv) {
    of.merge_num = std::strtoull(argv[11], nullptr, 10);
    of.merge_den = std::strtoull(argv[12], nullptr, 10);
    of.dissolve_below = std::atoi(argv[13]);
}

static int run_find(int argc, char **argv) {
    Events e;
    if (!read_events(argv[2], e)) return 1;
    const std::vector<int32_t> &fx = e.fx;
    const std::string prefix = argv[10];
    bf::ObjectFinder plain, held;
    for (bf::ObjectFinder *of : {&plain, &held})
        configure(*of, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8]),
                  std::atoi(argv[9]));
    if (argc == 14) {
        configure_merge(plain, argv);
        configure_merge(held, argv);
    }
    held.hold_flow = true;
    const int res_x = plain.refit.fit.sensor_res_x, res_y = plain.refit.fit.sensor_res_y;
    bf_ctx *ctx = nullptr, *helper = nullptr;
    if (bf_create(0, (int64_t)fx.size() + 1, 3 * res_x + 3, 3 * res_y + 3, nullptr, &ctx) != BF_OK ||
        bf_create(0, (int64_t)fx.size() + 1, 3 * res_x + 3, 3 * res_y + 3, nullptr, &helper) != BF_OK)
        return 1;
    plain.refit.helper = held.refit.helper = helper;
    const bf::Slice sl = e.slice();
    int rc = plain.find(ctx, sl);
    if (rc == BF_OK) rc = held.find(ctx, sl);
    if (rc != BF_OK) {
        std::fprintf(stderr, "test_object_flow: find: %d: %s%s\n", rc, plain.error.c_str(), held.error.c_str());
        return 1;
    }
    const size_t K = plain.grouping.models.size();
    if (held.grouping.models.size() != K || held.grouping.gid != plain.grouping.gid || held.grouping.counts != plain.grouping.counts ||
        (K && std::memcmp(held.grouping.models.data(), plain.grouping.models.data(), K * sizeof(bf_model)) != 0)) {
        std::fprintf(stderr, "test_object_flow: hold_flow changed the grouping or the models\n");
        return 3;
    }
    std::vector<double> u(fx.size()), v(fx.size());
    if (K == 0) {   // no group: nothing is held
        if (bf_global_get_flow(ctx, nullptr, nullptr, u.data(), v.data(), nullptr, nullptr) != BF_ERR_STATE ||
            bf_group_flow_medians(ctx, nullptr, nullptr, nullptr) != BF_ERR_STATE) {
            std::fprintf(stderr, "test_object_flow: no group is left, yet the context holds a flow\n");
            return 5;
        }
        if (!held.flow_u.empty() || !held.flow_v.empty() || !plain.flow_u.empty()) return 3;
        const bool ok = dump(prefix + "gid.i32", held.grouping.gid.data(), held.grouping.gid.size()) &&
                        dump(prefix + "counts.i32", held.grouping.counts.data(), held.grouping.counts.size());
        bf_destroy(helper);
        bf_destroy(ctx);
        return ok ? 0 : 1;
    }
    // what the second run left on the context: the slice, the grouping and the held flow
    std::vector<uint8_t> ppm((size_t)res_x * (size_t)(3 * res_y) * 3);
    std::vector<float> flo((size_t)res_x * (size_t)res_y * 2);
    std::vector<int32_t> counts(K + 1);
    if (bf_global_get_flow(ctx, nullptr, nullptr, u.data(), v.data(), nullptr, nullptr) != BF_OK ||
        bf_global_render_flow_frame(ctx, res_x, res_y, BF_FLOW_LAST_UPLOADED, ppm.data(), nullptr, flo.data()) != BF_OK ||
        bf_group_flow_medians(ctx, nullptr, nullptr, counts.data()) != BF_OK || counts != held.grouping.counts) {
        std::fprintf(stderr, "test_object_flow: the context holds no flow of the slice: %s\n", bf_last_error(ctx));
        return 4;
    }
    std::vector<double> a(plain.flow_u), b(held.flow_u);
    a.insert(a.end(), plain.flow_v.begin(), plain.flow_v.end());
    b.insert(b.end(), held.flow_v.begin(), held.flow_v.end());
    const bool ok = dump(prefix + "gid.i32", held.grouping.gid.data(), held.grouping.gid.size()) && dump(prefix + "models.bin", held.grouping.models.data(), K) &&
                    dump(prefix + "counts.i32", held.grouping.counts.data(), held.grouping.counts.size()) && dump(prefix + "flow_host.f64", a.data(), a.size()) &&
                    dump(prefix + "flow_held.f64", b.data(), b.size()) && dump(prefix + "held_u.f64", u.data(), u.size()) &&
                    dump(prefix + "held_v.f64", v.data(), v.size()) && dump(prefix + "frame.ppm.u8", ppm.data(), ppm.size()) &&
                    dump(prefix + "frame.flo.f32", flo.data(), flo.size());
    bf_destroy(helper);
    bf_destroy(ctx);
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    if ((argc == 11 || argc == 14) && !std::strcmp(argv[1], "find")) return run_find(argc, argv);
    if (argc == 2 && !std::strcmp(argv[1], "missing")) {
        const char *a = bf::ObjectFinder::missing_entry(false, false), *b = bf::ObjectFinder::missing_entry(false, true);
        std::printf("%s\n%s\n", a ? a : "-", b ? b : "-");
        return 0;
    }
    std::fprintf(stderr, "usage: test_object_flow find events K res_x res_y guard_x guard_y min_events hard_cap prefix [num den dissolve_below]\n"
                         "       test_object_flow missing\n");
    return 2;
}
