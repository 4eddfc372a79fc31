// test_segment.cpp -- bf::Segmenter (host/better_flow/clustering.h) as a stand-alone program, linked either against the CPU
// stand-in of the C-ABI (tests/shim + the oracle: the host path, also under ASan / UBSan) or against libbf_accel.so (the device
// path AND the host path on the same context, compared byte for byte here).
//
//   test_segment <events.txt> <scale> <res_x> <res_y> <nx> <ny> <above_s> <below_s> <min_count> <connectivity> <min_pixels> <prefix>
//
// events.txt: "fr_x fr_y t_ns [noise]" per line.  The slice is compensated with bf_project_4param_reinit(nx, ny, 0, 0, 0, 0).
// Writes <prefix>labels.i32, <prefix>comps.bin (bf_component rows), <prefix>cl_id.i32, <prefix>segments.txt and
// <prefix>labels.pgm; prints "path device|host", the info fields and, with both paths, "paths agree" and the wall time of each
// (the second run of each path: buffers grown, for scripts/segment_bench.py).
#include <better_flow/clustering.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int die(const char *what, bf_ctx *ctx) {
    std::fprintf(stderr, "test_segment: %s: %s\n", what, ctx ? bf_last_error(ctx) : "");
    return 1;
}

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    return std::fclose(f) == 0;
}

static bool same(const bf::Segmentation &a, const bf::Segmentation &b) {
    return std::memcmp(&a.info, &b.info, sizeof(a.info)) == 0 && a.labels == b.labels && a.cl_id == b.cl_id &&
           a.comps.size() == b.comps.size() &&
           (a.comps.empty() || std::memcmp(a.comps.data(), b.comps.data(), a.comps.size() * sizeof(bf_component)) == 0);
}

int main(int argc, char **argv) {
    if (argc != 13) {
        std::fprintf(stderr, "usage: test_segment events scale res_x res_y nx ny above below min_count connectivity min_pixels prefix\n");
        return 2;
    }
    std::vector<int32_t> fx, fy, t;
    std::vector<uint8_t> noise;
    bool any_noise = false;
    {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) return die("cannot read the events", nullptr);
        char line[256];
        while (std::fgets(line, sizeof(line), f)) {
            long a, b, c, d = 0;
            const int got = std::sscanf(line, "%ld %ld %ld %ld", &a, &b, &c, &d);
            if (got < 3) continue;
            fx.push_back((int32_t)a); fy.push_back((int32_t)b); t.push_back((int32_t)c);
            noise.push_back((uint8_t)(d != 0));
            any_noise = any_noise || d != 0;
        }
        std::fclose(f);
    }
    const int scale = std::atoi(argv[2]), res_x = std::atoi(argv[3]), res_y = std::atoi(argv[4]);
    const double nx = std::atof(argv[5]), ny = std::atof(argv[6]);
    bf::Segmenter seg;
    seg.opts.above_s = std::atof(argv[7]);
    seg.opts.below_s = std::atof(argv[8]);
    seg.opts.min_count = std::atoi(argv[9]);
    seg.opts.connectivity = std::atoi(argv[10]);
    seg.opts.min_pixels = std::atoi(argv[11]);
    const std::string prefix = argv[12];

    bf_ctx *ctx = nullptr;
    if (bf_create(0, (int64_t)fx.size() + 1, scale * res_x + scale, scale * res_y + scale, nullptr, &ctx) != BF_OK)
        return die("bf_create", nullptr);
    const uint8_t *flags = any_noise ? noise.data() : nullptr;
    if (bf_upload_events(ctx, fx.data(), fy.data(), t.data(), flags, (int64_t)fx.size()) != BF_OK) return die("upload", ctx);
    bf_window w;
    if (bf_set_cloud(ctx, scale, res_x, res_y, &w) != BF_OK) return die("bf_set_cloud", ctx);
    if (bf_project_4param_reinit(ctx, nx, ny, 0.0, 0.0, 0.0, 0.0) != BF_OK) return die("warp", ctx);

    bf::Segmentation out;
    const bool device = bf::Segmenter::device_available();
    int rc = seg.run(ctx, w, fx.size(), flags, out);
    if (rc != BF_OK) return die("Segmenter::run", ctx);
    std::printf("path %s\n", device ? "device" : "host");
    if (device) {
        bf::Segmentation host;
        rc = seg.run(ctx, w, fx.size(), flags, host, true);
        if (rc != BF_OK) return die("Segmenter::run (host path)", ctx);
        if (!same(out, host)) {
            std::fprintf(stderr, "test_segment: the device path and the host path differ\n");
            return 1;
        }
        std::printf("paths agree\n");
        double ms[2];
        for (int k = 0; k < 2; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            rc = seg.run(ctx, w, fx.size(), flags, host, k == 1);
            if (rc != BF_OK) return die("Segmenter::run (timed)", ctx);
            ms[k] = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        std::printf("time_ms device %.3f host %.3f\n", ms[0], ms[1]);
    }
    std::printf("info %d %d %lld %lld %lld %d %d %d\n", out.info.rows, out.info.cols, (long long)out.info.n1, (long long)out.info.q_sum,
                (long long)out.info.q_mean, out.info.foreground_pixels, out.info.components_found, out.info.components);
    if (!dump(prefix + "labels.i32", out.labels) || !dump(prefix + "comps.bin", out.comps) || !dump(prefix + "cl_id.i32", out.cl_id) ||
        !bf::write_segments_txt(prefix + "segments.txt", out) || !bf::write_labels_pgm(prefix + "labels.pgm", out))
        return die("cannot write the outputs", nullptr);
    // bad options are refused on either path
    seg.opts.connectivity = 6;
    bf::Segmentation bad;
    if (seg.run(ctx, w, fx.size(), flags, bad) != BF_ERR_ARG) return die("connectivity 6 was not refused", nullptr);
    bf_destroy(ctx);
    return 0;
}
