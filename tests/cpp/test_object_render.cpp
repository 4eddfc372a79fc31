// test_object_render.cpp -- bf::ObjectRenderer (host/better_flow/object_render.h) as a stand-alone program, linked either against
// the CPU stand-in of the C-ABI (tests/shim + the oracle: project_host, also under ASan / UBSan) or against libbf_accel.so
// (bf_project_groups).
//
//   test_object_render <events.txt> <ids.i32> <models.bin> <K> <scale> <res_x> <res_y> <margin> <gain> <prefix>
//
// events.txt: "fr_x fr_y t_ns" per line (may be empty).  ids.i32: one group id per event.  models.bin: K bf_model records.
// Writes <prefix>count.u32, <prefix>label.i32, <prefix>bgr.u8, <prefix>scores.bin (K bf_group_score), <prefix>info.bin, and through
// the writers <prefix>img.ppm, <prefix>label.pgm, <prefix>scores.txt; prints "path device|host".
#include <better_flow/object_render.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int die(const char *what, bf_ctx *ctx) {
    std::fprintf(stderr, "test_object_render: %s: %s\n", what, ctx ? bf_last_error(ctx) : "");
    return 1;
}

template <class T>
static bool dump(const std::string &path, const T *v, size_t n) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (n) std::fwrite(v, sizeof(T), n, f);
    return std::fclose(f) == 0;
}

int main(int argc, char **argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: test_object_render events ids models K scale res_x res_y margin gain prefix\n");
        return 2;
    }
    const int K = std::atoi(argv[4]);
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
    std::vector<int32_t> ids(fx.size());
    std::vector<bf_model> models((size_t)K);
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) return die("cannot read the ids", nullptr);
        const size_t got = ids.empty() ? 0 : std::fread(ids.data(), sizeof(int32_t), ids.size(), f);
        std::fclose(f);
        if (got != ids.size()) return die("short ids file", nullptr);
        f = std::fopen(argv[3], "rb");
        if (!f) return die("cannot read the models", nullptr);
        const size_t gm = std::fread(models.data(), sizeof(bf_model), (size_t)K, f);
        std::fclose(f);
        if (gm != (size_t)K) return die("short models file", nullptr);
    }
    bf::ObjectRenderer r;
    r.opts.scale = std::atoi(argv[5]);
    r.opts.sensor_res_x = std::atoi(argv[6]); r.opts.sensor_res_y = std::atoi(argv[7]);
    r.opts.margin = std::atoi(argv[8]);
    r.opts.gain = std::atoi(argv[9]);
    const std::string prefix = argv[10];

    bf_ctx *ctx = nullptr;
    const int s = r.opts.scale;
    if (bf_create(0, (int64_t)fx.size() + 1, s * r.opts.sensor_res_x + s, s * r.opts.sensor_res_y + s, nullptr, &ctx) != BF_OK)
        return die("bf_create", nullptr);
    std::printf("path %s\n", bf::ObjectRenderer::device_available() ? "device" : "host");
    const bf::Slice sl = {fx.data(), fy.data(), t.data(), fx.size()};

    // refused on either path: an id outside -1 .. K-1, a gain of zero
    if (!ids.empty()) {
        std::vector<int32_t> bad(ids);
        bad[0] = K;
        if (r.render(ctx, sl, bad, models) != BF_ERR_ARG) return die("an id beyond the groups was not refused", nullptr);
    }
    const int gain = r.opts.gain;
    r.opts.gain = 0;
    if (r.render(ctx, sl, ids, models) != BF_ERR_ARG) return die("a gain of zero was not refused", nullptr);
    r.opts.gain = gain;

    if (r.render(ctx, sl, ids, models) != BF_OK) return die("render", ctx);
    if (!dump(prefix + "count.u32", r.count.data(), r.count.size()) || !dump(prefix + "label.i32", r.label.data(), r.label.size()) ||
        !dump(prefix + "bgr.u8", r.bgr.data(), r.bgr.size()) || !dump(prefix + "scores.bin", r.scores.data(), r.scores.size()) ||
        !dump(prefix + "info.bin", &r.info, 1))
        return die("cannot write the outputs", nullptr);
    if (!r.write_ppm(prefix + "img.ppm") || !r.write_label_pgm(prefix + "label.pgm") || !r.write_scores(prefix + "scores.txt"))
        return die("cannot write the images", nullptr);
    bf_destroy(ctx);
    return 0;
}
