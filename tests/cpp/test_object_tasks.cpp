// test_object_tasks.cpp -- bf::ObjectTasks (host/better_flow/object_tasks.h) as a stand-alone program, linked either against the
// CPU stand-in of the C-ABI (tests/shim + the oracle: the host path, also under ASan / UBSan) or against libbf_accel.so (the
// device path).
//
//   test_object_tasks <events.txt> <groups> <scale> <res_x> <res_y> <guard_x> <guard_y> <min_events> <hard_cap> <models.bin|-> <prefix>
//
// events.txt: "fr_x fr_y t_ns group" per line (group -1: in no task).  models.bin: <groups> bf_model records the tasks start
// from, "-": cold.  Writes <prefix>models.bin (bf_model), <prefix>infos.i32 (rc, iterations per task) and <prefix>nxny.f64
// (nx then ny, per event); prints "path device|host".
#include <better_flow/object_tasks.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int die(const char *what, bf_ctx *ctx) {
    std::fprintf(stderr, "test_object_tasks: %s: %s\n", what, ctx ? bf_last_error(ctx) : "");
    return 1;
}

template <class T>
static bool dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    return std::fclose(f) == 0;
}

int main(int argc, char **argv) {
    if (argc != 12) {
        std::fprintf(stderr, "usage: test_object_tasks events groups scale res_x res_y guard_x guard_y min_events hard_cap models|- prefix\n");
        return 2;
    }
    const int K = std::atoi(argv[2]);
    if (K < 0) return die("bad group count", nullptr);
    std::vector<int32_t> fx, fy, t;
    std::vector<std::vector<int32_t>> ids((size_t)K);
    {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) return die("cannot read the events", nullptr);
        char line[256];
        while (std::fgets(line, sizeof(line), f)) {
            long a, b, c, g;
            if (std::sscanf(line, "%ld %ld %ld %ld", &a, &b, &c, &g) != 4) continue;
            if (g >= K) { std::fclose(f); return die("group id beyond the count", nullptr); }
            if (g >= 0) ids[(size_t)g].push_back((int32_t)fx.size());
            fx.push_back((int32_t)a); fy.push_back((int32_t)b); t.push_back((int32_t)c);
        }
        std::fclose(f);
    }
    bf::ObjectTasks q;
    q.opts.scale = std::atoi(argv[3]);
    q.opts.sensor_res_x = std::atoi(argv[4]); q.opts.sensor_res_y = std::atoi(argv[5]);
    q.opts.guard_res_x = std::atoi(argv[6]); q.opts.guard_res_y = std::atoi(argv[7]);
    q.opts.min_events = std::atoi(argv[8]);
    q.opts.hard_iter_cap = std::atoi(argv[9]);
    std::vector<bf_model> warm;
    if (std::string(argv[10]) != "-") {
        warm.resize((size_t)K);
        FILE *f = std::fopen(argv[10], "rb");
        if (!f) return die("cannot read the models", nullptr);
        const size_t got = K > 0 ? std::fread(warm.data(), sizeof(bf_model), (size_t)K, f) : 0;
        std::fclose(f);
        if (got != (size_t)K) return die("short models file", nullptr);
    }
    for (int k = 0; k < K; ++k) q.push(ids[(size_t)k], warm.empty() ? nullptr : &warm[(size_t)k]);
    const std::string prefix = argv[11];

    bf_ctx *ctx = nullptr;
    const int s = q.opts.scale;
    if (bf_create(0, (int64_t)fx.size() + 1, s * q.opts.sensor_res_x + s, s * q.opts.sensor_res_y + s, nullptr, &ctx) != BF_OK)
        return die("bf_create", nullptr);
    const int rc = q.run(ctx, fx.data(), fy.data(), t.data(), fx.size());
    if (rc != BF_OK) return die("ObjectTasks::run", ctx);
    std::printf("path %s\n", bf::ObjectTasks::device_available() ? "device" : "host");
    std::vector<int32_t> infos;
    for (const bf_run_info &i : q.infos) { infos.push_back(i.rc); infos.push_back(i.iterations); }
    std::vector<double> nxny(q.nx);
    nxny.insert(nxny.end(), q.ny.begin(), q.ny.end());
    if (!dump(prefix + "models.bin", q.models) || !dump(prefix + "infos.i32", infos) || !dump(prefix + "nxny.f64", nxny))
        return die("cannot write the outputs", nullptr);
    // an event in two tasks is refused on either path
    if (K > 0 && !ids[0].empty()) {
        q.push(std::vector<int32_t>(1, ids[0][0]));
        if (q.run(ctx, fx.data(), fy.data(), t.data(), fx.size()) != BF_ERR_ARG) return die("a doubly claimed event was not refused", nullptr);
    }
    bf_destroy(ctx);
    return 0;
}
