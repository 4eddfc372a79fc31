// object_test_common.h -- what the stand-alone programs of the object pipeline (test_object_merge, test_object_flow,
// test_object_tracker, test_groups_wide) share: a slice read from "fr_x fr_y t_ns" lines, the finder's configuration for the
// tests' scenes, and a byte string to compare results through.
#ifndef BF_TESTS_OBJECT_TEST_COMMON_H
#define BF_TESTS_OBJECT_TEST_COMMON_H

#include <better_flow/object_finder.h>

#include <cstdio>
#include <string>
#include <vector>

struct Events {
    std::vector<int32_t> fx, fy, t;
    bf::Slice slice() const {
        const bf::Slice s = {fx.data(), fy.data(), t.data(), fx.size()};
        return s;
    }
};

inline bool read_events(const char *path, Events &e) {
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char line[256];
    while (std::fgets(line, sizeof(line), f)) {
        long a, b, c;
        if (std::sscanf(line, "%ld %ld %ld", &a, &b, &c) != 3) continue;
        e.fx.push_back((int32_t)a); e.fy.push_back((int32_t)b); e.t.push_back((int32_t)c);
    }
    std::fclose(f);
    return true;
}

// The search over -0.72 .. 0.72 in steps of 0.04 on both axes, K proposals, the sensor and the refit's guards.
inline void configure(bf::ObjectFinder &of, int K, int res_x, int res_y, int guard_x, int guard_y, int min_events, int hard_cap) {
    of.lattice.x_low = of.lattice.y_low = -0.72;
    of.lattice.x_hi = of.lattice.y_hi = 0.72;
    of.lattice.x_step = of.lattice.y_step = 0.04;
    of.propose.max_models = K;
    of.assign.sensor_res_x = of.refit.fit.sensor_res_x = res_x;
    of.assign.sensor_res_y = of.refit.fit.sensor_res_y = res_y;
    of.refit.fit.guard_res_x = guard_x; of.refit.fit.guard_res_y = guard_y;
    of.refit.fit.min_events = min_events;
    of.refit.fit.hard_iter_cap = hard_cap;
}
inline void configure(bf::ObjectFinder &of, int K, int res_x, int res_y) { configure(of, K, res_x, res_y, res_x, res_y, 100, 20000); }

// everything compared goes through one byte string
struct Bytes {
    std::string s;
    template <class T> void add(const std::vector<T> &v) {
        const uint64_t n = v.size();
        s.append(reinterpret_cast<const char *>(&n), sizeof(n));
        if (n) s.append(reinterpret_cast<const char *>(v.data()), n * sizeof(T));
    }
    void add(int64_t v) { s.append(reinterpret_cast<const char *>(&v), sizeof(v)); }
    void add(const std::vector<bf::MotionAssigner::Record> &recs) {
        add((int64_t)recs.size());
        for (const bf::MotionAssigner::Record &r : recs) {
            add((int64_t)r.changed);
            add(r.counts);
            add(r.iterations);
        }
    }
};

#endif  // BF_TESTS_OBJECT_TEST_COMMON_H
