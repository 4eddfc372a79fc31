// OptimizerGlobal (better_flow_amd/host/better_flow/optimizer_global.h) driven the way a caller of the reference's class
// would: the three constructors, project_all, a narrowed compute_flow_bruteforce, the per-event read-back.  Prints
// full-precision numbers and writes the cloud as loaded (argv[2]); tests/test_host_global.py compares them with the numpy restatement (tests/global_ref.py).
#include <better_flow/common.h>
#include <better_flow/event_file.h>
#include <better_flow/optimizer_global.h>
#include <cstdio>

static void print_events(const char *tag, LinearEventCloud &cloud) {
    unsigned long long k = 0;
    for (auto &e : cloud) {
        if (k % 97 == 0)
            std::printf("%s event %llu %.17g %.17g %.17g %.17g %.17g\n", tag, k, e.max_score, e.best_pr_x, e.best_pr_y,
                        e.best_u, e.best_v);
        ++k;
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    LinearEventCloud cloud;
    EventFile::from_file(&cloud, argv[1]);
    if (FILE *f = std::fopen(argv[2], "w")) {   // the cloud as loaded: the restatement's input
        for (auto &e : cloud) std::fprintf(f, "%u %u %lld\n", e.fr_x, e.fr_y, (long long)e.t);
        std::fclose(f);
    }
    {
        OptimizerGlobal og(&cloud);   // scale 5, window 21
        long long s0 = og.project_all(0.0, 0.0);
        unsigned long long sum = 0;
        const bf::Image2D<uint8_t> &img = og.get_project_img();
        for (size_t i = 0; i < img.data.size(); ++i) sum += img.data[i] * (unsigned long long)(i % 251 + 1);
        std::printf("default S0=%lld img=%dx%d checksum=%llu\n", s0, img.rows, img.cols, sum);
        og.set_search_range(-0.01, 0.0105, 0.001, -0.005, 0.0055, 0.001);
        og.compute_flow_bruteforce();
        std::printf("default best nx=%.17g ny=%.17g S=%lld grid=%lldx%lld\n", og.get_best_nx(), og.get_best_ny(),
                    og.get_best_sum(), og.get_n_x(), og.get_n_y());
        og.read_back();
        print_events("default", cloud);
    }
    {
        OptimizerGlobal og(&cloud, 3);   // window 15
        long long s = og.project_all(0.02, -0.01);
        std::printf("scale3 S=%lld\n", s);
    }
    {   // two objects alive at once on one thread, at different windows, calls interleaved
        OptimizerGlobal a(&cloud, 3, 5), b(&cloud, 7, 35);
        long long sa1 = a.project_all(0.01, 0.0);
        long long sb1 = b.project_all(-0.02, 0.01);
        long long sa2 = a.project_all(-0.005, 0.002);
        a.read_back();
        double ms = 0;
        for (auto &e : cloud) ms += e.max_score;
        const bf::Image2D<uint8_t> &ia = a.get_project_img();
        std::printf("pair a1=%lld b1=%lld a2=%lld img=%dx%d max_score_sum=%.17g\n", sa1, sb1, sa2, ia.rows, ia.cols, ms);
    }
    {
        OptimizerGlobal og(&cloud, 7, 9);
        long long s = og.project_all(-0.03, 0.02, 127);
        double tot = 0;
        for (float f : og.get_current_scores()) tot += f;
        std::printf("scale7 S=%lld scores_sum=%.17g\n", s, tot);
    }
    return 0;
}
