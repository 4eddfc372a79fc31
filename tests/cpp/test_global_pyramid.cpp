// The coarse-to-fine and seeded per-cell search of OptimizerGlobal (better_flow_amd/host/better_flow/optimizer_global.h):
// compute_flow_cells_pyramid on a first slice, its answers as the seeds of compute_flow_cells_seeded on a second one, the
// per-cell getters and write_cell_flo.  Prints full-precision numbers and writes the two clouds as loaded (argv[3], argv[4])
// and the second slice's .flo (argv[5]); tests/test_host_global_pyramid.py compares them with the numpy restatement
// (tests/global_pyramid_ref.py).
#include <better_flow/common.h>
#include <better_flow/event_file.h>
#include <better_flow/optimizer_global.h>
#include <cstdio>

static void dump_cloud(LinearEventCloud &cloud, const char *path) {
    if (FILE *f = std::fopen(path, "w")) {
        for (auto &e : cloud) std::fprintf(f, "%u %u %lld\n", e.fr_x, e.fr_y, (long long)e.t);
        std::fclose(f);
    }
}

static void print(const char *tag, const OptimizerGlobal &og) {
    const bf_global_pyramid_info &pi = og.get_pyramid_info();
    std::printf("%s grid %dx%d slice nx=%.17g ny=%.17g S=%lld lattice=%lldx%lld evaluated=%lld levels=%d counts", tag,
                og.get_n_cell_x(), og.get_n_cell_y(), og.get_best_nx(), og.get_best_ny(), og.get_best_sum(), (long long)pi.n_x,
                (long long)pi.n_y, (long long)pi.evaluated, (int)pi.levels_run);
    for (int l = 0; l < pi.levels_run; ++l) std::printf(" %lld", (long long)pi.level_count[l]);
    std::printf("\n");
    for (int cx = 0; cx < og.get_n_cell_x(); ++cx)
        for (int cy = 0; cy < og.get_n_cell_y(); ++cy) {
            const bf_global_cell_result &r = og.get_cell(cx, cy);
            std::printf("%s cell %d %d %.17g %.17g %.17g %.17g %lld %lld %lld\n", tag, cx, cy, r.best_nx, r.best_ny, r.best_u,
                        r.best_v, (long long)r.best_sum, (long long)r.best_index, (long long)r.events);
        }
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    LinearEventCloud a, b;
    EventFile::from_file(&a, argv[1]);
    EventFile::from_file(&b, argv[2]);
    dump_cloud(a, argv[3]);
    dump_cloud(b, argv[4]);
    bf_global_pyramid_opts coarse, fine;
    coarse.levels = 3; coarse.factor = 2; coarse.radius = 2;
    fine.levels = 1; fine.factor = 2; fine.radius = 2;

    OptimizerGlobal first(&a, 3);   // window 15
    first.set_search_range(0.036, 0.0585, 0.001, -0.0375, -0.0250, 0.001);
    first.set_cells(64, 48, 16, 16);   // the clouds lie on the upper rows: the last rows of cells are empty
    first.compute_flow_cells_seeded(coarse);   // no seeds yet: the unseeded pyramid
    print("first", first);

    OptimizerGlobal second(&b, 3);
    second.set_search_range(0.036, 0.0585, 0.001, -0.0375, -0.0250, 0.001);
    second.set_cells(64, 48, 16, 16);
    second.set_seeds(first.get_seeds());
    second.compute_flow_cells_seeded(fine);
    print("second", second);
    std::printf("flo written=%d\n", second.write_cell_flo(argv[5]) ? 1 : 0);
    second.clear_seeds();
    std::printf("cleared seeds=%d\n", (int)second.get_seeds().size());
    second.read_back();
    unsigned long long k = 0;
    for (auto &e : b) {
        if (k % 97 == 0)
            std::printf("event %llu %.17g %.17g %.17g %.17g %.17g\n", k, e.max_score, e.best_pr_x, e.best_pr_y, e.best_u, e.best_v);
        ++k;
    }
    return 0;
}
