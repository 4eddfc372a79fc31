// The piecewise projection of OptimizerGlobal (better_flow_amd/host/better_flow/optimizer_global.h): project_cells() under
// the answers of compute_flow_cells, and the overload with explicit grids.  Prints the sums, writes the cloud as loaded
// (argv[2]), the image (argv[3]) and current_scores (argv[4]) as raw bytes; tests/test_host_global_piecewise.py compares them
// with the Python binding on the same cloud.
#include <better_flow/common.h>
#include <better_flow/event_file.h>
#include <better_flow/optimizer_global.h>
#include <cstdio>

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    LinearEventCloud cloud;
    EventFile::from_file(&cloud, argv[1]);
    if (FILE *f = std::fopen(argv[2], "w")) {   // the cloud as loaded: the binding's input
        for (auto &e : cloud) std::fprintf(f, "%u %u %lld\n", e.fr_x, e.fr_y, (long long)e.t);
        std::fclose(f);
    }
    OptimizerGlobal og(&cloud, 3);   // window 15
    og.set_search_range(-0.045, 0.056, 0.005, -0.03, 0.036, 0.005);
    og.set_cells(64, 128, 32, 32);
    bool threw = false;
    try {
        og.project_cells();   // before any cell search: there is nothing to apply
    } catch (const bf::AccelError &) {
        threw = true;
    }
    std::printf("no results threw=%d\n", threw ? 1 : 0);
    og.compute_flow_cells();
    og.read_back();
    double state = 0;   // the per-event state before the projection ...
    for (auto &e : cloud) state += e.max_score + e.best_pr_x + e.best_pr_y;
    const long long S_pw = og.project_cells();
    std::printf("grid %dx%d slice nx=%.17g ny=%.17g S=%lld S_pw=%lld last=%lld\n", og.get_n_cell_x(), og.get_n_cell_y(),
                og.get_best_nx(), og.get_best_ny(), og.get_best_sum(), S_pw, og.get_last_sum());
    for (int cx = 0; cx < og.get_n_cell_x(); ++cx)
        for (int cy = 0; cy < og.get_n_cell_y(); ++cy)
            std::printf("cell %d %d %.17g %.17g %lld\n", cx, cy, og.get_cell(cx, cy).best_nx, og.get_cell(cx, cy).best_ny,
                        (long long)og.get_cell_sums()[(size_t)cx * og.get_n_cell_y() + cy]);
    const bf::Image2D<uint8_t> &img = og.get_project_img();
    std::printf("img %dx%d scores %zu\n", img.rows, img.cols, og.get_current_scores().size());
    if (FILE *f = std::fopen(argv[3], "wb")) {
        std::fwrite(img.data.data(), 1, img.data.size(), f);
        std::fclose(f);
    }
    if (FILE *f = std::fopen(argv[4], "wb")) {
        std::fwrite(og.get_current_scores().data(), sizeof(float), og.get_current_scores().size(), f);
        std::fclose(f);
    }
    og.read_back();
    double state2 = 0;   // ... and after it
    for (auto &e : cloud) state2 += e.max_score + e.best_pr_x + e.best_pr_y;
    std::printf("state kept=%d\n", state == state2 ? 1 : 0);
    // explicit grids: the slice's one flow in every cell is project_all of it
    const size_t nc = og.get_cell_results().size();
    const long long S_uni = og.project_cells(std::vector<double>(nc, og.get_best_nx()), std::vector<double>(nc, og.get_best_ny()));
    long long cells_total = 0;
    for (int64_t v : og.get_cell_sums()) cells_total += (long long)v;
    const long long S_all = og.project_all(og.get_best_nx(), og.get_best_ny());
    std::printf("uniform S=%lld cells=%lld project_all S=%lld\n", S_uni, cells_total, S_all);
    // grids of another length than the cell grid, or of two lengths, are refused and the kept sums stay
    int refused = 0;
    const std::vector<double> fit(nc, 0.0), longer(nc + 1, 0.0), shorter(nc - 1, 0.0);
    for (const std::vector<double> *g : {&longer, &shorter})
        for (int which = 0; which < 3; ++which) {
            try {
                og.project_cells(which == 1 ? fit : *g, which == 0 ? fit : *g);
            } catch (const bf::AccelError &e) {
                refused += e.code == BF_ERR_ARG ? 1 : 0;
            }
        }
    long long cells_after = 0;
    for (int64_t v : og.get_cell_sums()) cells_after += (long long)v;
    std::printf("refused=%d sums kept=%d\n", refused, og.get_cell_sums().size() == nc && cells_after == cells_total ? 1 : 0);
    return 0;
}
