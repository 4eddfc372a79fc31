// The interpolated field of OptimizerGlobal (better_flow_amd/host/better_flow/optimizer_global.h): project_field() under the
// filled answers of compute_flow_cells, the overload with explicit grids, get_event_field and write_field_flo.  Prints the
// sums, writes the cloud as loaded (argv[2]), the image (argv[3]), current_scores (argv[4]), the per-event nx, ny, u, v as raw
// doubles (argv[5]) and the .flo (argv[6]); tests/test_host_global_field.py compares them with the Python binding and the
// numpy restatement on the same cloud.
#include <better_flow/common.h>
#include <better_flow/event_file.h>
#include <better_flow/optimizer_global.h>
#include <cstdio>

static long long total(const std::vector<int64_t> &v) {
    long long s = 0;
    for (int64_t x : v) s += (long long)x;
    return s;
}

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    LinearEventCloud cloud;
    EventFile::from_file(&cloud, argv[1]);
    if (FILE *f = std::fopen(argv[2], "w")) {   // the cloud as loaded: the binding's input
        for (auto &e : cloud) std::fprintf(f, "%u %u %lld\n", e.fr_x, e.fr_y, (long long)e.t);
        std::fclose(f);
    }
    OptimizerGlobal og(&cloud, 3);   // window 15
    og.set_search_range(-0.06, 0.061, 0.004, -0.03, -0.019, 0.002);
    og.set_cells(96, 160, 32, 32);   // the slice lies on 64 x 128: the last row and column of cells have no event
    bool threw = false;
    try {
        og.project_field();   // before any cell search: there is nothing to apply
    } catch (const bf::AccelError &) {
        threw = true;
    }
    std::printf("no results threw=%d\n", threw ? 1 : 0);
    og.compute_flow_cells();
    og.read_back();
    double state = 0;   // the per-event state before the projection ...
    for (auto &e : cloud) state += e.max_score + e.best_pr_x + e.best_pr_y;
    const long long S_f = og.project_field();
    std::printf("grid %dx%d S_f=%lld last=%lld\n", og.get_n_cell_x(), og.get_n_cell_y(), S_f, og.get_last_sum());
    for (int cx = 0; cx < og.get_n_cell_x(); ++cx)
        for (int cy = 0; cy < og.get_n_cell_y(); ++cy) {
            const size_t i = (size_t)cx * og.get_n_cell_y() + cy;
            std::printf("cell %d %d %.17g %.17g %.17g %.17g %lld %lld\n", cx, cy, og.get_cell(cx, cy).best_nx,
                        og.get_cell(cx, cy).best_ny, og.get_field_nx()[i], og.get_field_ny()[i],
                        (long long)og.get_cell(cx, cy).events, (long long)og.get_cell_sums()[i]);
        }
    const bf::Image2D<uint8_t> &img = og.get_project_img();
    std::printf("img %dx%d scores %zu events %zu\n", img.rows, img.cols, og.get_current_scores().size(),
                og.get_event_field(0).size());
    if (FILE *f = std::fopen(argv[3], "wb")) {
        std::fwrite(img.data.data(), 1, img.data.size(), f);
        std::fclose(f);
    }
    if (FILE *f = std::fopen(argv[4], "wb")) {
        std::fwrite(og.get_current_scores().data(), sizeof(float), og.get_current_scores().size(), f);
        std::fclose(f);
    }
    if (FILE *f = std::fopen(argv[5], "wb")) {
        for (int k = 0; k < 4; ++k) std::fwrite(og.get_event_field(k).data(), sizeof(double), og.get_event_field(k).size(), f);
        std::fclose(f);
    }
    std::printf("flo written=%d\n", og.write_field_flo(argv[6]) ? 1 : 0);
    og.read_back();
    double state2 = 0;   // ... and after it
    for (auto &e : cloud) state2 += e.max_score + e.best_pr_x + e.best_pr_y;
    std::printf("state kept=%d\n", state == state2 ? 1 : 0);
    // grids of another length than the cell grid, or of two lengths, are refused and the previous results stay
    const size_t nc = og.get_cell_results().size();
    const std::vector<double> kept_nx = og.get_field_nx(), kept_ev = og.get_event_field(2);
    const long long kept_cells = total(og.get_cell_sums());
    int refused = 0;
    const std::vector<double> fit(nc, 0.0), longer(nc + 1, 0.0), shorter(nc - 1, 0.0);
    for (const std::vector<double> *g : {&longer, &shorter})
        for (int which = 0; which < 3; ++which) {
            try {
                og.project_field(which == 1 ? fit : *g, which == 0 ? fit : *g);
            } catch (const bf::AccelError &e) {
                refused += e.code == BF_ERR_ARG ? 1 : 0;
            }
        }
    std::vector<double> nan_grid(nc, 0.0);
    nan_grid[nc - 1] = std::nan("");   // a cell without events: read all the same
    try {
        og.project_field(nan_grid, fit);
    } catch (const bf::AccelError &e) {
        refused += e.code == BF_ERR_ARG ? 1 : 0;
    }
    const bool kept = og.get_cell_sums().size() == nc && total(og.get_cell_sums()) == kept_cells && og.get_field_nx() == kept_nx &&
                      og.get_event_field(2) == kept_ev && og.get_last_sum() == S_f;
    std::printf("refused=%d results kept=%d\n", refused, kept ? 1 : 0);
    // an explicit grid: the filled one mirrored left <-> right
    std::vector<double> mx(nc), my(nc);
    const int ncy = og.get_n_cell_y();
    for (size_t i = 0; i < nc; ++i) {
        const size_t j = (i / ncy) * ncy + (ncy - 1 - i % ncy);
        mx[i] = kept_nx[j]; my[i] = og.get_field_ny()[j];
    }
    const long long S_m = og.project_field(mx, my);
    std::printf("mirrored S=%lld cells=%lld\n", S_m, total(og.get_cell_sums()));
    // the slice's one flow in every cell is project_all of it
    const long long S_uni = og.project_field(std::vector<double>(nc, og.get_best_nx()), std::vector<double>(nc, og.get_best_ny()));
    const long long cells_total = total(og.get_cell_sums());
    bool uniform_ev = true;
    for (double v : og.get_event_field(0)) uniform_ev = uniform_ev && v == og.get_best_nx();
    const long long S_all = og.project_all(og.get_best_nx(), og.get_best_ny());
    std::printf("uniform S=%lld cells=%lld project_all S=%lld best S=%lld events uniform=%d\n", S_uni, cells_total, S_all,
                og.get_best_sum(), uniform_ev ? 1 : 0);
    return 0;
}
