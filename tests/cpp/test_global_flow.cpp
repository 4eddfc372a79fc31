// The held flow of OptimizerGlobal (better_flow_amd/host/better_flow/optimizer_global.h): hold_field() under the filled
// answers of compute_flow_cells, the overload with explicit grids, hold_best, get_flow, flow_field, write_flow_flo,
// write_flow_ppm and emit_slice, on a 64 x 128 sensor.  Writes the cloud as loaded (argv[2]) and, into the directory argv[3],
// per hold <name>.flow (nx, ny, u, v, pr_x, pr_y as raw doubles), <name>.field (owner as int32, then u, v), <name>.flo,
// <name>.ppm and <name>.rows (t u64, row u16, col u16, u, v per column); tests/test_host_global_flow.py compares them with the
// Python binding on the same cloud.
#include <better_flow/common.h>
#include <better_flow/event_file.h>
#include <better_flow/flow_table.h>
#include <better_flow/optimizer_global.h>
#include <cstdio>
#include <functional>

static void put(FILE *f, const void *p, size_t bytes) {
    if (bytes) std::fwrite(p, 1, bytes, f);
}

static int state_error(const std::function<void()> &call) {   // 1: the call threw BF_ERR_STATE
    try {
        call();
    } catch (const bf::AccelError &e) {
        return e.code == BF_ERR_STATE ? 1 : 0;
    }
    return 0;
}

// every reader of the held flow, into <dir>/<name>.*; the slice's rows start a fresh table
static void dump(OptimizerGlobal &og, const std::string &dir, const std::string &name, size_t n) {
    const std::string base = dir + "/" + name;
    std::vector<double> a[6];
    og.get_flow(&a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
    if (FILE *f = std::fopen((base + ".flow").c_str(), "wb")) {
        for (int k = 0; k < 6; ++k) put(f, a[k].data(), a[k].size() * sizeof(double));
        std::fclose(f);
    }
    const bf::FlowField fld = og.flow_field();
    if (FILE *f = std::fopen((base + ".field").c_str(), "wb")) {
        put(f, fld.owner.data(), fld.owner.size() * sizeof(int32_t));
        put(f, fld.u.data(), fld.u.size() * sizeof(double));
        put(f, fld.v.data(), fld.v.size() * sizeof(double));
        std::fclose(f);
    }
    const bool flo = og.write_flow_flo(base + ".flo"), ppm = og.write_flow_ppm(base + ".ppm");
    bf_emit *em = nullptr;
    int rc = bf_emit_create(og.own_context(), (int64_t)(4 * n + 4), RES_X, RES_Y, (int64_t)(2 * n + 2), &em);
    long long rows = -1;
    if (rc == BF_OK) {
        const int64_t ticket = og.emit_slice(em, 0, 1000);
        uint64_t first_row = 0;
        int64_t nr = 0;
        uint64_t *t; uint16_t *row, *col; double *u, *v;
        int64_t R = 0;
        if (ticket >= 0 && bf_emit_wait(og.own_context(), em, ticket, &first_row, &nr) == BF_OK &&
            bf_emit_output(em, &t, &row, &col, &u, &v, &R) == BF_OK) {
            rows = (long long)nr;
            if (FILE *f = std::fopen((base + ".rows").c_str(), "wb")) {   // (a fresh table: the rows start at 0, nothing wraps)
                put(f, t + first_row, (size_t)nr * 8); put(f, row + first_row, (size_t)nr * 2); put(f, col + first_row, (size_t)nr * 2);
                put(f, u + first_row, (size_t)nr * 8); put(f, v + first_row, (size_t)nr * 8);
                std::fclose(f);
            }
            bf_emit_release(em, first_row + (uint64_t)nr);
        }
        bf_emit_destroy(em);
    }
    std::printf("%s events=%zu field=%dx%d flo=%d ppm=%d rows=%lld\n", name.c_str(), a[0].size(), fld.rows, fld.cols, flo ? 1 : 0,
                ppm ? 1 : 0, rows);
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    bf::sensor().res_x = 64;
    bf::sensor().res_y = 128;
    LinearEventCloud cloud;
    EventFile::from_file(&cloud, argv[1]);
    if (FILE *f = std::fopen(argv[2], "w")) {   // the cloud as loaded: the binding's input
        for (auto &e : cloud) std::fprintf(f, "%u %u %lld\n", e.fr_x, e.fr_y, (long long)e.t);
        std::fclose(f);
    }
    const std::string dir = argv[3];
    const size_t n = cloud.size();
    OptimizerGlobal og(&cloud, 3);   // window 15
    og.set_search_range(-0.06, 0.061, 0.004, -0.03, -0.019, 0.002);
    og.set_cells(64, 128, 32, 32);
    bool threw = false;
    try {
        og.hold_field();   // before any cell search: there is nothing to hold
    } catch (const bf::AccelError &) {
        threw = true;
    }
    std::printf("no results threw=%d\n", threw ? 1 : 0);
    std::printf("no hold state errors=%d\n", state_error([&] { og.flow_field(); }) + state_error([&] { og.write_flow_ppm(dir + "/none.ppm"); }) +
                                                 state_error([&] { og.get_flow(nullptr, nullptr, nullptr, nullptr); }));
    og.compute_flow_cells();
    og.read_back();
    double state = 0;   // the per-event state before the holds ...
    for (auto &e : cloud) state += e.max_score + e.best_pr_x + e.best_pr_y;
    og.hold_field();
    dump(og, dir, "field", n);
    std::vector<double> cx, cy;
    og.filled_cell_grid(&cx, &cy);
    for (size_t i = 0; i < cx.size(); ++i) std::printf("cell %zu %.17g %.17g\n", i, cx[i], cy[i]);
    og.hold_field(cx, cy, BF_GLOBAL_HOLD_CELLS);
    dump(og, dir, "cells", n);
    og.hold_best();
    dump(og, dir, "best", n);
    std::vector<double> px, py;
    og.get_flow(nullptr, nullptr, nullptr, nullptr, &px, &py);
    og.read_back();
    double state2 = 0;   // ... and after them
    bool pr_same = px.size() == n;
    size_t i = 0;
    for (auto &e : cloud) {
        state2 += e.max_score + e.best_pr_x + e.best_pr_y;
        pr_same = pr_same && px[i] == e.best_pr_x && py[i] == e.best_pr_y;
        ++i;
    }
    std::printf("state kept=%d best pr same=%d\n", state == state2 ? 1 : 0, pr_same ? 1 : 0);
    // a refused grid leaves the held flow; set_cells ends a grid hold, not the best one
    int refused = 0;
    try {
        og.hold_field(std::vector<double>(cx.size() + 1, 0.0), cy);
    } catch (const bf::AccelError &e) {
        refused += e.code == BF_ERR_ARG ? 1 : 0;
    }
    std::vector<double> again;
    og.get_flow(nullptr, nullptr, nullptr, nullptr, &again, nullptr);
    std::printf("refused=%d held kept=%d\n", refused, again == px ? 1 : 0);
    og.hold_field(cx, cy);
    og.set_cells(64, 128, 16, 16);
    og.compute_flow_cells();   // (stages the new cells)
    std::printf("after set_cells state errors=%d\n", state_error([&] { og.flow_field(); }));
    return 0;
}
