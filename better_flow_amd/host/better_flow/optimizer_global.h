// optimizer_global.h -- the exhaustive (nx, ny) search (mirror of the reference's better_flow/optimizer_global.h:11-57 and
// optimizer_global.cpp).  Same constructors and public methods (project_all, compute_flow_bruteforce); every candidate's
// projection, saturating 8-bit image, Gaussian blur and per-event window score run on the GPU behind bf_global_* (batches
// of candidates per launch).  manual() (:153-185) is an OpenCV trackbar GUI and is not part of this path.
//
// Two definitions of this build (include/bf_accel.h, DESIGN.md "OptimizerGlobal"): each event's result is the candidate
// that gave its largest score (best_nx, best_ny; best_u / best_v = Event::compute_uv of it), and the slice's answer is the
// first candidate in sweep order with the largest S = sum of floor(score * 2^32).  The blur is this build's stated 8-bit
// Gaussian, not pinned to any OpenCV.
//
// A third: the objective per cell of a grid over the sensor (set_cells, compute_flow_cells; include/bf_accel.h), which
// answers with one candidate per cell where the slice-level search answers with one.  write_cell_flo writes that grid as a
// Middlebury .flo through bf::flo_payload / bf::write_flo (flow_field.h), with that writer's conventions: width =
// n_cell_y, height = n_cell_x, per cell float32 horizontal = best_v (columns) then vertical = best_u (rows), and the
// writer's unknown-flow value 1e9 in both for a cell with events == 0.
//
// A fourth: the per-cell search over a candidate set chosen on the device (compute_flow_cells_pyramid: a strided pass over
// the range's lattice, then windows around every cell's own best; compute_flow_cells_seeded: windows around the previous
// call's per-cell answers).  The seeds are lattice indices, so they carry from one OptimizerGlobal to the next only through
// get_seeds / set_seeds, and only over the same search range and cell grid: the grid is anchored at sensor pixel (0, 0), so
// a cell means the same pixels in every slice.
//
// A fifth: the piecewise projection (project_cells; include/bf_accel.h, bf_global_project_cells): the slice rendered and
// scored with every event under its own cell's (nx, ny) -- the compensated image and the objective S_pw of a per-cell
// answer.  It folds nothing into the per-event state.
//
// A sixth: the interpolated field (project_field; include/bf_accel.h, bf_global_project_field; the arithmetic is
// include/bf_global_field.h): project_cells with every event's (nx, ny) interpolated between the centres of the cells around
// its recorded address -- a smooth field instead of steps at the cell borders --, which also gives a flow per event
// (get_event_field).  project_field() takes the cell results after bf_field_fill: a cell with events == 0 or best_sum == 0
// carries no answer and takes the (nx, ny) of the nearest cell that does.  write_field_flo writes the field sampled at every
// sensor pixel as a .flo with write_cell_flo's conventions: width = res_y, height = res_x, horizontal = v, vertical = u.
//
// A seventh: the held flow (hold_field, hold_best; include/bf_accel.h, "the held flow"): the per-event flow of the piecewise
// projection, of the interpolated field or of the searches' best state kept on the device, where the renderers of the rolling
// optimiser and the -o table read it -- get_flow, flow_field, write_flow_flo, write_flow_ppm on the RES_X x RES_Y sensor, and
// emit_slice.  An upload, a new window and (for the two grid forms) set_cells end it; its readers throw (BF_ERR_STATE) then.
//
// Each object stages its slice on a device context of its OWN (not the thread's shared one that OptimizerLocal and
// OptimizerRolling use): the window and the per-event best state live there and accumulate over project_all /
// compute_flow_bruteforce calls, so no other optimiser on the thread may replace them.  Objects are not copyable.
#ifndef BF_HOST_OPTIMIZER_GLOBAL_H
#define BF_HOST_OPTIMIZER_GLOBAL_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>
#include <better_flow/datastructures.h>
#include <better_flow/event.h>
#include <better_flow/flow_field.h>
#include <better_flow/frame_writer.h>
#include <bf_global_field.h>

#include <algorithm>

#include <string>
#include <vector>

class OptimizerGlobal {
protected:
    struct OwnedContext {   // bf_create'd for this object alone; released with it
        bf_ctx *ctx = nullptr;
        ~OwnedContext() { if (ctx) bf_destroy(ctx); }
    };
    LinearEventCloud *events;
    OwnedContext own;       // (declared before accel: accel refers to it, and is gone first)
    AccelLib accel;
    bf::Image2D<uint8_t> project_img;
    std::vector<float> current_scores;   // scale_img_x x scale_img_y, row-major

    int scale;
    int metric_wsize;
    int scale_img_x, scale_img_y;
    int scale_bordered_img_x, scale_bordered_img_y;

    bf_global_search_opts range;
    bf_global_result result;
    std::vector<int64_t> surface;
    long long last_sum;

    int cells_res_x = 0, cells_res_y = 0, cell_rows = 0, cell_cols = 0;   // set_cells' arguments (0: not called)
    bool cells_staged = false;
    bf_global_cells cell_grid;
    std::vector<bf_global_cell_result> cell_results;                      // [n_cell_x][n_cell_y]
    std::vector<int64_t> seeds;                                           // per cell: a lattice index or -1 (empty: none)
    bf_global_pyramid_info pyramid_info;
    std::vector<int64_t> cell_sums;                                       // S_pw(cell) / S_f(cell) of the last project_cells / _field
    std::vector<double> field_nx, field_ny;                               // the grid of the last project_field, and its nz
    double field_nz = NZ;
    std::vector<double> event_field[4];                                   // per event: nx, ny, u, v of the last project_field

    void ensure_cells() {   // the slice, the window and the cell grid are on the device
        this->stage();
        if (!this->cells_staged) {
            accel.global_set_cells(cells_res_x, cells_res_y, cell_rows, cell_cols, &this->cell_grid);   // (throws before set_cells)
            this->cells_staged = true;
        }
    }
    void stage_cells() {    // ... for a search: its results start empty
        this->ensure_cells();
        this->cell_results.assign((size_t)cell_grid.n_cell_x * (size_t)cell_grid.n_cell_y, bf_global_cell_result());
        this->surface.clear();
    }
    void keep_seeds() {   // the answers of the cells that have events seed the next call
        this->seeds.assign(cell_results.size(), (int64_t)-1);
        for (size_t i = 0; i < cell_results.size(); ++i)
            if (cell_results[i].events > 0) this->seeds[i] = cell_results[i].best_index;
    }
    void search_pyramid(const bf_global_pyramid_opts &pyramid, const std::vector<int64_t> &from) {   // (after stage_cells)
        accel.global_search_cells_pyramid(this->range, pyramid, from, &this->result, &this->cell_results, nullptr,
                                          &this->pyramid_info);
        this->keep_seeds();
    }

    void stage() {   // the slice goes to the device once; the window resets every event's best state
        if (accel.is_staged()) return;
        if (!own.ctx) {
            const long long n = (long long)this->events->size();
            // (images of the sensor's size at least: the held flow's renders are RES_X x RES_Y)
            int rc = bf_create(bf::DeviceContext::device(), n > 1024 ? n : 1024, std::max(64, RES_X), std::max(64, RES_Y), nullptr,
                               &own.ctx);
            if (rc != BF_OK) {
                own.ctx = nullptr;
                throw bf::AccelError(rc, "OptimizerGlobal: bf_create failed (" + std::to_string(rc) + "): the search needs a "
                                         "HIP device (there is no CPU fallback)");
            }
        }
        accel.init_gpu_on(own.ctx, this->events);
        bf_global_window w;
        accel.global_set_window(this->scale, this->metric_wsize, &w);
        this->scale_img_x = w.scale_img_x; this->scale_img_y = w.scale_img_y;
        this->scale_bordered_img_x = w.scale_bordered_img_x; this->scale_bordered_img_y = w.scale_bordered_img_y;
        this->cells_staged = false;   // (a new window clears the cells)
    }

    void update_fields() {   // optimizer_global.cpp:187-205 (the device recomputes the same numbers in stage())
        assert(this->scale % 2 != 0);
        assert(this->metric_wsize % 2 != 0);
        bf_global_search_opts_default(&this->range);
        memset(&this->result, 0, sizeof(this->result));
        memset(&this->pyramid_info, 0, sizeof(this->pyramid_info));
        this->last_sum = 0;
        const bool empty = this->events->size() == 0;
        this->scale_img_x = empty ? 0 : (this->events->x_max - this->events->x_min + 1) * this->scale;
        this->scale_img_y = empty ? 0 : (this->events->y_max - this->events->y_min + 1) * this->scale;
        this->scale_bordered_img_x = this->scale_img_x + this->metric_wsize;
        this->scale_bordered_img_y = this->scale_img_y + this->metric_wsize;
    }

public:
    OptimizerGlobal(const OptimizerGlobal &) = delete;
    OptimizerGlobal &operator=(const OptimizerGlobal &) = delete;

    // optimizer_global.h:27-41
    OptimizerGlobal(LinearEventCloud *events_) : events(events_), scale(5), metric_wsize(21) { this->update_fields(); }
    OptimizerGlobal(LinearEventCloud *events_, int sc_) : events(events_), scale(sc_), metric_wsize(5 * sc_) {
        this->update_fields();
    }
    OptimizerGlobal(LinearEventCloud *events_, int sc_, int wsz_) : events(events_), scale(sc_), metric_wsize(wsz_) {
        this->update_fields();
    }

    // optimizer_global.cpp:4-79: one candidate; project_img and current_scores are refreshed, every accepted event's
    // best state folds in.  Returns S of the candidate.
    long long project_all(double nx_, double ny_, double nz_ = NZ) {
        this->stage();
        this->project_img = bf::Image2D<uint8_t>(scale_bordered_img_x, scale_bordered_img_y);
        this->current_scores.assign((size_t)scale_img_x * (size_t)scale_img_y, 0.0f);
        this->last_sum = accel.global_project_all(nx_, ny_, nz_, this->project_img.ptr(0),
                                                  this->current_scores.empty() ? nullptr : this->current_scores.data());
        return this->last_sum;
    }

    // optimizer_global.cpp:104-150 over the search range (the reference's defaults unless set_search_range was called),
    // continuing from the current per-event state.
    void compute_flow_bruteforce() {
        this->stage();
        long long nx = 0, ny = 0;   // the candidate counts of the reference's loops (:134-135), for the surface buffer
        if (this->range.x_step > 0 && this->range.y_step > 0) {
            for (double v = this->range.x_low; v < this->range.x_hi && nx <= (1ll << 26); v += this->range.x_step) ++nx;
            for (double v = this->range.y_low; v < this->range.y_hi && ny <= (1ll << 26); v += this->range.y_step) ++ny;
        }
        this->surface.assign(nx * ny > 0 && nx * ny <= (1ll << 26) ? (size_t)(nx * ny) : 0, 0);
        accel.global_search(this->range, &this->result, &this->surface);
    }

    // A grid of cell_rows x cell_cols-pixel cells over the res_x x res_y sensor, anchored at pixel (0, 0), for
    // compute_flow_cells.
    void set_cells(int res_x, int res_y, int cell_rows_, int cell_cols_) {
        this->cells_res_x = res_x; this->cells_res_y = res_y; this->cell_rows = cell_rows_; this->cell_cols = cell_cols_;
        this->cells_staged = false;
        this->cell_results.clear();
    }

    // compute_flow_bruteforce with the objective kept per cell: the slice's result as there (from the sum over the cells),
    // one result per cell, and the same per-event state.  No surface is kept.
    void compute_flow_cells() {
        this->stage_cells();
        accel.global_search_cells(this->range, &this->result, &this->cell_results, nullptr);
    }

    // compute_flow_cells over a strided pass and pyramid.levels - 1 refinements (bf_global_search_cells_pyramid without
    // seeds).  Its answers become the seeds of compute_flow_cells_seeded.
    void compute_flow_cells_pyramid(const bf_global_pyramid_opts &pyramid) {
        this->stage_cells();
        this->search_pyramid(pyramid, std::vector<int64_t>());
    }

    // pyramid.levels windows around the seeds (the last pyramid / seeded call's per-cell best_index, or set_seeds); without
    // a seed, the unseeded pyramid.  Keeps its answers as the next seeds.  Throws (BF_ERR_ARG) when no seeded cell has an
    // event in this slice: clear_seeds() and call again.
    void compute_flow_cells_seeded(const bf_global_pyramid_opts &pyramid) {
        this->stage_cells();
        bool any = false;
        if (this->seeds.size() == this->cell_results.size())
            for (size_t i = 0; i < seeds.size(); ++i) any = any || seeds[i] >= 0;
        this->search_pyramid(pyramid, any ? this->seeds : std::vector<int64_t>());
    }

    // The piecewise projection under one (nx, ny) per cell, row-major [n_cell_x][n_cell_y] (the entry of a cell without
    // events is not read): project_img and current_scores are refreshed like project_all, the per-event state is not
    // touched.  Returns S_pw and keeps the per-cell sums (get_cell_sums).
    long long project_cells(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, double nz_ = NZ) {
        this->ensure_cells();
        this->project_img = bf::Image2D<uint8_t>(scale_bordered_img_x, scale_bordered_img_y);
        this->current_scores.assign((size_t)scale_img_x * (size_t)scale_img_y, 0.0f);
        this->last_sum = accel.global_project_cells(cell_nx, cell_ny, nz_, this->project_img.ptr(0),
                                                    this->current_scores.empty() ? nullptr : this->current_scores.data(),
                                                    &this->cell_sums);
        return this->last_sum;
    }

    // ... under the answers of the last compute_flow_cells / _pyramid / _seeded call (cell_results' best_nx, best_ny, with
    // the search range's nz).  Throws when there are none.
    long long project_cells() {
        if (this->cell_results.empty())
            throw bf::AccelError(BF_ERR_STATE, "OptimizerGlobal::project_cells: no per-cell results (call compute_flow_cells first)");
        std::vector<double> cx(cell_results.size()), cy(cell_results.size());
        for (size_t i = 0; i < cell_results.size(); ++i) { cx[i] = cell_results[i].best_nx; cy[i] = cell_results[i].best_ny; }
        return this->project_cells(cx, cy, this->range.nz);
    }
    const std::vector<int64_t> &get_cell_sums() const { return cell_sums; }   // [n_cell_x][n_cell_y]

    // The interpolated field under one (nx, ny) per cell, row-major [n_cell_x][n_cell_y]; every entry is read and must be
    // finite.  Refreshes project_img, current_scores, the per-cell sums (get_cell_sums) and the per-event field
    // (get_event_field); the per-event best state is not touched.  Returns S_f.  A refused grid leaves the previous
    // results in place.
    long long project_field(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, double nz_ = NZ) {
        this->ensure_cells();
        bf::Image2D<uint8_t> img(scale_bordered_img_x, scale_bordered_img_y);
        std::vector<float> scores((size_t)scale_img_x * (size_t)scale_img_y, 0.0f);
        const long long S = accel.global_project_field(cell_nx, cell_ny, nz_, img.ptr(0), scores.empty() ? nullptr : scores.data(),
                                                       &this->cell_sums, this->event_field);
        this->project_img = img;
        this->current_scores.swap(scores);
        this->field_nx = cell_nx; this->field_ny = cell_ny; this->field_nz = nz_;
        this->last_sum = S;
        return S;
    }

    // ... under the answers of the last compute_flow_cells / _pyramid / _seeded call after the fill (bf_field_fill: a cell
    // is valid when events > 0 and best_sum > 0), with the search range's nz.  Throws when there are none.
    long long project_field() {
        if (this->cell_results.empty())
            throw bf::AccelError(BF_ERR_STATE, "OptimizerGlobal::project_field: no per-cell results (call compute_flow_cells first)");
        std::vector<double> cx, cy;
        this->filled_cell_grid(&cx, &cy);
        return this->project_field(cx, cy, this->range.nz);
    }

    // The cell results' (best_nx, best_ny) with the cells that carry no answer filled from their nearest valid neighbour
    void filled_cell_grid(std::vector<double> *cx, std::vector<double> *cy) const {
        const size_t nc = cell_results.size();
        std::vector<uint8_t> valid(nc);
        cx->assign(nc, 0.0); cy->assign(nc, 0.0);
        for (size_t i = 0; i < nc; ++i) {
            valid[i] = cell_results[i].events > 0 && cell_results[i].best_sum > 0 ? 1 : 0;
            (*cx)[i] = cell_results[i].best_nx; (*cy)[i] = cell_results[i].best_ny;
        }
        if (nc) bf_field_fill(cell_grid.n_cell_x, cell_grid.n_cell_y, valid.data(), cx->data(), cy->data());
    }

    // Per event, in the cloud's order: the interpolated nx (k = 0), ny (1) and compute_uv of them, u (2), v (3), of the
    // last project_field.
    const std::vector<double> &get_event_field(int k) const { return event_field[k]; }
    const std::vector<double> &get_field_nx() const { return field_nx; }   // the grid of the last project_field
    const std::vector<double> &get_field_ny() const { return field_ny; }

    // The field of the last project_field sampled at every pixel of the res_x x res_y sensor of set_cells, as a .flo (the
    // conventions are at the top of this file): per pixel Event::compute_uv of the interpolated (nx, ny).
    bool write_field_flo(const std::string &path) const {
        if (field_nx.empty() || field_nx.size() != (size_t)cell_grid.n_cell_x * (size_t)cell_grid.n_cell_y) return false;
        bf::FlowField f(cells_res_x, cells_res_y);
        for (int x = 0; x < cells_res_x; ++x)
            for (int y = 0; y < cells_res_y; ++y) {
                double nx, ny;
                bf_field_at((uint32_t)x, (uint32_t)y, (uint32_t)cell_rows, (uint32_t)cell_cols, (uint32_t)cell_grid.n_cell_x,
                            (uint32_t)cell_grid.n_cell_y, field_nx.data(), field_ny.data(), &nx, &ny);
                const size_t at = (size_t)x * cells_res_y + y;
                f.owner[at] = 0;
                bf_field_uv(nx, ny, field_nz, &f.u[at], &f.v[at]);
            }
        const std::vector<float> payload = bf::flo_payload(f);
        return bf::write_flo(path, f.rows, f.cols, payload.data());
    }

    // Keeps the per-event flow of project_cells (mode BF_GLOBAL_HOLD_CELLS) or project_field (BF_GLOBAL_HOLD_FIELD) under the
    // given grids on the device, without rendering or scoring anything; grids and refusals as there.
    void hold_field(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, int mode = BF_GLOBAL_HOLD_FIELD,
                    double nz_ = NZ) {
        this->ensure_cells();
        accel.global_hold_field(cell_nx, cell_ny, nz_, mode);
    }

    // ... the smooth form under the answers of the last compute_flow_cells / _pyramid / _seeded call after the fill, with the
    // search range's nz: the flow project_field() renders.  Throws when there are none.
    void hold_field() {
        if (this->cell_results.empty())
            throw bf::AccelError(BF_ERR_STATE, "OptimizerGlobal::hold_field: no per-cell results (call compute_flow_cells first)");
        std::vector<double> cx, cy;
        this->filled_cell_grid(&cx, &cy);
        this->hold_field(cx, cy, BF_GLOBAL_HOLD_FIELD, this->range.nz);
    }

    // Keeps a snapshot of every event's best candidate so far (what read_back returns); later searches do not change it.
    void hold_best() {
        this->stage();
        accel.global_hold_best();
    }

    // The held flow per event, in the cloud's order; each vector may be null.  (This and every reader below throw
    // BF_ERR_STATE without a held flow.)
    void get_flow(std::vector<double> *nx, std::vector<double> *ny, std::vector<double> *u, std::vector<double> *v,
                  std::vector<double> *pr_x = nullptr, std::vector<double> *pr_y = nullptr) {
        std::vector<double> *out[6] = {nx, ny, u, v, pr_x, pr_y};
        double *p[6];
        for (int k = 0; k < 6; ++k) {
            if (out[k]) out[k]->assign(this->events->size(), 0.0);
            p[k] = out[k] && !out[k]->empty() ? out[k]->data() : nullptr;
        }
        this->stage();
        accel.global_get_flow(p[0], p[1], p[2], p[3], p[4], p[5]);
    }

    // The per-pixel field of the held flow on the RES_X x RES_Y sensor: the last event of the cloud that lands on a pixel
    // owns it (AccelLib::flow_field's rule, every event taking part).
    bf::FlowField flow_field() {
        this->stage();
        return accel.global_flow_field();
    }

    // ... as a Middlebury .flo (flow_field.h's writer and conventions), and the flow frame of the held flow -- held positions |
    // colour-coded flow | raw events -- as a PPM (frame_writer.h), composed on the device.
    bool write_flow_flo(const std::string &path) {
        const bf::FlowField f = this->flow_field();
        const std::vector<float> payload = bf::flo_payload(f);
        return bf::write_flo(path, f.rows, f.cols, payload.data());
    }
    bool write_flow_ppm(const std::string &path) {
        std::vector<uint8_t> ppm((size_t)RES_X * (size_t)(3 * RES_Y) * 3);
        this->stage();
        accel.global_render_flow_frame(ppm.data(), nullptr, nullptr);
        return bf::write_ppm_raw(path, RES_X, 3 * RES_Y, ppm.data());
    }

    // The slice's rows of the -o table into `emit` (bf_emit_create on own_context()) with the held flow as their (u, v):
    // bf_emit_slice's arguments, rule and ticket (wait and release with bf_emit_wait / bf_emit_release).
    int64_t emit_slice(bf_emit *emit, uint64_t first, uint64_t start_time, bool lead = false, uint64_t lead_t = 0, int lead_row = 0,
                       int lead_col = 0) {
        this->stage();
        return accel.global_emit_slice(emit, first, start_time, lead, lead_t, lead_row, lead_col);
    }
    bf_ctx *own_context() {   // (staged: the context exists)
        this->stage();
        return own.ctx;
    }

    void clear_seeds() { this->seeds.clear(); }
    const std::vector<int64_t> &get_seeds() const { return seeds; }
    void set_seeds(const std::vector<int64_t> &s) { this->seeds = s; }   // e.g. the previous slice's OptimizerGlobal::get_seeds
    const bf_global_pyramid_info &get_pyramid_info() const { return pyramid_info; }

    int get_n_cell_x() const { return cell_results.empty() ? 0 : cell_grid.n_cell_x; }
    int get_n_cell_y() const { return cell_results.empty() ? 0 : cell_grid.n_cell_y; }
    const std::vector<bf_global_cell_result> &get_cell_results() const { return cell_results; }   // [n_cell_x][n_cell_y]
    const bf_global_cell_result &get_cell(int cx, int cy) const { return cell_results[(size_t)cx * cell_grid.n_cell_y + cy]; }

    // The per-cell (best_u, best_v) of the last compute_flow_cells as a .flo (the conventions are at the top of this file).
    bool write_cell_flo(const std::string &path) const {
        bf::FlowField f(this->get_n_cell_x(), this->get_n_cell_y());
        for (size_t i = 0; i < cell_results.size(); ++i) {
            if (cell_results[i].events == 0) continue;   // owner -1: the writer's unknown flow
            f.owner[i] = 0; f.u[i] = cell_results[i].best_u; f.v[i] = cell_results[i].best_v;
        }
        const std::vector<float> payload = bf::flo_payload(f);
        return bf::write_flo(path, f.rows, f.cols, payload.data());
    }

    // The search range (optimizer_global.cpp:106-108 hard-codes x in [-0.09, 0.09), y in [-0.04, 0.04), step 0.001:
    // about +-71 x +-31 px/s).
    void set_search_range(double x_low, double x_hi, double x_step, double y_low, double y_hi, double y_step,
                          double nz = NZ) {
        this->range.x_low = x_low; this->range.x_hi = x_hi; this->range.x_step = x_step;
        this->range.y_low = y_low; this->range.y_hi = y_hi; this->range.y_step = y_step;
        this->range.nz = nz;
    }

    double get_best_nx() const { return result.best_nx; }
    double get_best_ny() const { return result.best_ny; }
    long long get_best_sum() const { return (long long)result.best_sum; }
    long long get_n_x() const { return (long long)result.n_x; }
    long long get_n_y() const { return (long long)result.n_y; }
    long long get_last_sum() const { return last_sum; }
    const std::vector<int64_t> &get_surface() const { return surface; }   // S per candidate, [n_x][n_y]
    const bf::Image2D<uint8_t> &get_project_img() const { return project_img; }
    const std::vector<float> &get_current_scores() const { return current_scores; }

    // The per-event state into the cloud's Event fields: max_score, best_pr_x / _y, best_u / _v (compute_uv of the
    // event's winning candidate).
    void read_back() {
        this->stage();
        const size_t n = this->events->size();
        std::vector<double> ms(n), px(n), py(n), u(n), v(n);
        if (n) accel.global_get_events(ms.data(), nullptr, nullptr, px.data(), py.data(), u.data(), v.data());
        size_t i = 0;
        for (auto &e : *this->events) {
            e.max_score = ms[i]; e.best_pr_x = px[i]; e.best_pr_y = py[i]; e.best_u = u[i]; e.best_v = v[i];
            ++i;
        }
    }
};

#endif  // BF_HOST_OPTIMIZER_GLOBAL_H
