// accel_lib.h -- the operator API of the motion-compensation path (mirror of the reference's
// `class AccelLib`, better_flow/accel_lib.h:14-616), implemented over the C-ABI of
// libbf_accel.so (include/bf_accel.h): every operator runs on the MI355X.  There is no CPU
// branch: `gpu_enabled` is always true and a missing device is a hard error.
//
// Differences that are forced by the device path (all documented in INTEGRATION.md):
//   * images are bf::Image2D<float> (row-major, rows x cols) instead of cv::Mat;
//   * init_gpu() only remembers the cloud; the slice is staged by sync() once the local
//     time has been set (the reference re-uploads `t` on every projection, accel_lib.h:284-289);
//   * one device context is shared by all AccelLib objects of a thread and reused across
//     slices (the reference allocates per slice, accel_lib.h:86-115).
#ifndef BF_HOST_ACCEL_LIB_H
#define BF_HOST_ACCEL_LIB_H

#include <better_flow/event.h>
#include <better_flow/clustering.h>
#include <better_flow/flow_field.h>
#include <better_flow/object_model.h>
#include <better_flow/object_tasks.h>   // bf::ObjectTasks and the weak declarations of bf_set_groups / bf_run_groups
#include <better_flow/motion_assign.h>  // bf::MotionAssigner and the weak declaration of bf_assign_groups
#include <bf_accel.h>

#include <stdexcept>
#include <string>

namespace bf {

// A failed call of the C-ABI (include/bf_accel.h) as a C++ exception: `code` is the bf_* return code (BF_ERR_*), what()
// the context's last error text.  Nothing in the host front end terminates the process; the command line catches this
// at top level, a library user wherever it likes.
struct AccelError : std::runtime_error {
    int code;
    AccelError(int code_, const std::string &msg) : std::runtime_error(msg), code(code_) {}
};

template <class T> struct Image2D {
    int rows = 0, cols = 0;
    std::vector<T> data;
    Image2D() {}
    Image2D(int r, int c) : rows(r), cols(c), data((size_t)r * (size_t)c) {}
    T &at(int r, int c) { return data[(size_t)r * cols + c]; }
    const T &at(int r, int c) const { return data[(size_t)r * cols + c]; }
    T *ptr(int r) { return &data[(size_t)r * cols]; }
};

// Process-wide device context, created on first use and grown on demand.
class DeviceContext {
public:
    static int &device() {
        static int d = 0;
        return d;
    }
    static bf_ctx *get(long long events, int rows, int cols) {
        State &s = state();
        if (s.ctx && events <= s.events && (long long)rows * cols <= (long long)s.rows * s.cols) return s.ctx;
        if (s.ctx) bf_destroy(s.ctx);
        s.ctx = nullptr;
        s.events = events > s.events ? events : s.events;
        if ((long long)rows * cols > (long long)s.rows * s.cols) { s.rows = rows; s.cols = cols; }
        int rc = bf_create(device(), s.events, s.rows, s.cols, nullptr, &s.ctx);
        if (rc != BF_OK) {
            s.ctx = nullptr;
            throw AccelError(rc, "bf_create failed (" + std::to_string(rc) + "): the motion-compensation path needs a HIP "
                                 "device (there is no CPU fallback)");
        }
        return s.ctx;
    }
    static void release() {
        State &s = state();
        if (s.ctx) bf_destroy(s.ctx);
        s.ctx = nullptr;
    }

private:
    struct State {
        bf_ctx *ctx = nullptr;
        long long events = 0;
        int rows = 0, cols = 0;
        ~State() { if (ctx) bf_destroy(ctx); }
    };
    static State &state() {
        static thread_local State s;
        return s;
    }
};

}  // namespace bf

class AccelLib {
private:
    bf_ctx *ctx;
    size_t size;   // number of events staged
    bool staged;
    std::vector<uint8_t> noise_staged;   // Event::noise as uploaded (empty: none) -- the host composition of the flow field reads it
    size_t global_n_cells = 0;           // n_cell_x * n_cell_y of the last global_set_cells (0: none)

    void check(int rc, const char *what) const {
        if (rc < 0)
            throw bf::AccelError(rc, std::string("AccelLib::") + what + " failed (" + std::to_string(rc) + "): " +
                                         (ctx ? bf_last_error(ctx) : "no ctx"));
    }
    // the candidate grids of global_project_cells / global_project_field: one entry per cell of the last global_set_cells
    // (without cells the library refuses, BF_ERR_ARG, before it reads a buffer)
    void check_cell_grids(const char *who, const std::vector<double> &cell_nx, const std::vector<double> &cell_ny) const {
        if (global_n_cells && (cell_nx.size() != global_n_cells || cell_ny.size() != global_n_cells))
            throw bf::AccelError(BF_ERR_ARG, std::string("AccelLib::") + who + ": grids of " + std::to_string(cell_nx.size()) +
                                                 " and " + std::to_string(cell_ny.size()) + " entries for " +
                                                 std::to_string(global_n_cells) + " cells");
    }

public:
    bool gpu_enabled;   // accel_lib.h:41 -- here: always true

    AccelLib() : ctx(nullptr), size(0), staged(false), gpu_enabled(true) {}

    bool is_staged() const { return staged; }
    bf_ctx *context() const { return ctx; }

    // AccelLib::init_gpu, accel_lib.h:71-145.  Stages the slice: AoS -> SoA (int fr_x, fr_y, t as
    // at :83-85,:101-103) and one upload.  Event::t must already hold the slice-local time.
    template <class T> inline void init_gpu(T *events, int nRows, int nCols) {
        this->size = events->size();
        this->ctx = bf::DeviceContext::get((long long)(size > 1024 ? size : 1024), nRows > 64 ? nRows : 64,
                                           nCols > 64 ? nCols : 64);
        this->upload(events);
    }

    // The same staging on a context the caller created and owns (bf_create), which no other object uses: for state that
    // must outlive other optimisers on the thread (OptimizerGlobal's per-event state and window).
    template <class T> inline void init_gpu_on(bf_ctx *own, T *events) {
        this->size = events->size();
        this->ctx = own;
        this->upload(events);
    }

private:
    template <class T> inline void upload(T *events) {
        std::vector<int32_t> fx(size), fy(size), ft(size);
        std::vector<uint8_t> noise(size);
        bool any_noise = false;
        size_t i = 0;
        for (auto &e : *events) {
            fx[i] = (int32_t)e.fr_x;
            fy[i] = (int32_t)e.fr_y;
            if (e.t > (sll)INT32_MAX || e.t <= (sll)INT32_MIN)
                throw bf::AccelError(BF_ERR_ARG, "AccelLib::init_gpu: slice-local time " + std::to_string((long long)e.t) +
                                                     " ns does not fit 32 bits (slices span at most 2.1 s)");
            ft[i] = (int32_t)e.t;
            noise[i] = e.noise ? 1 : 0;
            any_noise |= e.noise;
            ++i;
        }
        check(bf_upload_events(ctx, fx.data(), fy.data(), ft.data(), any_noise ? noise.data() : nullptr,
                               (int64_t)size), "init_gpu");
        this->staged = true;
        if (!any_noise) noise.clear();
        this->noise_staged.swap(noise);
    }

public:

    // OptimizerRolling::set_cloud's device half: bounding box, window, Event::reset on the device.
    inline bf_window set_window(int scale) {
        bf_window w;
        check(bf_set_cloud(ctx, scale, RES_X, RES_Y, &w), "set_window");
        return w;
    }

    // accel_lib.h:211-217 -> :147-178.  w, h, scale, x_sh, y_sh are implied by the window that
    // set_window() computed from the same events (they are asserted to agree).
    template <class T>
    inline bf::Image2D<float> get_time_img(T * /*events*/, int w, int h, int scale, int /*x_sh*/, int /*y_sh*/) {
        bf::Image2D<float> img(w + scale, h + scale);
        check(bf_get_time_img(ctx, img.data.data(), nullptr), "get_time_img");
        return img;
    }

    inline bf::Image2D<uint32_t> get_count_img(int w, int h, int scale) {
        bf::Image2D<uint32_t> img(w + scale, h + scale);
        check(bf_get_time_img(ctx, nullptr, img.data.data()), "get_count_img");
        return img;
    }

    // accel_lib.h:275-281: the incremental form (its only call in the reference is commented out, optimizer_rolling.h:333-339)
    template <class T>
    inline void project_4param(T * /*events*/, double dnx_, double dny_, double cx, double cy, double div, double crl) {
        check(bf_project_4param(ctx, dnx_, dny_, cx, cy, div, crl), "project_4param");
    }

    // accel_lib.h:263-267
    template <class T>
    inline void project_4param_reinit(T * /*events*/, double dnx_, double dny_, double cx, double cy, double div,
                                      double crl) {
        check(bf_project_4param_reinit(ctx, dnx_, dny_, cx, cy, div, crl), "project_4param_reinit");
    }

    // accel_lib.h:310-329: copy pr / n back into the events.
    template <class T> inline void writeout_events(T *events) {
        if (!staged || size == 0) return;
        std::vector<double> px(size), py(size), nx(size), ny(size);
        check(bf_writeout_events(ctx, px.data(), py.data(), nx.data(), ny.data()), "writeout_events");
        size_t i = 0;
        for (auto &e : *events) {
            e.pr_x = px[i]; e.pr_y = py[i];
            e.nx = nx[i]; e.ny = ny[i];
            ++i;
        }
    }

    // Event::compute_uv (event.h:135-142) for every event, evaluated on the device.
    template <class T> inline void compute_uv(T *events) {
        if (!staged || size == 0) return;
        std::vector<double> u(size), v(size);
        check(bf_compute_uv(ctx, u.data(), v.data()), "compute_uv");
        size_t i = 0;
        for (auto &e : *events) {
            e.set_uv(u[i], v[i]);
            ++i;
        }
    }

    // accel_lib.h:337-341
    void fast_model(ObjectModel &model, bf::Image2D<float> &time_img) {
        bf_model m = model.to_abi();
        check(bf_fast_model(ctx, time_img.data.data(), time_img.rows, time_img.cols, &m), "fast_model");
        model.cx = m.cx; model.cy = m.cy; model.dx = m.dx; model.dy = m.dy;
        model.rot = m.rot; model.div = m.div; model.cnt = m.cnt;
    }
    ObjectModel fast_model(bf::Image2D<float> &time_img) {
        ObjectModel model;
        this->fast_model(model, time_img);
        return model;
    }

    // accel_lib.h:400-432 / :513-543
    void Sobel(bf::Image2D<float> &img, bf::Image2D<float> &grad_x, bf::Image2D<float> &grad_y) {
        if (!ctx) ctx = bf::DeviceContext::get(1024, img.rows, img.cols);
        grad_x = bf::Image2D<float>(img.rows, img.cols);
        grad_y = bf::Image2D<float>(img.rows, img.cols);
        check(bf_sobel(ctx, img.data.data(), img.rows, img.cols, grad_x.data.data(), grad_y.data.data()), "Sobel");
    }

    // OptimizerRolling::set_model's warp (optimizer_rolling.h:294-298)
    void set_model(const ObjectModel &m) {
        bf_model a = m.to_abi();
        check(bf_set_model(ctx, &a), "set_model");
    }

    // EventFile::projection_img (event_file.h:460-515) of the staged slice: the 8-bit event image at the current
    // projected positions (motion compensated once run() has converged) or, show_final, at the sensor positions.
    bf::Image2D<uint8_t> projection_img(int scale, bool show_final) {
        bf::Image2D<uint8_t> img(RES_X * scale, RES_Y * scale);
        check(bf_projection_img(ctx, scale, RES_X, RES_Y, show_final ? 1 : 0, img.ptr(0)), "projection_img");
        return img;
    }

    // EventFile::color_time_img (event_file.h:649-747) of the staged slice: B, G, R bytes, (RES_X * scale + scale) x
    // (RES_Y * scale + scale) pixels; hue = phase of the events' time in the slice
    std::vector<uint8_t> color_time_img(int scale, bool show_final, int *rows, int *cols) {
        const int sc = scale ? scale : 11;
        *rows = RES_X * sc + sc; *cols = RES_Y * sc + sc;
        std::vector<uint8_t> img((size_t)*rows * (size_t)*cols * 3);
        check(bf_color_time_img(ctx, scale, RES_X, RES_Y, show_final ? 1 : 0, img.data()), "color_time_img");
        return img;
    }

    // The per-pixel flow field of the staged slice (bf_flow_field): RES_X x RES_Y owner indices and (best_u, best_v).  The
    // events were uploaded in the cloud's iteration order, which is the order EventFile::color_flow_img walks them in
    // (event_file.h:321), so the last uploaded event on a pixel owns it: BF_FLOW_LAST_UPLOADED.
    bf::FlowField flow_field() {
        bf::FlowField f(RES_X, RES_Y);
        if (bf_flow_field) check(bf_flow_field(ctx, RES_X, RES_Y, BF_FLOW_LAST_UPLOADED, f.owner.data(), f.u.data(), f.v.data()), "flow_field");
        else check(bf::flow_field_from_readbacks(ctx, size, noise_staged.empty() ? nullptr : noise_staged.data(), RES_X, RES_Y,
                                                 BF_FLOW_LAST_UPLOADED, f), "flow_field");
        return f;
    }

    // The segmentation of the staged slice under window w (bf::Segmenter: the device entries, or the host path on read-backs)
    bf::Segmentation segmentation(const bf::Segmenter &seg, const bf_window &w) {
        bf::Segmentation out;
        check(seg.run(ctx, w, size, noise_staged.empty() ? nullptr : noise_staged.data(), out), "segmentation");
        return out;
    }

    // EventFile::color_flow_img (event_file.h:318-350) of the staged slice: RES_X x RES_Y pixels of B, G, R bytes
    std::vector<uint8_t> color_flow_img() {
        if (!bf_color_flow_img) return bf::color_flow_img_of(flow_field());
        std::vector<uint8_t> img((size_t)RES_X * (size_t)RES_Y * 3);
        check(bf_color_flow_img(ctx, RES_X, RES_Y, BF_FLOW_LAST_UPLOADED, img.data(), nullptr), "color_flow_img");
        return img;
    }

    // OptimizerLocal on the device (optimizer_sampler.h:29-48; optimizer_sampler.cpp:4-38,120-153)
    void local_set_window(int scale, int wsz, int c_fr_x, int c_fr_y, long long c_t, bf_local_window *w) {
        check(bf_local_set_window(ctx, scale, wsz, c_fr_x, c_fr_y, c_t, w), "local_set_window");
    }
    double local_iteration_step(double nx, double ny, uint8_t *img_out) {
        double score = 0;
        check(bf_local_iteration_step(ctx, nx, ny, &score, img_out), "local_iteration_step");
        return score;
    }
    int local_run(bf_local_state *st) {
        int rc = bf_local_run(ctx, RES_X, RES_Y, 0, st);
        check(rc, "local_run");
        return rc;
    }

    // OptimizerGlobal on the device (optimizer_global.h:27-41; optimizer_global.cpp:4-150)
    void global_set_window(int scale, int metric_wsize, bf_global_window *w) {
        this->global_n_cells = 0;   // (a new window clears the cells)
        check(bf_global_set_window(ctx, scale, metric_wsize, w), "global_set_window");
    }
    long long global_project_all(double nx, double ny, double nz, uint8_t *img_out, float *scores_out) {
        int64_t sum = 0;
        check(bf_global_project_all(ctx, nx, ny, nz, img_out, scores_out, &sum), "global_project_all");
        return (long long)sum;
    }
    void global_search(const bf_global_search_opts &o, bf_global_result *r, std::vector<int64_t> *surface) {
        int64_t *sp = nullptr;
        int64_t cap = 0;
        if (surface && !surface->empty()) { sp = surface->data(); cap = (int64_t)surface->size(); }
        check(bf_global_search(ctx, &o, r, sp, cap), "global_search");
    }
    // the objective per cell of a grid over the sensor (include/bf_accel.h: bf_global_set_cells, bf_global_search_cells)
    void global_set_cells(int res_x, int res_y, int cell_rows, int cell_cols, bf_global_cells *g) {
        this->global_n_cells = 0;
        check(bf_global_set_cells(ctx, res_x, res_y, cell_rows, cell_cols, g), "global_set_cells");
        this->global_n_cells = (size_t)g->n_cell_x * (size_t)g->n_cell_y;
    }
    void global_search_cells(const bf_global_search_opts &o, bf_global_result *r, std::vector<bf_global_cell_result> *cells,
                             std::vector<int64_t> *cell_surface) {
        int64_t *sp = nullptr;
        int64_t cap = 0;
        if (cell_surface && !cell_surface->empty()) { sp = cell_surface->data(); cap = (int64_t)cell_surface->size(); }
        check(bf_global_search_cells(ctx, &o, r, cells ? cells->data() : nullptr, cells ? (int64_t)cells->size() : 0, sp, cap),
              "global_search_cells");
    }
    // ... over a candidate set decided on the device (bf_global_search_cells_pyramid); seeds: empty, or one lattice index
    // (or -1) per cell.  evaluated (may be null) is resized to what was evaluated.
    void global_search_cells_pyramid(const bf_global_search_opts &o, const bf_global_pyramid_opts &p,
                                     const std::vector<int64_t> &seeds, bf_global_result *r,
                                     std::vector<bf_global_cell_result> *cells, std::vector<int64_t> *evaluated,
                                     bf_global_pyramid_info *info) {
        bf_global_pyramid_info local;
        if (!info) info = &local;
        check(bf_global_search_cells_pyramid(ctx, &o, &p, seeds.empty() ? nullptr : seeds.data(), r,
                                             cells ? cells->data() : nullptr, cells ? (int64_t)cells->size() : 0,
                                             evaluated ? evaluated->data() : nullptr, evaluated ? (int64_t)evaluated->size() : 0,
                                             nullptr, 0, info),
              "global_search_cells_pyramid");
        if (evaluated) evaluated->resize((size_t)info->evaluated);
    }
    // the piecewise projection (bf_global_project_cells): one (nx, ny) per cell of the last global_set_cells' grid,
    // row-major; grids of any other length are refused (BF_ERR_ARG) before the library is called.  cell_sums (may be null)
    // is resized to that grid.  Returns S_pw.
    long long global_project_cells(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, double nz,
                                   uint8_t *img_out, float *scores_out, std::vector<int64_t> *cell_sums) {
        check_cell_grids("global_project_cells", cell_nx, cell_ny);
        int64_t sum = 0;
        if (cell_sums) cell_sums->assign(global_n_cells, 0);
        check(bf_global_project_cells(ctx, cell_nx.data(), cell_ny.data(), (int64_t)global_n_cells, nz, img_out, scores_out, &sum,
                                      cell_sums ? cell_sums->data() : nullptr, (int64_t)global_n_cells),
              "global_project_cells");
        return (long long)sum;
    }
    // the interpolated field (bf_global_project_field): global_project_cells with every event's (nx, ny) interpolated
    // between the cell centres; the whole grid is read.  events (may be null): four vectors, resized to the slice --
    // the per-event nx, ny (interpolated) and u, v (compute_uv of them).  Returns S_f.
    long long global_project_field(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, double nz,
                                   uint8_t *img_out, float *scores_out, std::vector<int64_t> *cell_sums,
                                   std::vector<double> *events) {
        check_cell_grids("global_project_field", cell_nx, cell_ny);
        int64_t sum = 0;
        std::vector<int64_t> sums(cell_sums ? global_n_cells : 0, 0);
        std::vector<double> ev[4];
        for (int k = 0; events && k < 4; ++k) ev[k].assign((size_t)size, 0.0);
        double *ep[4];
        for (int k = 0; k < 4; ++k) ep[k] = events && size ? ev[k].data() : nullptr;
        check(bf_global_project_field(ctx, cell_nx.data(), cell_ny.data(), (int64_t)global_n_cells, nz, img_out, scores_out, &sum,
                                      cell_sums ? sums.data() : nullptr, (int64_t)global_n_cells, ep[0], ep[1], ep[2], ep[3]),
              "global_project_field");
        if (cell_sums) cell_sums->swap(sums);   // (a refused call leaves the caller's vectors as they were)
        for (int k = 0; events && k < 4; ++k) events[k].swap(ev[k]);
        return (long long)sum;
    }
    void global_get_events(double *max_score, double *best_nx, double *best_ny, double *best_pr_x, double *best_pr_y,
                           double *best_u, double *best_v) {
        check(bf_global_get_events(ctx, max_score, best_nx, best_ny, best_pr_x, best_pr_y, best_u, best_v), "global_get_events");
    }
    // The held flow (include/bf_accel.h, "the held flow"): the search's per-event flow kept on the device -- under one
    // (nx, ny) per cell (mode BF_GLOBAL_HOLD_CELLS: the event's cell's; BF_GLOBAL_HOLD_FIELD: interpolated at its address; grids
    // as in global_project_cells) or as a snapshot of the per-event best state -- and what reads it.
    void global_hold_field(const std::vector<double> &cell_nx, const std::vector<double> &cell_ny, double nz, int mode) {
        check_cell_grids("global_hold_field", cell_nx, cell_ny);
        check(bf_global_hold_field(ctx, cell_nx.data(), cell_ny.data(), (int64_t)global_n_cells, nz, mode), "global_hold_field");
    }
    void global_hold_best() { check(bf_global_hold_best(ctx), "global_hold_best"); }
    // n doubles each, in the cloud's order; each may be null
    void global_get_flow(double *nx, double *ny, double *u, double *v, double *pr_x, double *pr_y) {
        check(bf_global_get_flow(ctx, nx, ny, u, v, pr_x, pr_y), "global_get_flow");
    }
    // flow_field() of the held flow: every event takes part, a pixel's (u, v) is its owner's held flow
    bf::FlowField global_flow_field() {
        bf::FlowField f(RES_X, RES_Y);
        check(bf_global_flow_field(ctx, RES_X, RES_Y, BF_FLOW_LAST_UPLOADED, f.owner.data(), f.u.data(), f.v.data()), "global_flow_field");
        return f;
    }
    // the flow frame of the held flow (held positions | colour-coded flow | raw events), composed on the device: the PPM
    // payload (RES_X x 3 RES_Y x 3 bytes, top-down RGB), the AVI payload and the .flo payload; each may be null, not all
    void global_render_flow_frame(uint8_t *ppm_out, uint8_t *avi_out, float *flo_out) {
        check(bf_global_render_flow_frame(ctx, RES_X, RES_Y, BF_FLOW_LAST_UPLOADED, ppm_out, avi_out, flo_out), "global_render_flow_frame");
    }
    // bf_emit_slice with the rows' (u, v) from the held flow; returns the ticket (-1: nothing to enqueue)
    int64_t global_emit_slice(bf_emit *emit, uint64_t first, uint64_t start_time, bool lead, uint64_t lead_t, int lead_row,
                              int lead_col) {
        int64_t ticket = -1;
        check(bf_global_emit_slice(ctx, emit, (int64_t)size, first, start_time, lead ? 1 : 0, lead_t, lead_row, lead_col, &ticket),
              "global_emit_slice");
        return ticket;
    }

    // The fused OptimizerRolling::run (optimizer_rolling.h:48-125) on the device.
    int run(int max_itercount, ObjectModel &model, bf_run_info *info) {
        bf_run_opts o;
        bf_run_opts_default(&o);
        o.max_iter = max_itercount;
        o.res_x = RES_X;
        o.res_y = RES_Y;
        bf_model m;
        int rc = bf_run(ctx, &o, &m, info);
        check(rc, "run");
        model = ObjectModel(m);
        return rc;
    }
};

#endif  // BF_HOST_ACCEL_LIB_H
