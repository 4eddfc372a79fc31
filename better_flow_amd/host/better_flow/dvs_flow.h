// dvs_flow.h -- the slice manager (mirror of the reference's better_flow/dvs_flow.h:21-389):
// a time-span ring of events, triggers on new-event count / elapsed time, one optimizer per
// slice warm-started from the previous model ("STM"), accumulation of processed events.
// Same public interface; the optimizer it drives runs on the MI355X.
//
// --img / --video render the reference's per-slice frame (dvs_flow.h:256-335): the 2 x 2 mosaic of the projection
// images and colour-coded time images, raw on top, motion compensated below -- the four tiles are computed on the
// device, composition and containers are in better_flow/frame_writer.h (PPM / uncompressed AVI, statistics in a
// side-car text file instead of cv::putText).  Not reproduced: the unbounded `motion_memory` copies of every slice
// (:239-242): only the per-slice summary the reference prints (:245-252) is kept.
#ifndef BF_HOST_DVS_FLOW_H
#define BF_HOST_DVS_FLOW_H

#include <better_flow/common.h>
#include <better_flow/event.h>
#include <better_flow/event_file.h>
#include <better_flow/frame_writer.h>
#include <better_flow/object_tracker.h>
#include <better_flow/object_render.h>
#include <better_flow/optimizer_rolling.h>

#include <chrono>
#include <unordered_map>

template <size_t MAX_SZ, sll SPAN> class DVS_flow {
public:
    // Buffer for incoming events (aka 'slice')
    CircularArray<Event, MAX_SZ, SPAN> ev_buffer;

protected:
    ull on_ev_change, on_time_change;          // triggers
    sll time_diff, event_diff;                 // time passed / new event count
    ull last_slice_time, current_slice_time;
    ObjectModel last_model;                    // starting point for the next minimizer
    bool accumulate;
    std::vector<LinearEventCloudTemplate<Event>> accumulated;

    struct SliceSummary {                      // what dvs_flow.h:245-252 prints per past slice
        ObjectModel model;
        size_t size;
        ull first_ts, last_ts;
    };
    std::vector<SliceSummary> motion_memory;

    bool manual_mode;
    int max_iter;
    int scale;
    bool generate_video;
    int video_fps;
    std::string video_name;
    bf::AviWriter outputvideo;
    bool generate_pictures;
    std::string img_prefix;
    bool generate_flow_img = false, generate_flow_field = false;   // --flow-img / --flow-field: flow_N.ppm / flow_N.flo
    std::string flow_prefix;
    bool generate_segments = false;            // --segments: segments_N.txt / segments_N.pgm
    bf::Segmenter segmenter;
    std::string segments_prefix;
    ull segments_count = 0;
    bool generate_objects = false;             // --objects: objects_N.txt
    bf::ObjectTracker tracker;                 // its .finder is the finder, with or without tracking; .finder.refit is the refit policy
    std::string objects_prefix;
    ull objects_count = 0;
    bf_ctx *objects_helper = nullptr;          // owned; lent to the refit policy: a group too large for the grouped solve is refit here
    bool generate_objects_track = false;       // --objects-track: identities carried across slices, objects_N.tracks.txt
    ull objects_origin = 0;                    // the previous slice's time origin
    bool generate_objects_img = false;         // --objects-img: objects_N.ppm / objects_N.pgm / objects_N.score.txt
    bf::ObjectRenderer renderer;
    bool generate_objects_flow = false;        // --objects-flow: objects_N.flo / objects_N.flow.ppm / objects_N.events.txt
    bf::AviWriter flowvideo;
    ull flow_count = 0;
    bool stm_disable;
    bool quiet;
    ull slices_done, slices_skipped, iterations_total;
    ull frame_count = 0;
    FILE *slice_log = nullptr;

    ull slice_origin();
    void render_frame(OptimizerRolling<LinearEventPtrs> &optimizer);
    void render_flow_frame(OptimizerRolling<LinearEventPtrs> &optimizer);
    void write_objects(LinearEventPtrs &slice, ull origin);
    void write_object_files(bf_ctx *ctx, const bf::Slice &sl, const std::string &base);

public:
    DVS_flow(ull on_ev_change_, ull on_time_change_, ull start_time = 0)
        : on_ev_change(on_ev_change_), on_time_change(on_time_change_), time_diff(0), event_diff(0),
          last_slice_time(start_time), current_slice_time(start_time), accumulate(false), manual_mode(false),
          max_iter(-1), scale(3), generate_video(false), video_fps(30), generate_pictures(false),
          stm_disable(false), quiet(false), slices_done(0), slices_skipped(0), iterations_total(0) {}

    bool add_event(Event &ev);
    void recompute();
    // one CSV record per slice (slice,events,new_events,rc,iterations,ms,mevents_per_s)
    bool open_slice_log(const std::string &path) {
        slice_log = std::fopen(path.c_str(), "w");
        if (slice_log) std::fprintf(slice_log, "slice,events,new_events,rc,iterations,ms,mevents_per_s\n");
        return slice_log != nullptr;
    }
    ~DVS_flow() {
        if (slice_log) std::fclose(slice_log);
        if (objects_helper) bf_destroy(objects_helper);
    }

    void set_accumulate(bool on = true) { accumulate = on; }
    LinearEventCloudTemplate<Event> get_accumulated();
    void set_manual_mode(bool on = true) { manual_mode = on; }
    void set_max_iter(int cap = -1) { max_iter = cap; }
    void set_scale(int s = 3) { scale = s; }
    void set_generate_video(bool val = true, std::string name = "out.avi", int framerate = 30) {   // :115-129
        generate_video = val; video_name = name; video_fps = framerate;   // (opened with the first frame, at the mosaic's size)
    }
    void set_generate_pictures(bool val = true, std::string img_prefix_ = "./") {
        generate_pictures = val; img_prefix = img_prefix_;
    }
    // the flow frame (compensated events | colour-coded flow | raw events: flow_N.ppm) and the per-pixel flow field
    // (flow_N.flo) of every slice under `prefix`; with set_generate_video, the flow frames also go to bf::flow_video_name
    void set_generate_flow(bool img, bool field, std::string prefix = "./") {
        generate_flow_img = img; generate_flow_field = field; flow_prefix = prefix;
    }
    // the component table (segments_N.txt) and the label image (segments_N.pgm) of every slice under `prefix`
    void set_generate_segments(const bf_segment_opts &opts, std::string prefix = "./") {
        generate_segments = true; segmenter.opts = opts; segments_prefix = prefix;
    }
    // the moving objects of every slice (objects_N.txt under `prefix`): `cfg`'s search, proposal, alternation and refit policy
    // (its result fields, hold_flow and refit.helper are not read); the number of objects is cfg.propose.max_models
    void set_generate_objects(const bf::ObjectFinder &cfg, std::string prefix = "./") {
        generate_objects = true; tracker.finder = cfg; objects_prefix = prefix;
    }
    // ... and their picture and score (objects_N.ppm, objects_N.pgm, objects_N.score.txt): the slice with every event under
    // its own object's model, in the assignment's window; a box sum of 255 / gain saturates an object's colour
    void set_generate_objects_img(int gain) { generate_objects_img = true; renderer.opts.gain = gain; }
    // ... and their per-event flow (objects_N.flo, objects_N.flow.ppm, objects_N.events.txt): every event under its own
    // object's model, held on the device by the finder (bf::ObjectFinder::hold_flow) and read through the held flow's outputs
    void set_generate_objects_flow() { generate_objects_flow = true; }
    // ... and their identities across slices (objects_N.tracks.txt): bf::ObjectTracker around the finder, a search every
    // `research_every` slices (0: only when it must)
    void set_generate_objects_track(int research_every) { generate_objects_track = true; tracker.research_every = research_every; }
    void set_stm_disable(bool off = true) { stm_disable = off; }
    void set_quiet(bool val = true) { this->quiet = val; }   // the reference parses --quiet but ignores it

    sll get_buf_size() { return this->ev_buffer.size(); }
    sll get_time_diff() { return this->time_diff; }
    sll get_buf_time_diff() { return (sll)(current_slice_time - slice_origin()); }   // dvs_flow.h:150-159
    ObjectModel get_last_model() { return this->last_model; }
    ull get_slices_done() const { return slices_done; }
    ull get_slices_skipped() const { return slices_skipped; }
    ull get_iterations_total() const { return iterations_total; }
};

// A new event enters the ring; a slice is solved as soon as enough events OR enough time have accumulated since the
// previous slice (either trigger; dvs_flow.h:164-181).  Returns whether this event closed a slice.
template <size_t MAX_SZ, sll SPAN> bool DVS_flow<MAX_SZ, SPAN>::add_event(Event &ev) {
    ev_buffer.push_back(ev);
    ++event_diff;
    current_slice_time = ev.timestamp;                        // (timestamps only grow)
    time_diff = (sll)(current_slice_time - last_slice_time);
    const bool due = event_diff >= (sll)on_ev_change || time_diff >= (sll)on_time_change;
    if (due) recompute();
    return due;
}

// Time origin of the slice in the ring: the oldest event of a full ring, else `SPAN` before the newest event (clamped
// at 0) -- dvs_flow.h:186-193.
template <size_t MAX_SZ, sll SPAN> ull DVS_flow<MAX_SZ, SPAN>::slice_origin() {
    if (ev_buffer.size() == MAX_SZ) return ev_buffer[MAX_SZ - 1].timestamp;
    return current_slice_time > (ull)SPAN ? current_slice_time - (ull)SPAN : 0;
}

// The reference's per-slice frame (dvs_flow.h:256-335): a 2 x 2 mosaic -- events as recorded on top, motion compensated
// below; projection image left, colour-coded time image right --, the four tiles computed on the device at scale 3.
template <size_t MAX_SZ, sll SPAN>
void DVS_flow<MAX_SZ, SPAN>::render_frame(OptimizerRolling<LinearEventPtrs> &optimizer) {
    const int rows = RES_X * 3, cols = RES_Y * 3;
    auto gray_tile = [&](bool compensated) {
        bf::Image2D<uint8_t> g = optimizer.get_projection_img(3, compensated);
        return bf::resize_bilinear(bf::gray_to_bgr(g.ptr(0), g.rows, g.cols), rows, cols);
    };
    auto colour_tile = [&](bool compensated) {
        int r = 0, c = 0;
        bf::FrameBGR f(0, 0);
        f.px = optimizer.get_color_time_img(3, compensated, &r, &c);
        f.rows = r; f.cols = c;
        return bf::resize_bilinear(f, rows, cols);
    };
    const bf::FrameBGR frame = bf::mosaic_2x2(gray_tile(true), colour_tile(true), gray_tile(false), colour_tile(false));
    if (generate_pictures) {
        const std::string base = img_prefix + "/frame_" + std::to_string(frame_count++);
        if (!bf::write_ppm(base + ".ppm", frame) && !quiet) std::cerr << "cannot write " << base << ".ppm\n";
        // what the reference draws with cv::putText, :277-315
        (void)bf::write_text(base + ".txt", bf::frame_sidecar(current_slice_time, on_time_change, time_diff, (size_t)ev_buffer.size(),
                                                              (long long)event_diff, last_model));
    }
    if (generate_video) {
        if (!outputvideo.is_open() && !outputvideo.open(video_name, frame.rows, frame.cols, video_fps))
            std::cout << "Could not open the output video for write" << std::endl;   // :329-331
        if (outputvideo.is_open()) outputvideo.write(frame);
    }
}

// The flow frame and the flow field of the slice (include/bf_accel.h, "per-pixel flow"): the three images the reference's
// visualiser publishes per recompute() (bf_visualizer.cpp:249-265), rendered synchronously beside render_frame.  The slice was
// uploaded in the ring's iteration order, newest -> oldest, which is the order color_flow_img walks it in: AccelLib asks for
// BF_FLOW_LAST_UPLOADED, and the owner of a pixel is the oldest event that lands on it.
template <size_t MAX_SZ, sll SPAN>
void DVS_flow<MAX_SZ, SPAN>::render_flow_frame(OptimizerRolling<LinearEventPtrs> &optimizer) {
    const std::string base = flow_prefix + "/flow_" + std::to_string(flow_count++);
    if (generate_flow_field) {
        const std::vector<float> flo = bf::flo_payload(optimizer.get_flow_field());
        if (!bf::write_flo(base + ".flo", RES_X, RES_Y, flo.data()) && !quiet) std::cerr << "cannot write " << base << ".flo\n";
    }
    if (!generate_flow_img) return;
    bf::Image2D<uint8_t> comp = optimizer.get_projection_img(1, false), raw = optimizer.get_projection_img(1, true);
    const std::vector<uint8_t> flow = optimizer.get_color_flow_img();
    const bf::FrameBGR frame = bf::compose_flow_frame(comp.ptr(0), flow.data(), raw.ptr(0), RES_X, RES_Y);
    if (!bf::write_ppm(base + ".ppm", frame) && !quiet) std::cerr << "cannot write " << base << ".ppm\n";
    if (generate_video) {
        if (!flowvideo.is_open() && !flowvideo.open(bf::flow_video_name(video_name), frame.rows, frame.cols, video_fps))
            std::cout << "Could not open the output video for write" << std::endl;
        if (flowvideo.is_open()) flowvideo.write(frame);
    }
}

// The moving objects of the slice (better_flow/object_finder.h) in three steps: the slice as arrays (Event::t holds the
// slice-local time, set_time); bf::ObjectFinder::find on it, or with --objects-track bf::ObjectTracker::next -- either leaves the
// slice's result in tracker.finder --; the files (write_object_files).
template <size_t MAX_SZ, sll SPAN> void DVS_flow<MAX_SZ, SPAN>::write_objects(LinearEventPtrs &slice, ull origin) {
    std::vector<int32_t> fx, fy, ft;
    fx.reserve(slice.size()); fy.reserve(slice.size()); ft.reserve(slice.size());
    for (auto &e : slice) {
        fx.push_back((int32_t)e.fr_x); fy.push_back((int32_t)e.fr_y); ft.push_back((int32_t)e.t);
    }
    const bf::Slice sl = {fx.data(), fy.data(), ft.data(), fx.size()};
    bf::ObjectFinder &fd = tracker.finder;   // (what is this class's to decide is set here, whatever order the setters were called in)
    const int s = fd.refit.fit.scale;
    bf_ctx *ctx = bf::DeviceContext::get((long long)MAX_SZ, s * RES_X + s, s * RES_Y + s);
    // (--objects-wide, bf::Refit::wide: every group is refit inside the grouped solve -- no second context)
    if (!fd.refit.wide && !objects_helper && bf_create(bf::DeviceContext::device(), (long long)MAX_SZ, s * RES_X + s, s * RES_Y + s, nullptr, &objects_helper) != BF_OK)
        objects_helper = nullptr;   // (a group too large for the grouped solve then keeps its model)
    fd.refit.helper = objects_helper;
    fd.assign.sensor_res_x = fd.refit.fit.sensor_res_x = fd.refit.fit.guard_res_x = RES_X;
    fd.assign.sensor_res_y = fd.refit.fit.sensor_res_y = fd.refit.fit.guard_res_y = RES_Y;
    fd.hold_flow = generate_objects_flow;
    if (generate_objects_track) {   // dt: the difference of the two slices' time origins, the absolute time set_time subtracts
        const int rc = tracker.next(ctx, sl, objects_count ? (int64_t)origin - (int64_t)objects_origin : 0);
        objects_origin = origin;
        if (rc < 0) throw bf::AccelError(rc, "--objects-track: " + tracker.error);
    } else {
        const int rc = fd.find(ctx, sl);
        if (rc < 0) throw bf::AccelError(rc, "--objects: " + fd.error);
    }
    write_object_files(ctx, sl, objects_prefix + "/objects_" + std::to_string(objects_count++));
}

// objects_N.txt; with --objects-track objects_N.tracks.txt; with --objects-merge the groups are those bf::ObjectMerger left, and
// objects_N.merge.txt lists its steps; with --objects-flow the held flow's outputs; with --objects-img the slice under its objects' models.
template <size_t MAX_SZ, sll SPAN>
void DVS_flow<MAX_SZ, SPAN>::write_object_files(bf_ctx *ctx, const bf::Slice &sl, const std::string &base) {
    const bf::ObjectFinder &fd = tracker.finder;
    const bf::Grouping &g = fd.grouping;
    if (!fd.write_objects(base + ".txt")) {
        if (!quiet) std::cerr << "cannot write " << base << ".txt\n";
        return;
    }
    if (generate_objects_track && !tracker.write_tracks(base + ".tracks.txt") && !quiet) std::cerr << "cannot write " << base << ".tracks.txt\n";
    // (--objects-merge) what the merger did to the proposed groups, and the contrast sum N^2 of the grouping it left
    if (fd.merge_num > 0 && !bf::ObjectMerger::write_steps(base + ".merge.txt", fd.steps, g.models.size(), fd.merged_sum_sq) && !quiet)
        std::cerr << "cannot write " << base << ".merge.txt\n";
    // (--objects-flow) the finder left the slice, the grouping and the held flow on the context: the flow field and the flow
    // frame as render_flow_frame writes the rolling optimiser's (oldest event owns a pixel), and one line per event.  A slice
    // without an object has no model to hold a flow under (bf::ObjectFinder::hold_flow): like --objects-img it writes nothing
    if (generate_objects_flow && !g.models.empty()) {
        std::vector<uint8_t> ppm((size_t)RES_X * (size_t)(3 * RES_Y) * 3);
        std::vector<float> flo((size_t)RES_X * (size_t)RES_Y * 2);
        std::vector<double> u(sl.n), v(sl.n);
        int frc = bf_global_render_flow_frame(ctx, RES_X, RES_Y, BF_FLOW_LAST_UPLOADED, ppm.data(), nullptr, flo.data());
        if (frc >= 0) frc = bf_global_get_flow(ctx, nullptr, nullptr, u.data(), v.data(), nullptr, nullptr);
        if (frc < 0) throw bf::AccelError(frc, std::string("--objects-flow: ") + bf_last_error(ctx));
        const bool w = bf::write_flo(base + ".flo", RES_X, RES_Y, flo.data()) && bf::write_ppm_raw(base + ".flow.ppm", RES_X, 3 * RES_Y, ppm.data());
        const bool we = fd.write_events(base + ".events.txt", sl, u, v);
        if (!(w && we) && !quiet) std::cerr << "cannot write " << base << ".flo / .flow.ppm / .events.txt\n";
    }
    if (!generate_objects_img || g.models.empty()) return;   // (no object: nothing to project)
    // find() leaves the context holding one group's events (its flows re-upload): the renderer uploads the slice again and
    // holds the final ids as its grouping
    renderer.opts.scale = fd.assign.scale;
    renderer.opts.sensor_res_x = RES_X; renderer.opts.sensor_res_y = RES_Y;
    renderer.opts.margin = fd.assign.margin;
    const int prc = renderer.render(ctx, sl, g.gid, g.models);
    if (prc < 0) throw bf::AccelError(prc, std::string("--objects-img: ") + bf_last_error(ctx));
    if ((!renderer.write_ppm(base + ".ppm") || !renderer.write_label_pgm(base + ".pgm") || !renderer.write_scores(base + ".score.txt")) && !quiet)
        std::cerr << "cannot write " << base << ".ppm / .pgm / .score.txt\n";
}

// One slice: the events now in the ring, their times made relative to the slice origin, one OptimizerRolling run --
// warm-started from the previous slice's model unless --stm-disable (the "short-term memory", dvs_flow.h:218-224) --,
// per-event flow fetched from the device, optional frame, bookkeeping (dvs_flow.h:185-347).
template <size_t MAX_SZ, sll SPAN> void DVS_flow<MAX_SZ, SPAN>::recompute() {
    const auto t_begin = std::chrono::steady_clock::now();
    const ull origin = slice_origin();
    const bool frames = generate_video || generate_pictures;
    if (frames)   // the frames are rendered at scale 3 whatever `scale` is: make room once
        (void)bf::DeviceContext::get((long long)MAX_SZ, 3 * RES_X + 3, 3 * RES_Y + 3);
    const int os = tracker.finder.refit.fit.scale;   // ... and the objects' refit at its own scale
    if (generate_objects) (void)bf::DeviceContext::get((long long)MAX_SZ, os * RES_X + os, os * RES_Y + os);

    LinearEventPtrs slice;                     // newest -> oldest, the ring's iteration order
    slice.reserve(ev_buffer.size());
    for (auto &e : ev_buffer) slice.push_back(&e);

    int rc;
    bf_run_info info;
    {
        OptimizerRolling<LinearEventPtrs> optimizer;
        optimizer.set_cloud(&slice, scale);
        optimizer.set_time(origin);
        optimizer.set_maxiter(max_iter);
        if (!stm_disable) optimizer.set_model(last_model);
        rc = manual_mode ? optimizer.manual() : optimizer.run();
        last_model = optimizer.get_model();
        optimizer.fetch_uv();                  // "compute the actual u and v after minimizations are done", :233-235
        if (frames) render_frame(optimizer);
        if (generate_flow_img || generate_flow_field) render_flow_frame(optimizer);
        if (generate_segments) {   // (after every other output: it reads the slice, and changes nothing the others read)
            const bf::Segmentation sg = optimizer.get_segmentation(segmenter);
            const std::string base = segments_prefix + "/segments_" + std::to_string(segments_count++);
            if ((!bf::write_segments_txt(base + ".txt", sg) || !bf::write_labels_pgm(base + ".pgm", sg)) && !quiet)
                std::cerr << "cannot write " << base << ".txt / .pgm\n";
        }
        info = optimizer.get_run_info();
    }
    // (after every other output, and after the optimizer: it uploads the slice again, and the next slice uploads its own)
    if (generate_objects) write_objects(slice, origin);
    ++slices_done;
    if (rc != 0) ++slices_skipped;
    iterations_total += (ull)info.iterations;

    // what the reference keeps of every past slice, and prints after each new one (:239-252)
    SliceSummary sm;
    sm.model = last_model;
    sm.size = 0;
    sm.first_ts = sm.last_ts = 0;
    for (auto &e : ev_buffer) {
        if (sm.size == 0) sm.first_ts = e.timestamp;
        sm.last_ts = e.timestamp;
        ++sm.size;
    }
    motion_memory.push_back(sm);
    if (!quiet) {
        std::cout << "\n\n------------------------\n";
        for (const SliceSummary &past : motion_memory)
            std::cout << past.model << "\n" << past.size << "\t" << past.first_ts << "\t" << past.last_ts << "\n";
    }
    if (slice_log) {   // one structured record per slice
        const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        std::fprintf(slice_log, "%llu,%zu,%lld,%d,%d,%.3f,%.3f\n", (unsigned long long)(slices_done - 1), sm.size,
                     (long long)event_diff, rc, (int)info.iterations, ms, ms > 0 ? sm.size / ms * 1e-3 : 0.0);
        std::fflush(slice_log);
    }

    if (accumulate) {   // a copy of the slice for get_accumulated(), oldest -> newest (:341-346)
        accumulated.emplace_back();
        LinearEventCloudTemplate<Event> &copy = accumulated.back();
        for (size_t k = ev_buffer.size(); k-- > 0;) copy.push_back(ev_buffer[k]);
    }
    event_diff = 0;
    last_slice_time = current_slice_time;
}

// Consecutive slices overlap (the ring spans more than the trigger interval), so an event is in several accumulated
// slices; the output keeps its FIRST copy (dvs_flow.h:351-389).  The reference finds the later copies with a linear
// scan of every later slice per event -- O(n^2) --, calling Event::operator== (event.h:39-45): same pixel, and, for
// a later-slice event e' at or before e in time (the scan stops at the first e' after e), e.timestamp - e'.timestamp
// < 0.1 ms.  Here every slice gets an index pixel -> positions (ascending in time) once, and an event only visits the
// events of its own pixel in the later slices: the same marks in the same order, O(n x slices).
template <size_t MAX_SZ, sll SPAN>
LinearEventCloudTemplate<Event> DVS_flow<MAX_SZ, SPAN>::get_accumulated() {
    typedef std::unordered_map<unsigned long long, std::vector<uint32_t>> PixelIndex;
    auto pixel_key = [](const Event &e) { return ((unsigned long long)e.fr_x << 32) | (unsigned long long)e.fr_y; };
    if (!quiet) std::cout << "Aggregating events into one cloud...\n";
    const size_t nslices = accumulated.size();
    std::vector<PixelIndex> index(nslices);
    for (size_t j = 1; j < nslices; ++j) {   // (slice 0 is never searched)
        uint32_t pos = 0;
        for (auto &e : accumulated[j]) index[j][pixel_key(e)].push_back(pos++);
    }
    LinearEventCloudTemplate<Event> unique;
    for (size_t i = 0; i < nslices; ++i) {
        if (!quiet) std::cout << "\tBuffer: " << i << "\n";
        for (auto &e : accumulated[i]) {
            if (e.t == -1) continue;          // a later copy of an event already written
            for (size_t j = i + 1; j < nslices; ++j) {
                const auto hit = index[j].find(pixel_key(e));
                if (hit == index[j].end()) continue;
                for (uint32_t pos : hit->second) {
                    Event &later = accumulated[j][pos];
                    if (later - e > 0) break;                 // positions ascend in time: nothing further can match
                    if (later.t != -1 && e == later) later.t = -1;
                }
            }
            unique.push_back(e);
        }
    }
    if (!quiet) std::cout << "Final buffer contains " << unique.size() << " events." << std::endl;
    return unique;
}

#endif  // BF_HOST_DVS_FLOW_H
