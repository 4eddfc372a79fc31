// frame_pipeline.h -- the stream engine's --img / --video frames: DVS_flow's frame of every slice (dvs_flow.h
// render_frame), the same bytes, without holding the solve up.
//
// The solving worker enqueues the render and compose (bf_frame_render) into a pinned frame slot before its context takes
// the next slice (render()); the engine's deliver() waits for it in slice order and hands it to a writer thread
// (deliver()), which writes the files and frees the slot.  A C-ABI library without the bf_frame_* entries (the CPU
// stand-in of the tests) gets the frame composed on the host from bf_projection_img / bf_color_time_img
// (frame_writer.h): the same bytes again.
//
// The flow frames and flow fields of --flow-img / --flow-field (include/bf_accel.h, "per-pixel flow") travel the same way, in
// the same job: bf_flow_frame_render into a slot of its own next to bf_frame_render, the same wait in deliver(), the same
// writer thread.  Without the bf_flow_frame_* entries the field is built on the host from bf_writeout_events + bf_compute_uv
// (flow_field.h) and the frame composed by frame_writer.h's compose_flow_frame.
#ifndef BF_HOST_FRAME_PIPELINE_H
#define BF_HOST_FRAME_PIPELINE_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>
#include <better_flow/failure_latch.h>
#include <better_flow/flow_field.h>
#include <better_flow/frame_writer.h>
#include <better_flow/object_model.h>
#include <better_flow/slice_farm.h>

// (weak: the host classes also link against C-ABI implementations that lack them -- the CPU stand-in the tests build --
// and the frames are then composed on the host)
extern "C" {
int bf_frame_create(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_frame **out) __attribute__((weak));
int bf_frame_destroy(bf_frame *frame) __attribute__((weak));
int bf_frame_render(bf_ctx *ctx, bf_frame *frame, int64_t *ticket_out) __attribute__((weak));
int bf_frame_wait(bf_ctx *ctx, bf_frame *frame, int64_t ticket, const uint8_t **ppm, const uint8_t **avi) __attribute__((weak));
int bf_frame_release(bf_frame *frame, int64_t ticket) __attribute__((weak));
}

namespace bf {

struct FrameSettings {
    std::string prefix;           // pictures: frame_N.ppm and the side-car frame_N.txt under it
    bool pictures = false;
    std::string video_name;       // non-empty: every frame appended to this AVI at video_fps
    int video_fps = 30;
    int slots = 4;                // frames rendered and not yet written, per worker
    bool flow_pictures = false;   // flow_N.ppm under flow_prefix; with a video_name, also appended to flow_video_name(video_name)
    bool flow_field = false;      // flow_N.flo under flow_prefix
    std::string flow_prefix;
    bool mosaic() const { return pictures || !video_name.empty(); }   // DVS_flow::render_frame's 2 x 2 frame
    bool flow() const { return flow_pictures || flow_field; }
    bool flow_video() const { return flow_pictures && !video_name.empty(); }
};


// What the side-car of a slice's frame says (frame_sidecar), next to the slice's model.
struct FrameFacts {
    uint64_t index = 0;           // the slice
    ull trigger_time = 0, on_time_change = 0;
    sll time_diff = 0;
    size_t ring_size = 0;
    long long new_events = 0;
};

// One lock, `mu`, for every member below it; `cfg`, `contexts` and `state` are constant once start() has returned, and
// `video` is the writer thread's alone.  render(): the farm's workers, each for the slice it solved (one worker renders
// into one bf_frame); deliver(): the engine's deliver(), in slice order.
class FramePipeline {
public:
    FramePipeline(const FrameSettings &settings, FailureLatch &failure_) : cfg(settings), failure(failure_) {}
    ~FramePipeline() {
        stop();
        for (bf_frame *f : state) (void)bf_frame_destroy(f);
        for (bf_flow_frame *f : flow_state) (void)bf_flow_frame_destroy(f);
    }
    FramePipeline(const FramePipeline &) = delete;
    FramePipeline &operator=(const FramePipeline &) = delete;

    // The frame slots of every worker (device composition) and the writer thread.  contexts: one per worker, which must
    // outlive the pipeline.  Throws bf::AccelError.
    void start(const std::vector<bf_ctx *> &worker_contexts) {
        contexts = worker_contexts;
        held.assign(contexts.size(), 0);
        flow_held.assign(contexts.size(), 0);
        if (cfg.flow() && bf_flow_frame_create) {
            const int layouts = (cfg.flow_pictures ? BF_FRAME_PPM : 0) | (cfg.flow_video() ? BF_FRAME_AVI : 0) | (cfg.flow_field ? BF_FLOW_FRAME_FLO : 0);
            for (bf_ctx *ctx : contexts) {
                bf_flow_frame *f = nullptr;
                const int rc = bf_flow_frame_create(ctx, RES_X, RES_Y, cfg.slots, layouts, &f);
                if (rc < 0) throw AccelError(rc, std::string("StreamEngine: bf_flow_frame_create failed: ") + bf_last_error(ctx));
                flow_state.push_back(f);
            }
        }
        if (cfg.mosaic() && bf_frame_create) {
            const int layouts = (cfg.pictures ? BF_FRAME_PPM : 0) | (cfg.video_name.empty() ? 0 : BF_FRAME_AVI);
            for (bf_ctx *ctx : contexts) {
                bf_frame *f = nullptr;
                const int rc = bf_frame_create(ctx, RES_X, RES_Y, cfg.slots, layouts, &f);
                if (rc < 0) throw AccelError(rc, std::string("StreamEngine: bf_frame_create failed: ") + bf_last_error(ctx));
                state.push_back(f);
            }
        }
        writer = std::thread([this] { write_frames(); });
    }

    void stop() {
        if (!writer.joinable()) return;
        {
            std::lock_guard<std::mutex> g(mu);
            stopping = true;
        }
        cv.notify_all();
        writer.join();
        video.close();
        flow_video.close();
    }

    // the frame(s) of slice `idx`, on the worker that solved it (SliceFarm::Task::on_solved), before its context takes the next
    // slice: enqueued into a frame slot (waiting for one if all are taken), or composed here on the host.  The slice was
    // uploaded oldest -> newest and the reference walks it newest -> oldest (datastructures.h:66-76), so the first uploaded
    // event on a pixel owns it in the flow field: BF_FLOW_FIRST_UPLOADED.
    // n_events: the slice's size; r.noise_uploaded: its noise flags as uploaded (SliceFarm::Task::keep_noise), for the host
    // composition of the flow field.
    void render(uint64_t idx, int worker, bf_ctx *ctx, SliceFarm::Result &r, size_t n_events = 0) {
        FrameJob job;
        job.worker = worker;
        if (cfg.mosaic() && r.rc >= 0 && !state.empty()) {
            bf_frame *f = state[(size_t)job.worker];
            slot_render(job.worker, held, r, ctx, job.ticket, [&] { return bf_frame_render(ctx, f, &job.ticket); });
        } else if (cfg.mosaic() && r.rc >= 0) {   // host composition: the four tiles through the synchronous renderers
            const int R = 3 * RES_X, C = 3 * RES_Y;
            std::vector<uint8_t> gray[2], colour[2];
            for (int i = 0; i < 2 && r.rc >= 0; ++i) {
                gray[i].resize((size_t)R * C);
                colour[i].resize((size_t)(R + 3) * (C + 3) * 3);
                int rc = bf_projection_img(ctx, 3, RES_X, RES_Y, i == 0 ? 1 : 0, gray[i].data());
                if (rc >= 0) rc = bf_color_time_img(ctx, 3, RES_X, RES_Y, i == 0 ? 1 : 0, colour[i].data());
                if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: frame tiles failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); }
            }
            if (r.rc >= 0) {
                const FrameBGR fr = compose_frame(gray[0].data(), colour[0].data(), gray[1].data(), colour[1].data(), R, C);
                if (cfg.pictures) { job.host_ppm.resize(fr.px.size()); ppm_payload(fr, job.host_ppm.data()); }
                if (!cfg.video_name.empty()) { job.host_avi.resize(avi_stride(fr.cols) * (size_t)fr.rows); avi_payload(fr, job.host_avi.data()); }
            }
        }
        if (cfg.flow() && r.rc >= 0 && !flow_state.empty()) {
            bf_flow_frame *f = flow_state[(size_t)job.worker];
            slot_render(job.worker, flow_held, r, ctx, job.flow_ticket, [&] { return bf_flow_frame_render(ctx, f, BF_FLOW_FIRST_UPLOADED, &job.flow_ticket); });
        } else if (cfg.flow() && r.rc >= 0) {     // host composition: the field from the per-event read-backs
            FlowField field;
            int rc = flow_field_from_readbacks(ctx, n_events, r.noise_uploaded ? r.noise_uploaded->data() : nullptr, RES_X, RES_Y,
                                               BF_FLOW_FIRST_UPLOADED, field);
            std::vector<uint8_t> gray[2];
            for (int i = 0; i < 2 && rc >= 0 && cfg.flow_pictures; ++i) {
                gray[i].resize((size_t)RES_X * RES_Y);
                rc = bf_projection_img(ctx, 1, RES_X, RES_Y, i, gray[i].data());
            }
            if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: flow frame failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); }
            else {
                if (cfg.flow_field) job.host_flo = flo_payload(field);
                if (cfg.flow_pictures) {
                    const FrameBGR fr = compose_flow_frame(gray[0].data(), color_flow_img_of(field).data(), gray[1].data(), RES_X, RES_Y);
                    job.host_flow_ppm.resize(fr.px.size()); ppm_payload(fr, job.host_flow_ppm.data());
                    if (cfg.flow_video()) { job.host_flow_avi.resize(avi_stride(fr.cols) * (size_t)fr.rows); avi_payload(fr, job.host_flow_avi.data()); }
                }
            }
        }
        std::lock_guard<std::mutex> g(mu);
        ready[idx] = std::move(job);
    }

    // deliver(), in slice order: wait for the slice's frame and hand it to the writer
    void deliver(const FrameFacts &s, const SliceFarm::Result &r) {
        FrameJob job;
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = ready.find(s.index);
            if (it == ready.end()) return;
            job = std::move(it->second);
            ready.erase(it);
        }
        if (r.rc < 0) return release(job);   // (failed: nothing to write; the slot goes back)
        const auto t0 = std::chrono::steady_clock::now();
        if (job.ticket >= 0) {
            bf_ctx *ctx = contexts[(size_t)job.worker];
            const int rc = bf_frame_wait(ctx, state[(size_t)job.worker], job.ticket, &job.ppm, &job.avi);
            if (rc < 0) {
                failure.fail(rc, "StreamEngine: slice " + std::to_string(s.index) + ": frame: " + bf_last_error(ctx));
                return release(job);
            }
        } else {
            job.ppm = job.host_ppm.empty() ? nullptr : job.host_ppm.data();
            job.avi = job.host_avi.empty() ? nullptr : job.host_avi.data();
        }
        if (job.flow_ticket >= 0) {
            bf_ctx *ctx = contexts[(size_t)job.worker];
            const int rc = bf_flow_frame_wait(ctx, flow_state[(size_t)job.worker], job.flow_ticket, &job.flow_ppm, &job.flow_avi, &job.flo);
            if (rc < 0) {
                failure.fail(rc, "StreamEngine: slice " + std::to_string(s.index) + ": flow frame: " + bf_last_error(ctx));
                return release(job);
            }
        } else {
            job.flow_ppm = job.host_flow_ppm.empty() ? nullptr : job.host_flow_ppm.data();
            job.flow_avi = job.host_flow_avi.empty() ? nullptr : job.host_flow_avi.data();
            job.flo = job.host_flo.empty() ? nullptr : job.host_flo.data();
        }
        if (cfg.pictures)
            job.text = frame_sidecar(s.trigger_time, s.on_time_change, s.time_diff, s.ring_size, s.new_events, ObjectModel(r.model));
        std::unique_lock<std::mutex> g(mu);
        if (cfg.pictures) job.number = next_number++;
        if (cfg.flow()) job.flow_number = next_flow_number++;
        // (host composition holds its frames in the queue: keep it short)
        if ((cfg.mosaic() && state.empty()) || (cfg.flow() && flow_state.empty()))
            cv.wait(g, [&] { return queue.size() < (size_t)cfg.slots || stopping; });
        wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        queue.push_back(std::move(job));
        ++handed;
        g.unlock();
        cv.notify_all();
    }

    // every frame delivered so far is in its files
    void wait_written() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return queue.empty() && !writing; });
    }

    void wake() { wake_waiters(mu, cv); }   // (the engine's failure waker)

    uint64_t delivered() { std::lock_guard<std::mutex> g(mu); return handed; }
    // 1: the flow frames are composed on the device, 0: on the host (a library without bf_flow_frame_*), -1: none asked for
    int flow_on_device() const { return cfg.flow() ? (flow_state.empty() ? 0 : 1) : -1; }
    // time spent waiting for frames: a free frame slot, a render to finish, room at the writer
    double seconds_waiting() { std::lock_guard<std::mutex> g(mu); return wait_s; }

private:
    struct FrameJob {             // one slice's frame, from its worker to the writer
        int worker = -1;
        int64_t ticket = -1;                  // device composition: the frame slot's ticket
        std::vector<uint8_t> host_ppm, host_avi;   // host composition: the payloads
        const uint8_t *ppm = nullptr, *avi = nullptr;
        std::string text;                     // the side-car
        uint64_t number = 0;                  // frame_<number>
        // the flow frame and the flow field of the same slice
        int64_t flow_ticket = -1;
        std::vector<uint8_t> host_flow_ppm, host_flow_avi;
        std::vector<float> host_flo;
        const uint8_t *flow_ppm = nullptr, *flow_avi = nullptr;
        const float *flo = nullptr;
        uint64_t flow_number = 0;             // flow_<number>
    };
    const FrameSettings cfg;
    FailureLatch &failure;
    std::vector<bf_ctx *> contexts;          // per worker
    std::vector<bf_frame *> state;           // per worker (device composition); empty: host composition
    std::vector<bf_flow_frame *> flow_state; // the same for the flow frames
    std::mutex mu;                           // everything below
    std::condition_variable cv;
    std::map<uint64_t, FrameJob> ready;      // slice index -> its frame, from the worker's hook to deliver()
    std::vector<int> held, flow_held;        // per worker: slots rendered and not yet released (frames, flow frames)
    std::deque<FrameJob> queue;              // delivered, in slice order, for the writer
    bool writing = false, stopping = false;
    uint64_t handed = 0, next_number = 0, next_flow_number = 0;
    double wait_s = 0;
    std::thread writer;
    AviWriter video, flow_video;             // (the writer's)

    // One render into a slot of this worker's frame state (`call` returns the C-ABI's code and sets `ticket`): with every slot
    // holding a frame not yet written, waits for the writer to free one.  (Only this worker renders into that state, so a slot
    // counted free in `count` is free there.)
    template <class Call>
    void slot_render(int worker, std::vector<int> &count, SliceFarm::Result &r, bf_ctx *ctx, int64_t &ticket, Call call) {
        bool retried = false;
        for (;;) {
            const int rc = call();
            if (rc == BF_ERR_CAPACITY) {
                std::unique_lock<std::mutex> g(mu);
                if (count[(size_t)worker] >= cfg.slots) {   // every slot holds a frame not yet written: wait for one
                    const auto t0 = std::chrono::steady_clock::now();
                    cv.wait(g, [&] { return count[(size_t)worker] < cfg.slots || failure.failed(); });
                    wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    retried = false;
                    if (!failure.failed()) continue;
                } else if (!retried) {   // the writer freed a slot since the call: once more
                    retried = true;
                    continue;
                }
            }
            if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: frame render failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); ticket = -1; }
            else { std::lock_guard<std::mutex> g(mu); ++count[(size_t)worker]; }
            break;
        }
    }

    // the frame slot of `job` (if it holds one) is free again
    void release(const FrameJob &job) {
        if (job.ticket >= 0) {
            (void)bf_frame_release(state[(size_t)job.worker], job.ticket);
            std::lock_guard<std::mutex> g(mu);
            --held[(size_t)job.worker];
        }
        if (job.flow_ticket >= 0) {
            (void)bf_flow_frame_release(flow_state[(size_t)job.worker], job.flow_ticket);
            std::lock_guard<std::mutex> g(mu);
            --flow_held[(size_t)job.worker];
        }
        cv.notify_all();
    }

    // the writer thread: the files of every delivered frame, in slice order; then the frame's slot is free again
    void write_frames() {
        const int rows = 6 * RES_X, cols = 6 * RES_Y;
        for (;;) {
            FrameJob job;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return stopping || !queue.empty(); });
                if (queue.empty()) return;
                job = std::move(queue.front());
                queue.pop_front();
                writing = true;
            }
            if (cfg.pictures && job.ppm) {
                const std::string base = cfg.prefix + "/frame_" + std::to_string(job.number);
                if (!write_ppm_raw(base + ".ppm", rows, cols, job.ppm)) std::cerr << "cannot write " << base << ".ppm\n";
                (void)write_text(base + ".txt", job.text);
            }
            if (!cfg.video_name.empty() && job.avi) {
                if (!video.is_open() && !video.open(cfg.video_name, rows, cols, cfg.video_fps))
                    std::cout << "Could not open the output video for write" << std::endl;
                if (video.is_open()) video.write_raw(job.avi);
            }
            if (cfg.flow()) {
                const std::string base = cfg.flow_prefix + "/flow_" + std::to_string(job.flow_number);
                if (job.flo && !write_flo(base + ".flo", RES_X, RES_Y, job.flo)) std::cerr << "cannot write " << base << ".flo\n";
                if (job.flow_ppm && !write_ppm_raw(base + ".ppm", RES_X, 3 * RES_Y, job.flow_ppm)) std::cerr << "cannot write " << base << ".ppm\n";
                if (job.flow_avi) {
                    if (!flow_video.is_open() && !flow_video.open(flow_video_name(cfg.video_name), RES_X, 3 * RES_Y, cfg.video_fps))
                        std::cout << "Could not open the output video for write" << std::endl;
                    if (flow_video.is_open()) flow_video.write_raw(job.flow_avi);
                }
            }
            release(job);
            {
                std::lock_guard<std::mutex> g(mu);
                writing = false;
            }
            cv.notify_all();
        }
    }
};

}  // namespace bf

#endif  // BF_HOST_FRAME_PIPELINE_H
