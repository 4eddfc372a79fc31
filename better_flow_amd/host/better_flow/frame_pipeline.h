// frame_pipeline.h -- the stream engine's --img / --video frames: DVS_flow's frame of every slice (dvs_flow.h
// render_frame), the same bytes, without holding the solve up.
//
// The solving worker enqueues the render and compose (bf_frame_render) into a pinned frame slot before its context takes
// the next slice (render()); the engine's deliver() waits for it in slice order and hands it to a writer thread
// (deliver()), which writes the files and frees the slot.  A C-ABI library without the bf_frame_* entries (the CPU
// stand-in of the tests) gets the frame composed on the host from bf_projection_img / bf_color_time_img
// (frame_writer.h): the same bytes again.
#ifndef BF_HOST_FRAME_PIPELINE_H
#define BF_HOST_FRAME_PIPELINE_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>
#include <better_flow/failure_latch.h>
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
    }
    FramePipeline(const FramePipeline &) = delete;
    FramePipeline &operator=(const FramePipeline &) = delete;

    // The frame slots of every worker (device composition) and the writer thread.  contexts: one per worker, which must
    // outlive the pipeline.  Throws bf::AccelError.
    void start(const std::vector<bf_ctx *> &worker_contexts) {
        contexts = worker_contexts;
        held.assign(contexts.size(), 0);
        if (bf_frame_create) {
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
    }

    // the frame of slice `idx`, on the worker that solved it (SliceFarm::Task::on_solved), before its context takes the next
    // slice: enqueued into a frame slot (waiting for one if all are taken), or composed here on the host
    void render(uint64_t idx, int worker, bf_ctx *ctx, SliceFarm::Result &r) {
        FrameJob job;
        job.worker = worker;
        if (r.rc >= 0 && !state.empty()) {
            bf_frame *f = state[(size_t)job.worker];
            bool retried = false;   // (only this worker renders into f, so a slot counted free here is free in f)
            for (;;) {
                const int rc = bf_frame_render(ctx, f, &job.ticket);
                if (rc == BF_ERR_CAPACITY) {
                    std::unique_lock<std::mutex> g(mu);
                    if (held[(size_t)job.worker] >= cfg.slots) {   // every slot holds a frame not yet written: wait for one
                        const auto t0 = std::chrono::steady_clock::now();
                        cv.wait(g, [&] { return held[(size_t)job.worker] < cfg.slots || failure.failed(); });
                        wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                        retried = false;
                        if (!failure.failed()) continue;
                    } else if (!retried) {   // the writer freed a slot since the call: once more
                        retried = true;
                        continue;
                    }
                }
                if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: frame render failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); job.ticket = -1; }
                else { std::lock_guard<std::mutex> g(mu); ++held[(size_t)job.worker]; }
                break;
            }
        } else if (r.rc >= 0) {   // host composition: the four tiles through the synchronous renderers
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
        if (cfg.pictures)
            job.text = frame_sidecar(s.trigger_time, s.on_time_change, s.time_diff, s.ring_size, s.new_events, ObjectModel(r.model));
        std::unique_lock<std::mutex> g(mu);
        if (cfg.pictures) job.number = next_number++;
        // (host composition holds its frames in the queue: keep it short)
        if (state.empty()) cv.wait(g, [&] { return queue.size() < (size_t)cfg.slots || stopping; });
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
    };
    const FrameSettings cfg;
    FailureLatch &failure;
    std::vector<bf_ctx *> contexts;          // per worker
    std::vector<bf_frame *> state;           // per worker (device composition); empty: host composition
    std::mutex mu;                           // everything below
    std::condition_variable cv;
    std::map<uint64_t, FrameJob> ready;      // slice index -> its frame, from the worker's hook to deliver()
    std::vector<int> held;                   // per worker: slots rendered and not yet released
    std::deque<FrameJob> queue;              // delivered, in slice order, for the writer
    bool writing = false, stopping = false;
    uint64_t handed = 0, next_number = 0;
    double wait_s = 0;
    std::thread writer;
    AviWriter video;                         // (the writer's)

    // the frame slot of `job` (if it holds one) is free again
    void release(const FrameJob &job) {
        if (job.ticket >= 0) {
            (void)bf_frame_release(state[(size_t)job.worker], job.ticket);
            std::lock_guard<std::mutex> g(mu);
            --held[(size_t)job.worker];
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
