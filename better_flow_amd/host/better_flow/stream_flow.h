// stream_flow.h -- the slice former for high event rates: the reference's event ring and triggers
// (CircularArray, datastructures.h:6-115; DVS_flow::add_event / recompute, dvs_flow.h:164-347) on a
// structure-of-arrays ring in PINNED memory (better_flow/event_ring.h), handed to the device without a copy on the
// host, with the slices solved by a slice farm (better_flow/slice_farm.h).
//
// Why a second front end next to DVS_flow.  DVS_flow keeps the reference's public `ev_buffer` of 152-byte Event
// records: one add_event() call and one 152-byte store per event, and an AoS -> SoA repack per slice
// (accel_lib.h:91-99; AccelLib::init_gpu here) -- 23 Mevents/s end to end, against a device path that solves
// warm-started 1M-event slices at several Gevents/s.  Here
//   * a slice is one or two contiguous pieces of the ring, copied by DMA (bf_upload_ring16_async), and
//     Event::set_local_time runs on the device;
//   * events arrive in BULK: add_events(rows, cols, timestamps, n) copies a block into the ring, and
//     reserve() / commit() let a producer (a file reader, a socket) write into the ring itself -- then the only host
//     copy is the producer's own.  Trigger points inside a block are found by a binary search on the timestamps and
//     a subtraction on the counts, not by visiting every event;
//   * slices are solved by SliceFarm workers: with set_pipelined(true) the caller goes on filling the ring while
//     slice k is being solved and slice k + 1 uploaded (an STM chain stays sequential on one worker); with
//     --stm-disable style independent slices, several workers / GPUs take them in parallel.  Results are applied in
//     slice order either way;
//   * per-event flow comes back only if asked for (set_want_flow / set_accumulate), straight into a pinned (u, v) ring;
//   * the -o table (set_accumulate, set_accumulate_device) and the frames (set_frames) are components of their own
//     (better_flow/flow_table.h, better_flow/frame_pipeline.h): the worker that solved a slice calls them through the
//     task's one on_solved hook, deliver() calls them in slice order, and they report a failure through the engine's
//     FailureLatch (better_flow/failure_latch.h).
//
// Semantics: those of DVS_flow, element for element --
//   * ring of at most MAX_SZ events spanning at most SPAN ns (push_back :31-44, fix_span :46-59);
//   * trigger: events since the last slice >= on_ev_change OR time since it >= on_time_change (:164-181);
//   * slice = the ring content, EXCEPT that a full ring leaves its oldest element out (end() :71-76);
//   * slice start time = oldest timestamp if the ring is full, else max(now - SPAN, 0) (:186-191);
//   * warm start from the previous slice's model unless stm_disable (:218-219);
//   * a slice stopped by the small-window guard flags its events as noise, and flagged events stay out of the time
//     images of later, overlapping slices (optimizer_rolling.h:49-55, accel_lib.h:152);
//   * set_accumulate + get_accumulated(): every event once, with the flow of the first slice it was solved in --
//     DVS_flow::get_accumulated (dvs_flow.h:351-389) with its exact marking rule.
// Order inside a slice is oldest -> newest here (the reference iterates newest -> oldest); the device accumulates
// integers, so the order does not change any result.  The bulk paths assume what the reference assumes of its input
// ("timestamps only grow"): non-decreasing timestamps; set_assume_sorted(false) makes add_events() visit every event.
// tests/cpp/test_stream.cpp holds this class to DVS_flow slice by slice, on the oracle shim and on the GPU.
#ifndef BF_HOST_STREAM_FLOW_H
#define BF_HOST_STREAM_FLOW_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>
#include <better_flow/event_ring.h>
#include <better_flow/failure_latch.h>
#include <better_flow/flow_table.h>
#include <better_flow/frame_pipeline.h>
#include <better_flow/object_model.h>
#include <better_flow/slice_farm.h>

#include <algorithm>
#include <memory>

namespace bf {

// One solved slice, in slice order (the slice callback, the slice log).
struct SliceRecord {
    uint64_t index = 0;           // 0, 1, ... in trigger order
    uint64_t first_event = 0;     // arrival number of the slice's oldest event
    uint64_t events = 0;          // events in the slice
    uint64_t ring_size = 0;       // CircularArray::size() at the trigger (events + 1 for a full ring)
    uint64_t new_events = 0;      // events since the previous slice
    ull start_time = 0, trigger_time = 0;   // slice origin / newest timestamp, ns
    ull oldest_time = 0;          // timestamp of the slice's oldest event (0 for an empty slice)
    uint64_t events_seen = 0;     // events that had arrived when the slice was triggered
    sll time_diff = 0;            // time since the previous slice
    int rc = 0;
    bool window_guard = false;
    bf_run_info info;
    ObjectModel model;
    double ms = 0;
    int device = 0;
};

class StreamEngine {
public:
    struct Span {                 // a writable piece of the ring (reserve)
        uint64_t *timestamp;
        uint16_t *row, *col;
        size_t n;
    };
    typedef std::function<void(const SliceRecord &)> SliceFn;

    StreamEngine(size_t max_sz_, sll span_, ull on_ev_change_, ull on_time_change_, ull start_time = 0)
        : max_sz(max_sz_), span(span_), on_ev_change(on_ev_change_), on_time_change(on_time_change_), last_slice_time(start_time),
          current_slice_time(start_time) {
        if (max_sz < 1) throw AccelError(BF_ERR_ARG, "StreamEngine: ring capacity must be >= 1");
        std::memset(&last_info, 0, sizeof(last_info));
        devices.push_back(DeviceContext::device());
        failure.on_failure([this] {   // every thread that waits for something a failure ends
            wake_waiters(mu, cv);
            if (device_table) device_table->wake();
            if (frames) frames->wake();
        });
    }
    virtual ~StreamEngine() {   // (then the members go, the farm and its contexts last)
        if (farm) try { farm->drain(); } catch (...) {}
    }
    StreamEngine(const StreamEngine &) = delete;
    StreamEngine &operator=(const StreamEngine &) = delete;

    // ---- settings (before the first event) ----
    void set_max_iter(int v = -1) { max_iter = v; }
    void set_scale(int v = 3) { scale = v; }
    void set_stm_disable(bool v = true) { stm_disable = v; }
    void set_want_flow(bool v = true) { want_flow = v; }     // fetch per-event (u, v) after every slice
    void set_accumulate(bool v = true) { accumulate = v; }   // keep every slice's events + flow for get_accumulated()
    // build get_accumulated()'s table on the device as the slices are solved (get_accumulated_device).  Needs non-decreasing
    // timestamps (set_assume_sorted, the default), a span below 2^31 ns (the device keeps slice-local times as int32), every
    // worker on one device (the covered state lives there; the workers enqueue their slices in slice order) and every event
    // on the RES_X x RES_Y sensor (an address outside it fails the run; get_accumulated takes any 16-bit address).
    // Independent of set_accumulate: both may be on.
    void set_accumulate_device(bool v = true) { accumulate_device = v; }
    void set_pipelined(bool v = true) { pipelined = v; }     // add_event(s) return at the trigger; drain() waits
    void set_assume_sorted(bool v = true) { assume_sorted = v; }
    void set_time_base(ull t) { time_base = t; }             // ring timestamps are absolute; logical time = timestamp - base
    void set_lookahead(size_t n) { lookahead = n; }          // ring slots beyond MAX_SZ (default: 2 MAX_SZ, at least 65536)
    void set_devices(const std::vector<int> &d, int contexts = 1) { devices = d; contexts_per_device = contexts; }
    void on_slice(SliceFn fn) { slice_fn = std::move(fn); }
    // DVS_flow's frames (set_generate_pictures / set_generate_video): one per slice, in slice order.  pictures: frame_N.ppm and
    // the side-car frame_N.txt under `prefix`; a non-empty video_name: every frame appended to that AVI at video_fps.  The
    // frames are rendered at scale 3 whatever set_scale says, so the contexts get that image capacity too.
    void set_frames(const std::string &prefix, bool pictures, const std::string &video_name = "", int video_fps = 30, int slots = 4) {
        frame_cfg.prefix = prefix; frame_cfg.pictures = pictures; frame_cfg.video_name = video_name; frame_cfg.video_fps = video_fps;
        frame_cfg.slots = slots < 1 ? 1 : slots;
        frames_on = frame_cfg.mosaic() || frame_cfg.flow();
    }
    // DVS_flow's flow frames and flow fields (set_generate_flow): flow_N.ppm / flow_N.flo under `prefix`, one per slice, in
    // slice order; with a video name set by set_frames, the flow frames also go to bf::flow_video_name of it.
    void set_flow_frames(const std::string &prefix, bool pictures, bool field) {
        frame_cfg.flow_prefix = prefix; frame_cfg.flow_pictures = pictures; frame_cfg.flow_field = field;
        frames_on = frame_cfg.mosaic() || frame_cfg.flow();
    }

    // Create the workers, their device contexts and the pinned ring now (otherwise: at the first event).
    void warm_up() { ensure_ring(); }

    // ---- input ----
    // DVS_flow::add_event (dvs_flow.h:164-181); row / column as Event::fr_x / fr_y.  Returns whether this event closed a slice.
    bool add_event(uint32_t row, uint32_t col, ull timestamp) {
        Span s[2];
        (void)reserve(1, s);
        s[0].timestamp[0] = timestamp + time_base;
        s[0].row[0] = narrow(row); s[0].col[0] = narrow(col);
        return commit(1) > 0;
    }

    // n add_event calls in one: the block is copied into the ring piecewise; returns the number of slices it closed.
    size_t add_events(const uint32_t *rows, const uint32_t *cols, const ull *timestamps, size_t n) {
        size_t slices = 0, done = 0;
        while (done < n) {
            Span s[2];
            const size_t got = reserve(n - done, s);
            size_t k = done;
            for (int p = 0; p < 2; ++p)
                for (size_t i = 0; i < s[p].n; ++i, ++k) {
                    s[p].timestamp[i] = timestamps[k] + time_base;
                    s[p].row[i] = narrow(rows[k]); s[p].col[i] = narrow(cols[k]);
                }
            slices += commit(got);
            done += got;
        }
        return slices;
    }
    // The same from arrays already in the ring's layout (absolute timestamps = logical + time base).
    size_t add_events(const uint16_t *rows, const uint16_t *cols, const uint64_t *timestamps, size_t n) {
        size_t slices = 0, done = 0;
        while (done < n) {
            Span s[2];
            const size_t got = reserve(n - done, s);
            size_t k = done;
            for (int p = 0; p < 2; ++p) {
                std::memcpy(s[p].timestamp, timestamps + k, s[p].n * 8);
                std::memcpy(s[p].row, rows + k, s[p].n * 2);
                std::memcpy(s[p].col, cols + k, s[p].n * 2);
                k += s[p].n;
            }
            slices += commit(got);
            done += got;
        }
        return slices;
    }

    // Producer interface: up to `want` free ring slots as one or two pieces, to be filled with ABSOLUTE timestamps
    // (logical time + time base), rows, columns -- then commit(n) for the first n of them.  Blocks (pipelined mode) until
    // the slots are no longer needed by a slice in flight.  Returns the number of slots granted (>= 1).
    size_t reserve(size_t want, Span out[2]) {
        ensure_ring();
        rethrow_failure();
        if (want < 1) want = 1;
        const size_t room = ring.cap - max_sz;
        if (want > room) want = room;
        uint64_t prot = protected_from.load(std::memory_order_acquire);
        if (prot != UINT64_MAX && head + 1 > prot + ring.cap) {   // not even one slot: wait for the oldest slice in flight
            const auto t_wait = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { prot = protected_from.load(std::memory_order_acquire); return failure.failed() || prot == UINT64_MAX || head + 1 <= prot + ring.cap; });
            g.unlock();
            blocked_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count();
            rethrow_failure();
        }
        if (prot != UINT64_MAX && head + want > prot + ring.cap) want = (size_t)(prot + ring.cap - head);
        const RingPieces w = ring.pieces(head, want);
        for (int p = 0; p < 2; ++p) out[p] = Span{ring.ts + w.p[p].at, ring.row + w.p[p].at, ring.col + w.p[p].at, w.p[p].n};
        return want;
    }

    // The first n reserved slots now hold events: run the triggers over them.  Returns the number of slices closed.
    size_t commit(size_t n) {
        size_t slices = 0;
        uint64_t g = head;
        const uint64_t end = head + n;
        if (n == 0) return 0;
        // new events are not noise (Event(x, y, t): noise(false)); before any flag was ever set the whole ring is still zero
        if (noise_live.load(std::memory_order_relaxed) > 0) ring_fill(ring.noise, ring.pieces(g, n), 0);
        if (accumulate) history.archive(ring, g, end, time_base);
        while (g < end) {
            // first event of [g, end) at which a trigger fires: by count ...
            const uint64_t need = (event_diff + 1 >= (sll)on_ev_change) ? 0 : (uint64_t)((sll)on_ev_change - event_diff - 1);
            uint64_t k = g + need;
            // ... or by time: (sll)(t - last_slice_time) >= on_time_change
            if (assume_sorted) {
                uint64_t lo = g, hi = (k < end ? k : end);   // a time trigger only matters before the count trigger
                if (lo < hi && time_due(logical(hi - 1))) {
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        if (time_due(logical(mid))) hi = mid; else lo = mid + 1;
                    }
                    k = lo;
                }
            } else {
                for (uint64_t q = g; q < end && q < k; ++q)
                    if (time_due(logical(q))) { k = q; break; }
            }
            if (k >= end) {   // no trigger in the rest of the block
                advance(end - g, end);
                break;
            }
            advance(k - g + 1, k + 1);
            recompute();
            ++slices;
            g = k + 1;
        }
        return slices;
    }

    // DVS_flow::recompute (dvs_flow.h:185-347) without the rendering branches: solve the ring's content now.
    void recompute() {
        ensure_ring();
        rethrow_failure();
        trim();
        Pending p;
        p.index = slices_submitted++;
        p.ring_size = ring_size;
        const uint64_t oldest = head - ring_size;
        p.full = ring_size == max_sz;
        if (p.full) {            // full ring: iteration stops one short (:71-76), start = oldest timestamp
            p.start_time = logical(oldest);
            p.first = oldest + 1;
            p.n = ring_size - 1;
            p.zero_excluded = want_flow_any() && oldest + 1 > last_trigger_plus1;   // that event has never been in a slice
        } else {
            p.start_time = (current_slice_time > (ull)span) ? current_slice_time - (ull)span : 0;
            p.first = oldest;
            p.n = ring_size;
            p.zero_excluded = false;
        }
        p.trigger_time = current_slice_time;
        p.oldest_time = p.n > 0 ? logical(p.first) : 0;
        p.new_events = (uint64_t)event_diff;
        p.time_diff = time_diff;
        p.trigger_plus1 = head;
        // (the ring slots a slice in flight still needs: its events and, for a full ring, the oldest element it leaves out --
        // deliver() zeroes that element's flow and must still find it there)
        p.protect = oldest;
        SliceFarm::Task t;
        t.ring_row = ring.row; t.ring_col = ring.col; t.ring_ts = ring.ts; t.ring_noise = ring.noise; t.noise_live = &noise_live;
        t.first_global = p.first;
        t.cap = (int64_t)ring.cap; t.first = (int64_t)ring.slot(p.first); t.n = (int64_t)p.n;
        t.t0 = p.start_time + time_base;
        t.scale = scale; t.res_x = RES_X; t.res_y = RES_Y; t.max_iter = max_iter;
        t.warm = stm_disable ? SliceFarm::Warm::Cold : SliceFarm::Warm::FromPrevious;
        if (device_table || frames) {
            EmitSlice e;
            if (device_table) {
                e.first = p.first; e.n = p.n; e.start_time = p.start_time;
                e.lead = p.full && oldest + 1 > last_trigger_plus1;
                if (e.lead) { e.lead_t = logical(oldest); e.lead_row = ring.row[ring.slot(oldest)]; e.lead_col = ring.col[ring.slot(oldest)]; }
                t.want_uv = true;
            }
            const uint64_t idx = p.index;
            // (the host composition of the flow field -- a library without bf_flow_frame_* -- rebuilds the field from per-event
            // read-backs and needs the noise flags the slice was uploaded with: the farm keeps a copy of them for the hook)
            t.keep_noise = frames && frames->flow_on_device() == 0;
            const size_t n_events = (size_t)p.n;
            t.on_solved = [this, idx, e, n_events](bf_ctx *ctx, SliceFarm::Result &r) {
                if (device_table) device_table->enqueue(idx, ctx, r, e);
                if (frames) frames->render(idx, (int)worker_of(ctx), ctx, r, n_events);
            };
        }
        if ((accumulate || (want_flow && farm->workers() > 1)) && p.n > 0) {
            // A private block per slice, copied into the ring by deliver() -- which runs in SLICE order.  Needed for
            // get_accumulated(), and whenever several workers solve overlapping slices at once: written straight into
            // the shared ring, an event's flow would be that of whichever slice FINISHED last (and two workers would
            // write overlapping host memory concurrently), not that of the latest slice as in DVS_flow.
            // (uninitialised: bf_compute_uv_ring writes every pair.  A value-initialised vector cost the producer 16 MB of
            // page faults and zeroes per 1M-event slice -- 4 ms, more than the slice's whole solve)
            p.block = std::shared_ptr<double>(new double[2 * (size_t)p.n], std::default_delete<double[]>());
            t.uv_ring = p.block.get(); t.uv_cap = (int64_t)p.n; t.uv_first = 0;
        } else if (want_flow && p.n > 0) {   // one worker: slices complete in order, straight into the pinned ring
            t.uv_ring = ring.uv; t.uv_cap = (int64_t)ring.cap; t.uv_first = t.first;
        }
        t.user = p.index;
        bool flag_after = false;
        if (farm->workers() > 1 && p.n > 0 && window_guard_on_host(p)) {   // see slice_farm.h: uploads run ahead
            // (earlier slices overlap this one in the ring and their workers may not have read it yet: in the reference's
            // order they do not see this slice's flags -- wait for them first.  The guard stops a slice once in a long while.)
            farm->drain();
            // With frames, the slice itself must not see its own flags either: DVS_flow renders it as uploaded, before
            // OptimizerRolling::run flagged it -- flag once it has been solved and rendered.
            if (frames_on) flag_after = true;
            else flag_noise(p);
        }
        {
            std::lock_guard<std::mutex> g(mu);
            pending.push_back(p);
            protected_from.store(pending.front().protect, std::memory_order_release);
        }
        last_trigger_plus1 = head;
        event_diff = 0;
        last_slice_time = current_slice_time;
        farm->submit(t);
        if (flag_after) {
            farm->drain();
            flag_noise(p);
        }
        if (!pipelined) drain();
    }

    // Wait for every slice triggered so far (pipelined mode); rethrows a failure of a slice as bf::AccelError.
    void drain() {
        if (farm) farm->drain();
        if (frames) frames->wait_written();   // every frame delivered so far is in its files
        rethrow_failure();
    }

    // ---- the ring, DVS_flow style (idx 0 = newest; CircularArray::operator[], :61-64).  Call drain() first in pipelined mode. ----
    size_t size() { trim(); return ring_size; }
    uint32_t row(size_t idx) const { return ring.row[slot_of(idx)]; }
    uint32_t col(size_t idx) const { return ring.col[slot_of(idx)]; }
    ull timestamp(size_t idx) const { return ring.ts[slot_of(idx)] - time_base; }
    double u(size_t idx) const { return flow_of(idx, 0); }
    double v(size_t idx) const { return flow_of(idx, 1); }

    ObjectModel get_last_model() { std::lock_guard<std::mutex> g(mu); return last_model; }
    bf_run_info get_run_info() { std::lock_guard<std::mutex> g(mu); return last_info; }
    ull get_slices_done() { std::lock_guard<std::mutex> g(mu); return slices_done; }
    ull get_slices_skipped() { std::lock_guard<std::mutex> g(mu); return slices_skipped; }
    ull get_iterations_total() { std::lock_guard<std::mutex> g(mu); return iterations_total; }
    sll get_buf_size() { return (sll)size(); }
    sll get_time_diff() const { return time_diff; }
    ull events_seen() const { return head; }
    double seconds_blocked() const { return blocked_s; }   // the producer waited this long in reserve() for slices in flight
    uint64_t frames_delivered() { return frames ? frames->delivered() : 0; }
    // 1: the flow frames are composed on the device (bf_flow_frame_*), 0: on the host from read-backs, -1: no flow frames
    int flow_frames_on_device() { return frames ? frames->flow_on_device() : -1; }
    // time the engine waited for frames: a free frame slot, a render to finish, room at the writer
    double seconds_frame_wait() { return frames ? frames->seconds_waiting() : 0.0; }

    // DVS_flow::get_accumulated (dvs_flow.h:351-389): the events of all slices, each once, with the flow of the first
    // slice that solved it, by the reference's marking rule (HostFlowAccumulator::table); drains first.
    FlowTable get_accumulated() { drain(); return history.table(); }
    // The same table, element for element, from the device (set_accumulate_device); drains first.
    FlowTable get_accumulated_device() { drain(); return device_table ? device_table->table() : FlowTable(); }
    // The same table written straight from its blocks as the binary flow file (BFFLSOA1, event_reader.h); drains first.
    bool write_accumulated_device_binary(const std::string &path) {
        drain();
        return device_table ? device_table->write_binary(path) : DeviceFlowRows().write_binary(path);
    }
    size_t rows_accumulated_device() { return device_table ? device_table->rows() : 0; }

private:
    struct Pending {
        uint64_t index = 0, first = 0, n = 0, ring_size = 0, new_events = 0, trigger_plus1 = 0, protect = 0;
        ull start_time = 0, trigger_time = 0, oldest_time = 0;
        sll time_diff = 0;
        bool full = false, zero_excluded = false;
        std::shared_ptr<double> block;   // (u, v) pairs of the slice's events
    };

    // -- configuration: the caller's thread, before the first event
    size_t max_sz;
    sll span;
    ull on_ev_change, on_time_change;
    ull time_base = 0;
    int max_iter = -1, scale = 3;
    bool stm_disable = false, want_flow = true, accumulate = false, accumulate_device = false, pipelined = false, assume_sorted = true;
    std::vector<int> devices;
    int contexts_per_device = 1;
    size_t lookahead = 0;
    SliceFn slice_fn;
    bool frames_on = false;
    FrameSettings frame_cfg;
    // -- the failure of any slice or component (a lock of its own), and what ensure_ring() builds, in this order -- so
    // that the farm's contexts outlive everything allocated through them.  Constant once built.
    FailureLatch failure;
    std::unique_ptr<SliceFarm> farm;
    EventRing ring;                          // slots: the producer's until committed, then read by the slices that hold them
    std::unique_ptr<DeviceFlowTable> device_table;   // set_accumulate_device
    std::unique_ptr<FramePipeline> frames;           // set_frames
    // -- the producer's thread (add_event(s) / reserve / commit / recompute)
    HostFlowAccumulator history;             // set_accumulate (keep(): deliver(), see there)
    uint64_t head = 0;                       // events committed so far
    double blocked_s = 0;
    size_t ring_size = 0;                    // CircularArray::current_size
    bool stale = false;                      // !span_checked
    sll time_diff = 0, event_diff = 0;
    ull last_slice_time, current_slice_time;
    uint64_t slices_submitted = 0, last_trigger_plus1 = 0;
    // -- producer and workers, lock-free
    std::atomic<uint64_t> noise_live{0};               // 1 + arrival number of the newest event flagged as noise (0: none)
    std::atomic<uint64_t> protected_from{UINT64_MAX};  // oldest event a slice in flight still needs (UINT64_MAX: none)
    // -- results (worker thread -> caller), under `mu`
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Pending> pending;
    ObjectModel last_model;
    bf_run_info last_info;
    ull slices_done = 0, slices_skipped = 0, iterations_total = 0;
    uint64_t flow_through_plus1 = 0;         // events below this arrival number have been in a delivered slice

    size_t worker_of(bf_ctx *ctx) const {
        for (size_t w = 0; w < farm->workers(); ++w)
            if (farm->context(w) == ctx) return w;
        return 0;
    }

    static uint16_t narrow(uint32_t v) {
        if (v > 65535u) throw AccelError(BF_ERR_ARG, "StreamEngine: event address " + std::to_string(v) + " does not fit 16 bits");
        return (uint16_t)v;
    }
    bool want_flow_any() const { return want_flow || accumulate; }
    ull logical(uint64_t g) const { return ring.logical(g, time_base); }
    bool time_due(ull t) const { return !((sll)(t - last_slice_time) < (sll)on_time_change); }
    size_t slot_of(size_t idx) const { return ring.slot(head - 1 - idx); }
    double flow_of(size_t idx, int which) const {
        const uint64_t g = head - 1 - idx;
        if (!ring.uv || g + 1 > flow_through_plus1) return 0.0;   // newer than the last solved slice: Event(): best_u = best_v = 0
        return ring.uv[2 * ring.slot(g) + which];
    }

    void rethrow_failure() { failure.rethrow(); }

    // m more events are in the ring; `upto` = events committed after them (CircularArray::push_back x m + the bookkeeping
    // of DVS_flow::add_event for the last of them)
    void advance(uint64_t m, uint64_t upto) {
        ring_size = (ring_size + m < max_sz) ? (size_t)(ring_size + m) : max_sz;
        stale = true;
        head = upto;
        event_diff += (sll)m;
        current_slice_time = logical(upto - 1);
        time_diff = (sll)(current_slice_time - last_slice_time);
    }

    void trim() {   // CircularArray::fix_span, datastructures.h:46-59
        if (!stale) return;
        stale = false;
        if (ring_size == 0) return;
        const ull newest = logical(head - 1);
        uint64_t oldest = head - ring_size;
        if (assume_sorted) {   // the events too old form a prefix: find its end instead of walking it
            uint64_t lo = oldest, hi = head - 1;   // (the newest event is never too old)
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if ((sll)(newest - logical(mid)) > span) lo = mid + 1; else hi = mid;
            }
            ring_size -= (size_t)(lo - oldest);
            return;
        }
        while ((sll)(newest - logical(oldest)) > span) { ++oldest; --ring_size; }
    }

    // Built into locals and moved into the members at the end: a throw half-way leaves the engine as it was, and what had
    // been built destroys itself (in reverse order, the farm last).
    void ensure_ring() {
        if (farm) return;
        const bool chained = !stm_disable;
        if (chained && devices.size() * (size_t)contexts_per_device != 1)
            throw AccelError(BF_ERR_ARG, "StreamEngine: several devices / contexts need independent slices (set_stm_disable): a warm-start "
                                         "chain is sequential");
        if (frames_on && max_sz < 2)   // (a slice of a one-event ring is empty: the context would still hold the previous one)
            throw AccelError(BF_ERR_ARG, "StreamEngine: frames need a ring of at least 2 events");
        // (frames are rendered at scale 3: the colour tile is (3 RES_X + 3) x (3 RES_Y + 3), as DVS_flow reserves it)
        const int fs = frame_cfg.mosaic() ? 3 : 0;
        std::unique_ptr<SliceFarm> f(new SliceFarm(devices, contexts_per_device, (long long)max_sz, std::max(scale * RES_X + scale, fs * RES_X + fs),
                                                   std::max(scale * RES_Y + scale, fs * RES_Y + fs), [this](const SliceFarm::Result &r) { deliver(r); }, chained));
        const size_t extra = lookahead ? lookahead : (2 * max_sz > 65536 ? 2 * max_sz : 65536);   // the producer may run two slices ahead
        const size_t cap = max_sz + extra;
        if (accumulate_device) {
            if (!assume_sorted) throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs non-decreasing timestamps (set_assume_sorted)");
            if (span >= (sll)INT_MAX)
                throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs a span below 2^31 ns (slice-local times are int32 on the device)");
            for (int d : devices)
                if (d != devices[0]) throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs every context on one device");
        }
        std::vector<bf_ctx *> contexts;
        for (size_t w = 0; w < f->workers(); ++w) contexts.push_back(f->context(w));
        for (bf_ctx *c : contexts) (void)bf_set_option(c, "stream_prealloc", 1);   // staging slots, copy stream: now, not at the first slice
        EventRing r(contexts[0], cap, want_flow_any());
        std::unique_ptr<DeviceFlowTable> table;
        if (accumulate_device) table.reset(new DeviceFlowTable(contexts[0], cap, failure));
        std::unique_ptr<FramePipeline> fp;
        if (frames_on) {
            fp.reset(new FramePipeline(frame_cfg, failure));
            fp->start(contexts);
        }
        ring = std::move(r); device_table = std::move(table); frames = std::move(fp); farm = std::move(f);
    }

    // optimizer_rolling.h:49-55 evaluated on the host: the bounding box of the slice (set_cloud, :248-283) against RES / 15
    bool window_guard_on_host(const Pending &p) const {
        int x_min = RES_X, y_min = RES_Y, x_max = 0, y_max = 0;
        const RingPieces pieces = ring.pieces(p.first, (size_t)p.n);
        for (const RingPieces::Piece &w : pieces.p)
            for (size_t s = w.at; s < w.at + w.n; ++s) {
                const int x = ring.row[s], y = ring.col[s];
                x_min = x < x_min ? x : x_min; x_max = x > x_max ? x : x_max;
                y_min = y < y_min ? y : y_min; y_max = y > y_max ? y : y_max;
            }
        const int img_x = scale * (x_max - x_min) + scale, img_y = scale * (y_max - y_min) + scale;
        return (img_x < scale * RES_X / 15) && (img_y < scale * RES_Y / 15);
    }

    void flag_noise(const Pending &p) {   // `for (auto &e : *events) e.noise = true`, optimizer_rolling.h:52-53
        if (p.n == 0) return;
        ring_fill(ring.noise, ring.pieces(p.first, (size_t)p.n), 1);
        uint64_t cur = noise_live.load(std::memory_order_relaxed);
        while (cur < p.first + p.n && !noise_live.compare_exchange_weak(cur, p.first + p.n, std::memory_order_release)) {}
    }

    // a slice's result, in slice order, on a farm worker's thread
    void deliver(const SliceFarm::Result &r) {
        Pending p;
        {
            std::lock_guard<std::mutex> g(mu);
            p = pending.front();
        }
        if (r.rc < 0) {
            failure.fail(r.rc, "StreamEngine: slice " + std::to_string(p.index) + ": " + r.error);
        } else {
            // (several workers: recompute() has already flagged the slice from its own evaluation of the guard -- other
            // workers may be reading the noise ring right now)
            if (r.window_guard && farm->workers() == 1) flag_noise(p);
            // accumulate: the slice's own copy of the flow -> the ring's
            if (p.block && ring.uv) ring_copy_in((double *)ring.uv, (const double *)p.block.get(), ring.pieces(p.first, (size_t)p.n), 2);
            if (p.zero_excluded && ring.uv) { const size_t s = ring.slot(p.first - 1); ring.uv[2 * s] = ring.uv[2 * s + 1] = 0.0; }
        }
        if (device_table) device_table->collect(farm->context((size_t)r.worker), p.index);
        if (frames) {
            FrameFacts s;
            s.index = p.index; s.trigger_time = p.trigger_time; s.on_time_change = on_time_change; s.time_diff = p.time_diff;
            s.ring_size = (size_t)p.ring_size; s.new_events = (long long)p.new_events;
            frames->deliver(s, r);
        }
        SliceRecord rec;
        rec.index = p.index; rec.first_event = p.first; rec.events = p.n; rec.ring_size = p.ring_size; rec.new_events = p.new_events;
        rec.start_time = p.start_time; rec.trigger_time = p.trigger_time; rec.time_diff = p.time_diff;
        rec.oldest_time = p.oldest_time; rec.events_seen = p.trigger_plus1;
        rec.rc = r.rc; rec.window_guard = r.window_guard; rec.info = r.info; rec.model = ObjectModel(r.model); rec.ms = r.ms; rec.device = r.device;
        {
            std::lock_guard<std::mutex> g(mu);
            if (r.rc >= 0) {
                last_model = rec.model;
                last_info = r.info;
                ++slices_done;
                if (r.rc != 0) ++slices_skipped;
                iterations_total += (ull)r.info.iterations;
                if (accumulate) history.keep(HostFlowAccumulator::Kept{p.first, p.n, p.start_time, p.block, p.zero_excluded});
                if (p.trigger_plus1 > flow_through_plus1) flow_through_plus1 = p.trigger_plus1;
            }
        }
        if (slice_fn && r.rc >= 0) slice_fn(rec);
        {
            std::lock_guard<std::mutex> g(mu);
            pending.pop_front();
            protected_from.store(pending.empty() ? UINT64_MAX : pending.front().protect, std::memory_order_release);
        }
        cv.notify_all();
    }
};

// The reference's interface: ring size and span as template parameters, like DVS_flow<MAX_SZ, SPAN>.
template <size_t MAX_SZ, sll SPAN> class StreamFlow : public StreamEngine {
public:
    StreamFlow(ull on_ev_change_, ull on_time_change_, ull start_time = 0)
        : StreamEngine(MAX_SZ, SPAN, on_ev_change_, on_time_change_, start_time) {}
};

}  // namespace bf

#endif  // BF_HOST_STREAM_FLOW_H
