// stream_flow.h -- the slice former for high event rates: the reference's event ring and triggers
// (CircularArray, datastructures.h:6-115; DVS_flow::add_event / recompute, dvs_flow.h:164-347) on a
// structure-of-arrays ring in PINNED memory, handed to the device without a copy on the host, with the slices solved
// by a slice farm (better_flow/slice_farm.h).
//
// Why a second front end next to DVS_flow.  DVS_flow keeps the reference's public `ev_buffer` of 152-byte Event
// records: one add_event() call and one 152-byte store per event, and an AoS -> SoA repack per slice
// (accel_lib.h:91-99; AccelLib::init_gpu here) -- 23 Mevents/s end to end, against a device path that solves
// warm-started 1M-event slices at several Gevents/s.  Here
//   * the ring is three parallel arrays (u64 timestamp, u16 row, u16 column: 12 bytes per event, the column layout
//     of the binary event file) plus a lazily used Event::noise ring; a slice is one or two contiguous pieces of it,
//     copied by DMA (bf_upload_ring16_async), and Event::set_local_time runs on the device;
//   * events arrive in BULK: add_events(rows, cols, timestamps, n) copies a block into the ring, and
//     reserve() / commit() let a producer (a file reader, a socket) write into the ring itself -- then the only host
//     copy is the producer's own.  Trigger points inside a block are found by a binary search on the timestamps and
//     a subtraction on the counts, not by visiting every event;
//   * slices are solved by SliceFarm workers: with set_pipelined(true) the caller goes on filling the ring while
//     slice k is being solved and slice k + 1 uploaded (an STM chain stays sequential on one worker); with
//     --stm-disable style independent slices, several workers / GPUs take them in parallel.  Results are applied in
//     slice order either way;
//   * per-event flow comes back only if asked for (set_want_flow / set_accumulate), straight into a pinned (u, v) ring;
//   * set_accumulate_device: the same table as get_accumulated(), built on the device slice by slice (bf_emit_slice) --
//     no per-slice flow block, no history, no walk at the end; memory grows with the output rows only.  The solving worker
//     only enqueues the emit kernels; they store the rows in a pinned output ring, and deliver() -- in slice order, after
//     the solve -- waits for them and moves the rows into blocks of the table.
//   * set_frames: DVS_flow's --img / --video frame of every slice (dvs_flow.h render_frame), the same bytes.  The solving
//     worker enqueues the render and compose (bf_frame_render) into a pinned frame slot before its context takes the next
//     slice; deliver() waits for it in slice order and hands it to a writer thread, which writes the files and frees the slot.
//     A C-ABI library without the bf_frame_* entries (the CPU stand-in of the tests) gets the frame composed on the host
//     from bf_projection_img / bf_color_time_img (frame_writer.h): the same bytes again.
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
#include <better_flow/frame_writer.h>
#include <better_flow/object_model.h>
#include <better_flow/slice_farm.h>

#include <algorithm>
#include <memory>

// (weak: the host classes also link against C-ABI implementations that lack the device-side table -- the CPU stand-in the
// tests build -- and set_accumulate_device then fails at warm-up)
extern "C" {
int bf_emit_create(bf_ctx *ctx, int64_t ring_cap, int32_t rows, int32_t cols, int64_t out_rows, bf_emit **out) __attribute__((weak));
int bf_emit_destroy(bf_emit *emit) __attribute__((weak));
int bf_emit_output(bf_emit *emit, uint64_t **t, uint16_t **row, uint16_t **col, double **u, double **v, int64_t *out_rows)
    __attribute__((weak));
int bf_emit_slice(bf_ctx *ctx, bf_emit *emit, int64_t n, uint64_t first, uint64_t start_time, int32_t lead, uint64_t lead_t,
                  int32_t lead_row, int32_t lead_col, int64_t *ticket_out) __attribute__((weak));
int bf_emit_wait(bf_ctx *ctx, bf_emit *emit, int64_t ticket, uint64_t *first_row, int64_t *rows) __attribute__((weak));
int bf_emit_release(bf_emit *emit, uint64_t upto_row) __attribute__((weak));
// (weak for the same reason: without them set_frames composes on the host)
int bf_frame_create(bf_ctx *ctx, int32_t res_x, int32_t res_y, int32_t slots, int32_t layouts, bf_frame **out) __attribute__((weak));
int bf_frame_destroy(bf_frame *frame) __attribute__((weak));
int bf_frame_render(bf_ctx *ctx, bf_frame *frame, int64_t *ticket_out) __attribute__((weak));
int bf_frame_wait(bf_ctx *ctx, bf_frame *frame, int64_t ticket, const uint8_t **ppm, const uint8_t **avi) __attribute__((weak));
int bf_frame_release(bf_frame *frame, int64_t ticket) __attribute__((weak));
}

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

// What get_accumulated() returns: the -o table, one row per event.
struct FlowTable {
    std::vector<uint64_t> timestamp;   // ns
    std::vector<uint16_t> row, col;
    std::vector<double> u, v;          // best_u, best_v
    size_t size() const { return timestamp.size(); }
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
        : max_sz(max_sz_), span(span_), on_ev_change(on_ev_change_), on_time_change(on_time_change_), cap(0), ts(nullptr),
          row_(nullptr), col_(nullptr), noise(nullptr), uv(nullptr), head(0), ring_size(0), stale(false), time_diff(0),
          event_diff(0), last_slice_time(start_time), current_slice_time(start_time), time_base(0), max_iter(-1), scale(3),
          stm_disable(false), want_flow(true), accumulate(false), pipelined(false), assume_sorted(true),
          contexts_per_device(1), lookahead(0), slices_submitted(0), last_trigger_plus1(0), noise_live(0),
          protected_from(UINT64_MAX), slices_done(0), slices_skipped(0), iterations_total(0), flow_through_plus1(0),
          failed(false), fail_code(0) {
        if (max_sz < 1) throw AccelError(BF_ERR_ARG, "StreamEngine: ring capacity must be >= 1");
        std::memset(&last_info, 0, sizeof(last_info));
        devices.push_back(DeviceContext::device());
    }
    virtual ~StreamEngine() {
        if (farm) {
            try { farm->drain(); } catch (...) {}
            stop_frame_writer();
            for (bf_frame *f : frame_state) if (f) (void)bf_frame_destroy(f);
            bf_ctx *c = farm->context(0);
            if (ts) (void)bf_host_free(c, ts);
            if (row_) (void)bf_host_free(c, row_);
            if (col_) (void)bf_host_free(c, col_);
            if (noise) (void)bf_host_free(c, noise);
            if (uv) (void)bf_host_free(c, uv);
            if (emit_state && bf_emit_destroy) (void)bf_emit_destroy(emit_state);
        }
        farm.reset();
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
        frame_prefix = prefix; frame_pictures = pictures; frame_video_name = video_name; frame_video_fps = video_fps;
        frame_slots = slots < 1 ? 1 : slots;
        frames_on = pictures || !video_name.empty();
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
        const size_t room = cap - max_sz;
        if (want > room) want = room;
        uint64_t prot = protected_from.load(std::memory_order_acquire);
        if (prot != UINT64_MAX && head + 1 > prot + cap) {   // not even one slot: wait for the oldest slice in flight
            const auto t_wait = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { prot = protected_from.load(std::memory_order_acquire); return failed.load() || prot == UINT64_MAX || head + 1 <= prot + cap; });
            g.unlock();
            blocked_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count();
            rethrow_failure();
        }
        if (prot != UINT64_MAX && head + want > prot + cap) want = (size_t)(prot + cap - head);
        const size_t slot = (size_t)(head % cap);
        const size_t n0 = want < cap - slot ? want : cap - slot;
        out[0] = Span{ts + slot, row_ + slot, col_ + slot, n0};
        out[1] = Span{ts, row_, col_, want - n0};
        return want;
    }

    // The first n reserved slots now hold events: run the triggers over them.  Returns the number of slices closed.
    size_t commit(size_t n) {
        size_t slices = 0;
        uint64_t g = head;
        const uint64_t end = head + n;
        if (n == 0) return 0;
        if (noise_live.load(std::memory_order_relaxed) > 0) {   // new events are not noise (Event(x, y, t): noise(false)); before any
                                                                // flag was ever set the whole ring is still zero
            const size_t slot = (size_t)(g % cap), n0 = n < cap - slot ? n : cap - slot;
            std::memset(noise + slot, 0, n0);
            std::memset(noise, 0, n - n0);
        }
        if (accumulate) archive(g, end);
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
        t.ring_row = row_; t.ring_col = col_; t.ring_ts = ts; t.ring_noise = noise; t.noise_live = &noise_live;
        t.first_global = p.first;
        t.cap = (int64_t)cap; t.first = (int64_t)(p.first % cap); t.n = (int64_t)p.n;
        t.t0 = p.start_time + time_base;
        t.scale = scale; t.res_x = RES_X; t.res_y = RES_Y; t.max_iter = max_iter;
        t.warm = stm_disable ? SliceFarm::Warm::Cold : SliceFarm::Warm::FromPrevious;
        if (accumulate_device) {
            // (the lead: the ring's oldest element, left out of a full ring's slice, that no slice has held -- as Kept::lead)
            const bool lead = p.full && oldest + 1 > last_trigger_plus1;
            const size_t ls = (size_t)(oldest % cap);
            const ull lt = lead ? logical(oldest) : 0;
            const int lr = lead ? row_[ls] : 0, lc = lead ? col_[ls] : 0;
            const uint64_t idx = p.index, first = p.first, n = p.n;
            const ull st = p.start_time;
            t.want_uv = true;
            t.on_solved = [this, idx, first, n, st, lead, lt, lr, lc](bf_ctx *ctx, SliceFarm::Result &r) {
                emit_slice(idx, ctx, r, first, n, st, lead, lt, lr, lc);
                if (frames_on) frame_slice(idx, ctx, r);
            };
        } else if (frames_on) {
            const uint64_t idx = p.index;
            t.on_solved = [this, idx](bf_ctx *ctx, SliceFarm::Result &r) { frame_slice(idx, ctx, r); };
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
            t.uv_ring = uv; t.uv_cap = (int64_t)cap; t.uv_first = t.first;
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
        if (frames_on) {   // every frame delivered so far is in its files
            std::unique_lock<std::mutex> g(frame_mu);
            frame_cv.wait(g, [&] { return frame_queue.empty() && !frame_writing; });
        }
        rethrow_failure();
    }

    // ---- the ring, DVS_flow style (idx 0 = newest; CircularArray::operator[], :61-64).  Call drain() first in pipelined mode. ----
    size_t size() { trim(); return ring_size; }
    uint32_t row(size_t idx) const { return row_[slot_of(idx)]; }
    uint32_t col(size_t idx) const { return col_[slot_of(idx)]; }
    ull timestamp(size_t idx) const { return ts[slot_of(idx)] - time_base; }
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
    uint64_t frames_delivered() { std::lock_guard<std::mutex> g(frame_mu); return frames_handed; }
    // time the engine waited for frames: a free frame slot, a render to finish, room at the writer
    double seconds_frame_wait() { std::lock_guard<std::mutex> g(frame_mu); return frame_wait_s; }

    // DVS_flow::get_accumulated (dvs_flow.h:351-389): the events of all slices, each once, with the flow of the first
    // slice that solved it.  The marking rule is the reference's: walking the slices in order and, inside a slice, the
    // events oldest -> newest, an unmarked event e marks, in every LATER slice, the events of e's pixel that are not
    // after e in time and less than 0.1 ms before it (Event::operator==, event.h:39-45) -- its own later copies, and on
    // rare occasions another event; marked events are left out.  An event whose slice-local time is exactly -1 counts
    // as marked from the start (the reference uses t == -1 as the mark).
    FlowTable get_accumulated();
    // The same table, element for element, from the device (set_accumulate_device); drains first.
    FlowTable get_accumulated_device() {
        drain();
        std::lock_guard<std::mutex> g(emit_mu);
        FlowTable out;
        out.timestamp.resize(dev_rows); out.row.resize(dev_rows); out.col.resize(dev_rows); out.u.resize(dev_rows); out.v.resize(dev_rows);
        size_t at = 0;
        for (const RowBlock &b : dev_blocks) {
            std::memcpy(out.timestamp.data() + at, b.t.get(), b.n * 8);
            std::memcpy(out.row.data() + at, b.row.get(), b.n * 2);
            std::memcpy(out.col.data() + at, b.col.get(), b.n * 2);
            std::memcpy(out.u.data() + at, b.u.get(), b.n * 8);
            std::memcpy(out.v.data() + at, b.v.get(), b.n * 8);
            at += b.n;
        }
        return out;
    }
    // The same table written straight from its blocks as the binary flow file (BFFLSOA1, event_reader.h); drains first.
    bool write_accumulated_device_binary(const std::string &path) {
        drain();
        std::lock_guard<std::mutex> g(emit_mu);
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        const uint64_t n = dev_rows;
        bool w = std::fwrite("BFFLSOA1", 1, 8, f) == 8 && std::fwrite(&n, 8, 1, f) == 1;
        for (const RowBlock &b : dev_blocks) w = w && std::fwrite(b.t.get(), 8, b.n, f) == b.n;
        for (const RowBlock &b : dev_blocks) w = w && std::fwrite(b.row.get(), 2, b.n, f) == b.n;
        for (const RowBlock &b : dev_blocks) w = w && std::fwrite(b.col.get(), 2, b.n, f) == b.n;
        for (const RowBlock &b : dev_blocks) w = w && std::fwrite(b.u.get(), 8, b.n, f) == b.n;
        for (const RowBlock &b : dev_blocks) w = w && std::fwrite(b.v.get(), 8, b.n, f) == b.n;
        return std::fclose(f) == 0 && w;
    }
    size_t rows_accumulated_device() { std::lock_guard<std::mutex> g(emit_mu); return dev_rows; }

protected:
    struct Pending {
        uint64_t index = 0, first = 0, n = 0, ring_size = 0, new_events = 0, trigger_plus1 = 0, protect = 0;
        ull start_time = 0, trigger_time = 0, oldest_time = 0;
        sll time_diff = 0;
        bool full = false, zero_excluded = false;
        std::shared_ptr<double> block;   // (u, v) pairs of the slice's events
    };
    struct Kept {                 // accumulate: one solved slice
        uint64_t first, n;
        ull start_time;
        std::shared_ptr<double> block;   // (u, v) pairs of the slice's events
        bool lead;                // the ring was full and its oldest element (event first - 1, which the slice leaves out,
                                  // datastructures.h:71-76) had never been in a slice: the reference's copy of the ring
                                  // (dvs_flow.h:340-345) holds it too, with the zero flow of a fresh Event
    };

    // configuration
    size_t max_sz;
    sll span;
    ull on_ev_change, on_time_change;
    // the ring (pinned): event number g lives in slot g % cap, cap = MAX_SZ + lookahead
    size_t cap;
    uint64_t *ts;
    uint16_t *row_, *col_;
    uint8_t *noise;
    double *uv;
    uint64_t head;                // events committed so far
    double blocked_s = 0;
    size_t ring_size;             // CircularArray::current_size
    bool stale;                   // !span_checked
    sll time_diff, event_diff;
    ull last_slice_time, current_slice_time, time_base;
    int max_iter, scale;
    bool stm_disable, want_flow, accumulate, pipelined, assume_sorted;
    std::vector<int> devices;
    int contexts_per_device;
    size_t lookahead;
    SliceFn slice_fn;
    std::unique_ptr<SliceFarm> farm;
    uint64_t slices_submitted, last_trigger_plus1;
    std::atomic<uint64_t> noise_live;        // 1 + arrival number of the newest event flagged as noise (0: none)
    std::atomic<uint64_t> protected_from;    // oldest event a slice in flight still needs (UINT64_MAX: none)
    // results (worker thread -> caller), under `mu`
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Pending> pending;
    ObjectModel last_model;
    bf_run_info last_info;
    ull slices_done, slices_skipped, iterations_total;
    uint64_t flow_through_plus1;             // events below this arrival number have been in a delivered slice
    std::atomic<bool> failed;   // (read by the producer without the lock)
    int fail_code;
    std::string fail_text;
    // accumulate
    std::vector<uint64_t> hist_ts;           // logical timestamps of every event seen
    std::vector<uint16_t> hist_row, hist_col;
    std::vector<Kept> kept;
    // accumulate_device
    struct RowBlock {             // one slice's rows (uninitialised storage: every element is written)
        size_t n = 0;
        std::unique_ptr<uint64_t[]> t;
        std::unique_ptr<uint16_t[]> row, col;
        std::unique_ptr<double[]> u, v;
    };
    bool accumulate_device = false;
    bf_emit *emit_state = nullptr;
    std::mutex emit_mu;                      // enqueueing in slice order; the blocks
    std::condition_variable emit_cv;
    uint64_t emit_turn = 0;                  // index of the next slice to enqueue
    std::deque<int64_t> emit_tickets;        // per slice enqueued, in slice order: its ticket (-1: nothing emitted)
    uint64_t emit_released = 0;              // rows of the output ring read so far
    std::vector<RowBlock> dev_blocks;
    size_t dev_rows = 0;
    // frames (set_frames)
    struct FrameJob {             // one slice's frame, from its worker to the writer
        int worker = -1;
        int64_t ticket = -1;                  // device composition: the frame slot's ticket
        std::vector<uint8_t> host_ppm, host_avi;   // host composition: the payloads
        const uint8_t *ppm = nullptr, *avi = nullptr;
        std::string text;                     // the side-car
        uint64_t number = 0;                  // frame_<number>
    };
    bool frames_on = false, frame_pictures = false;
    std::string frame_prefix, frame_video_name;
    int frame_video_fps = 30, frame_slots = 4;
    std::vector<bf_frame *> frame_state;     // per worker (device composition); empty: host composition
    std::mutex frame_mu;                     // everything below
    std::condition_variable frame_cv;
    std::map<uint64_t, FrameJob> frame_ready;   // slice index -> its frame, from the worker's hook to deliver()
    std::vector<int> frame_held;             // per worker: slots rendered and not yet released
    std::deque<FrameJob> frame_queue;        // delivered, in slice order, for the writer
    bool frame_writing = false, frame_stop = false;
    uint64_t frames_handed = 0, frame_number = 0;
    double frame_wait_s = 0;
    std::thread frame_writer;
    AviWriter video;                         // (the writer's)

    // the emit step of slice `idx`, on the worker that solved it (SliceFarm::Task::on_solved): enqueue only
    void emit_slice(uint64_t idx, bf_ctx *ctx, SliceFarm::Result &r, uint64_t first, uint64_t n, ull start, bool lead, ull lead_t,
                    int lead_row, int lead_col) {
        std::unique_lock<std::mutex> g(emit_mu);
        emit_cv.wait(g, [&] { return emit_turn == idx; });
        int64_t ticket = -1;
        if (r.rc >= 0 && n + (lead ? 1 : 0) > 0) {
            for (;;) {
                const int rc = bf_emit_slice(ctx, emit_state, (int64_t)n, first, start, lead ? 1 : 0, lead_t, lead_row, lead_col, &ticket);
                if (rc == BF_ERR_CAPACITY && emit_tickets.size() > 0) {   // the output ring holds rows not read yet: wait for deliver()
                    const uint64_t seen = emit_released;
                    const size_t waiting = emit_tickets.size();
                    emit_cv.wait(g, [&] { return emit_released != seen || emit_tickets.size() != waiting; });
                    continue;
                }
                if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: emit failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); ticket = -1; }
                break;
            }
        }
        emit_tickets.push_back(ticket);
        ++emit_turn;
        g.unlock();
        emit_cv.notify_all();
    }

    // deliver(), in slice order: the slice's rows out of the output ring into a block of the table
    void collect_rows(bf_ctx *ctx, uint64_t index) {
        int64_t ticket;
        {
            std::lock_guard<std::mutex> g(emit_mu);
            ticket = emit_tickets.front();
        }
        RowBlock b;
        uint64_t first_row = 0;
        int64_t rows = 0;
        int rc = BF_OK;
        if (ticket >= 0 && (rc = bf_emit_wait(ctx, emit_state, ticket, &first_row, &rows)) == BF_OK && rows > 0) {
            uint64_t *rt; uint16_t *rr, *rcol; double *ru, *rv; int64_t R;
            (void)bf_emit_output(emit_state, &rt, &rr, &rcol, &ru, &rv, &R);
            b.n = (size_t)rows;
            b.t.reset(new uint64_t[b.n]); b.row.reset(new uint16_t[b.n]); b.col.reset(new uint16_t[b.n]);
            b.u.reset(new double[b.n]); b.v.reset(new double[b.n]);
            const size_t s0 = (size_t)(first_row % (uint64_t)R), n0 = b.n < (size_t)R - s0 ? b.n : (size_t)R - s0;
            auto two = [&](void *dst, const void *src, size_t el) {
                std::memcpy(dst, (const char *)src + s0 * el, n0 * el);
                std::memcpy((char *)dst + n0 * el, src, (b.n - n0) * el);
            };
            two(b.t.get(), rt, 8); two(b.row.get(), rr, 2); two(b.col.get(), rcol, 2); two(b.u.get(), ru, 8); two(b.v.get(), rv, 8);
            (void)bf_emit_release(emit_state, first_row + (uint64_t)rows);
        }
        {
            std::lock_guard<std::mutex> g(emit_mu);
            emit_tickets.pop_front();
            if (rc < 0) {
                if (!failed) { fail_code = rc; fail_text = "StreamEngine: slice " + std::to_string(index) + ": emit: " + bf_last_error(ctx); failed = true; }
            } else if (b.n) {
                dev_rows += b.n;
                emit_released += b.n;
                dev_blocks.push_back(std::move(b));
            }
        }
        emit_cv.notify_all();
    }

    size_t worker_of(bf_ctx *ctx) const {
        for (size_t w = 0; w < farm->workers(); ++w)
            if (farm->context(w) == ctx) return w;
        return 0;
    }

    void start_frames() {
        frame_held.assign(farm->workers(), 0);
        if (bf_frame_create) {
            const int layouts = (frame_pictures ? BF_FRAME_PPM : 0) | (frame_video_name.empty() ? 0 : BF_FRAME_AVI);
            for (size_t w = 0; w < farm->workers(); ++w) {
                bf_frame *f = nullptr;
                const int rc = bf_frame_create(farm->context(w), RES_X, RES_Y, frame_slots, layouts, &f);
                if (rc < 0) throw AccelError(rc, std::string("StreamEngine: bf_frame_create failed: ") + bf_last_error(farm->context(w)));
                frame_state.push_back(f);
            }
        }
        frame_writer = std::thread([this] { write_frames(); });
    }

    void stop_frame_writer() {
        if (!frame_writer.joinable()) return;
        {
            std::lock_guard<std::mutex> g(frame_mu);
            frame_stop = true;
        }
        frame_cv.notify_all();
        frame_writer.join();
        video.close();
    }

    // the frame of slice `idx`, on the worker that solved it (SliceFarm::Task::on_solved), before its context takes the next
    // slice: enqueued into a frame slot (waiting for one if all are taken), or composed here on the host
    void frame_slice(uint64_t idx, bf_ctx *ctx, SliceFarm::Result &r) {
        FrameJob job;
        job.worker = (int)worker_of(ctx);
        if (r.rc >= 0 && !frame_state.empty()) {
            bf_frame *f = frame_state[(size_t)job.worker];
            bool retried = false;   // (only this worker renders into f, so a slot counted free here is free in f)
            for (;;) {
                const int rc = bf_frame_render(ctx, f, &job.ticket);
                if (rc == BF_ERR_CAPACITY) {
                    std::unique_lock<std::mutex> g(frame_mu);
                    if (frame_held[(size_t)job.worker] >= frame_slots) {   // every slot holds a frame not yet written: wait for one
                        const auto t0 = std::chrono::steady_clock::now();
                        frame_cv.wait(g, [&] { return frame_held[(size_t)job.worker] < frame_slots || failed.load(); });
                        frame_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                        retried = false;
                        if (!failed) continue;
                    } else if (!retried) {   // the writer freed a slot since the call: once more
                        retried = true;
                        continue;
                    }
                }
                if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: frame render failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); job.ticket = -1; }
                else { std::lock_guard<std::mutex> g(frame_mu); ++frame_held[(size_t)job.worker]; }
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
                if (frame_pictures) { job.host_ppm.resize(fr.px.size()); ppm_payload(fr, job.host_ppm.data()); }
                if (!frame_video_name.empty()) { job.host_avi.resize(avi_stride(fr.cols) * (size_t)fr.rows); avi_payload(fr, job.host_avi.data()); }
            }
        }
        std::lock_guard<std::mutex> g(frame_mu);
        frame_ready[idx] = std::move(job);
    }

    // deliver(), in slice order: wait for the slice's frame and hand it to the writer
    void deliver_frame(const Pending &p, const SliceFarm::Result &r) {
        FrameJob job;
        {
            std::lock_guard<std::mutex> g(frame_mu);
            auto it = frame_ready.find(p.index);
            if (it == frame_ready.end()) return;
            job = std::move(it->second);
            frame_ready.erase(it);
        }
        if (r.rc < 0) {   // (failed: nothing to write; the slot goes back)
            if (job.ticket >= 0) {
                (void)bf_frame_release(frame_state[(size_t)job.worker], job.ticket);
                std::lock_guard<std::mutex> g(frame_mu);
                --frame_held[(size_t)job.worker];
            }
            frame_cv.notify_all();
            return;
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (job.ticket >= 0) {
            bf_ctx *ctx = farm->context((size_t)job.worker);
            const int rc = bf_frame_wait(ctx, frame_state[(size_t)job.worker], job.ticket, &job.ppm, &job.avi);
            if (rc < 0) {
                {
                    std::lock_guard<std::mutex> g(mu);
                    if (!failed) { fail_code = rc; fail_text = "StreamEngine: slice " + std::to_string(p.index) + ": frame: " + bf_last_error(ctx); failed = true; }
                }
                (void)bf_frame_release(frame_state[(size_t)job.worker], job.ticket);
                {
                    std::lock_guard<std::mutex> g(frame_mu);
                    --frame_held[(size_t)job.worker];
                }
                frame_cv.notify_all();
                return;
            }
        } else {
            job.ppm = job.host_ppm.empty() ? nullptr : job.host_ppm.data();
            job.avi = job.host_avi.empty() ? nullptr : job.host_avi.data();
        }
        if (frame_pictures)
            job.text = frame_sidecar(p.trigger_time, on_time_change, p.time_diff, (size_t)p.ring_size, (long long)p.new_events, ObjectModel(r.model));
        std::unique_lock<std::mutex> g(frame_mu);
        if (frame_pictures) job.number = frame_number++;
        // (host composition holds its frames in the queue: keep it short)
        if (frame_state.empty()) frame_cv.wait(g, [&] { return frame_queue.size() < (size_t)frame_slots || frame_stop; });
        frame_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        frame_queue.push_back(std::move(job));
        ++frames_handed;
        g.unlock();
        frame_cv.notify_all();
    }

    // the writer thread: the files of every delivered frame, in slice order; then the frame's slot is free again
    void write_frames() {
        const int rows = 6 * RES_X, cols = 6 * RES_Y;
        for (;;) {
            FrameJob job;
            {
                std::unique_lock<std::mutex> g(frame_mu);
                frame_cv.wait(g, [&] { return frame_stop || !frame_queue.empty(); });
                if (frame_queue.empty()) return;
                job = std::move(frame_queue.front());
                frame_queue.pop_front();
                frame_writing = true;
            }
            if (frame_pictures && job.ppm) {
                const std::string base = frame_prefix + "/frame_" + std::to_string(job.number);
                if (!write_ppm_raw(base + ".ppm", rows, cols, job.ppm)) std::cerr << "cannot write " << base << ".ppm\n";
                (void)write_text(base + ".txt", job.text);
            }
            if (!frame_video_name.empty() && job.avi) {
                if (!video.is_open() && !video.open(frame_video_name, rows, cols, frame_video_fps))
                    std::cout << "Could not open the output video for write" << std::endl;
                if (video.is_open()) video.write_raw(job.avi);
            }
            if (job.ticket >= 0) (void)bf_frame_release(frame_state[(size_t)job.worker], job.ticket);
            {
                std::lock_guard<std::mutex> g(frame_mu);
                if (job.ticket >= 0) --frame_held[(size_t)job.worker];
                frame_writing = false;
            }
            frame_cv.notify_all();
        }
    }

    static uint16_t narrow(uint32_t v) {
        if (v > 65535u) throw AccelError(BF_ERR_ARG, "StreamEngine: event address " + std::to_string(v) + " does not fit 16 bits");
        return (uint16_t)v;
    }
    bool want_flow_any() const { return want_flow || accumulate; }
    ull logical(uint64_t g) const { return ts[g % cap] - time_base; }
    bool time_due(ull t) const { return !((sll)(t - last_slice_time) < (sll)on_time_change); }
    size_t slot_of(size_t idx) const { return (size_t)((head - 1 - idx) % cap); }
    double flow_of(size_t idx, int which) const {
        const uint64_t g = head - 1 - idx;
        if (!uv || g + 1 > flow_through_plus1) return 0.0;   // newer than the last solved slice: Event(): best_u = best_v = 0
        return uv[2 * (g % cap) + which];
    }

    void rethrow_failure() {
        if (!failed) return;
        std::lock_guard<std::mutex> g(mu);
        throw AccelError(fail_code, fail_text);
    }

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

    void ensure_ring() {
        if (farm) return;
        const bool chained = !stm_disable;
        if (chained && devices.size() * (size_t)contexts_per_device != 1)
            throw AccelError(BF_ERR_ARG, "StreamEngine: several devices / contexts need independent slices (set_stm_disable): a warm-start "
                                         "chain is sequential");
        if (frames_on && max_sz < 2)   // (a slice of a one-event ring is empty: the context would still hold the previous one)
            throw AccelError(BF_ERR_ARG, "StreamEngine: frames need a ring of at least 2 events");
        // (frames are rendered at scale 3: the colour tile is (3 RES_X + 3) x (3 RES_Y + 3), as DVS_flow reserves it)
        const int fs = frames_on ? 3 : 0;
        farm.reset(new SliceFarm(devices, contexts_per_device, (long long)max_sz, std::max(scale * RES_X + scale, fs * RES_X + fs),
                                 std::max(scale * RES_Y + scale, fs * RES_Y + fs), [this](const SliceFarm::Result &r) { deliver(r); }, chained));
        size_t extra = lookahead ? lookahead : (2 * max_sz > 65536 ? 2 * max_sz : 65536);   // the producer may run two slices ahead
        cap = max_sz + extra;
        if (accumulate_device) {
            if (!assume_sorted) throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs non-decreasing timestamps (set_assume_sorted)");
            if (span >= (sll)INT_MAX)
                throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs a span below 2^31 ns (slice-local times are int32 on the device)");
            for (int d : devices)
                if (d != devices[0]) throw AccelError(BF_ERR_ARG, "StreamEngine: the device-accumulated table needs every context on one device");
        }
        for (size_t w = 0; w < farm->workers(); ++w) (void)bf_set_option(farm->context(w), "stream_prealloc", 1);   // staging slots, copy stream: now, not at the first slice
        bf_ctx *c = farm->context(0);
        void *p = nullptr;   // (pinned host memory is not tied to the ctx object)
        auto alloc = [&](size_t bytes) {
            const int rc = bf_host_alloc(c, (int64_t)bytes, &p);
            if (rc < 0) throw AccelError(rc, std::string("StreamEngine: pinned allocation failed: ") + bf_last_error(c));
            return p;
        };
        ts = (uint64_t *)alloc(cap * 8);
        row_ = (uint16_t *)alloc(cap * 2);
        col_ = (uint16_t *)alloc(cap * 2);
        noise = (uint8_t *)alloc(cap);
        std::memset(noise, 0, cap);
        if (want_flow_any()) { uv = (double *)alloc(cap * 16); std::memset(uv, 0, cap * 16); }
        if (accumulate_device) {
            if (!bf_emit_create) throw AccelError(BF_ERR_STATE, "StreamEngine: this C-ABI library has no device-side flow table (bf_emit_create)");
            // (the output ring: a slice emits at most max_sz + 1 rows, and rows wait there only until their slice is delivered)
            const int rc = bf_emit_create(c, (int64_t)cap, RES_X, RES_Y, (int64_t)cap, &emit_state);
            if (rc < 0) throw AccelError(rc, std::string("StreamEngine: bf_emit_create failed: ") + bf_last_error(c));
        }
        if (frames_on) start_frames();
    }

    void archive(uint64_t g, uint64_t end) {   // (two contiguous pieces of the ring, appended in bulk)
        const size_t n = (size_t)(end - g), at = hist_ts.size();
        hist_ts.resize(at + n); hist_row.resize(at + n); hist_col.resize(at + n);
        const size_t slot = (size_t)(g % cap), n0 = n < cap - slot ? n : cap - slot;
        const ull base = time_base;
        for (size_t i = 0; i < n0; ++i) hist_ts[at + i] = ts[slot + i] - base;
        for (size_t i = n0; i < n; ++i) hist_ts[at + i] = ts[i - n0] - base;
        std::memcpy(hist_row.data() + at, row_ + slot, n0 * 2); std::memcpy(hist_row.data() + at + n0, row_, (n - n0) * 2);
        std::memcpy(hist_col.data() + at, col_ + slot, n0 * 2); std::memcpy(hist_col.data() + at + n0, col_, (n - n0) * 2);
    }

    // optimizer_rolling.h:49-55 evaluated on the host: the bounding box of the slice (set_cloud, :248-283) against RES / 15
    bool window_guard_on_host(const Pending &p) const {
        int x_min = RES_X, y_min = RES_Y, x_max = 0, y_max = 0;
        for (uint64_t g = p.first; g < p.first + p.n; ++g) {
            const size_t s = (size_t)(g % cap);
            const int x = row_[s], y = col_[s];
            x_min = x < x_min ? x : x_min; x_max = x > x_max ? x : x_max;
            y_min = y < y_min ? y : y_min; y_max = y > y_max ? y : y_max;
        }
        const int img_x = scale * (x_max - x_min) + scale, img_y = scale * (y_max - y_min) + scale;
        return (img_x < scale * RES_X / 15) && (img_y < scale * RES_Y / 15);
    }

    void flag_noise(const Pending &p) {   // `for (auto &e : *events) e.noise = true`, optimizer_rolling.h:52-53
        if (p.n == 0) return;
        const size_t slot = (size_t)(p.first % cap), n0 = p.n < cap - slot ? (size_t)p.n : cap - slot;
        std::memset(noise + slot, 1, n0);
        std::memset(noise, 1, (size_t)p.n - n0);
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
            std::lock_guard<std::mutex> g(mu);
            if (!failed) { fail_code = r.rc; fail_text = "StreamEngine: slice " + std::to_string(p.index) + ": " + r.error; failed = true; }
        } else {
            // (several workers: recompute() has already flagged the slice from its own evaluation of the guard -- other
            // workers may be reading the noise ring right now)
            if (r.window_guard && farm->workers() == 1) flag_noise(p);
            if (p.block && uv) {   // accumulate: the slice's own copy of the flow -> the ring's
                const size_t slot = (size_t)(p.first % cap), n0 = p.n < cap - slot ? (size_t)p.n : cap - slot;
                std::memcpy(uv + 2 * slot, p.block.get(), n0 * 16);
                std::memcpy(uv, p.block.get() + 2 * n0, ((size_t)p.n - n0) * 16);
            }
            if (p.zero_excluded && uv) { const size_t s = (size_t)((p.first - 1) % cap); uv[2 * s] = uv[2 * s + 1] = 0.0; }
        }
        if (accumulate_device) collect_rows(farm->context((size_t)r.worker), p.index);
        if (frames_on) deliver_frame(p, r);
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
                if (accumulate) kept.push_back(Kept{p.first, p.n, p.start_time, p.block, p.zero_excluded});
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

inline FlowTable StreamEngine::get_accumulated() {
    drain();
    FlowTable out;
    const size_t K = kept.size();
    const uint64_t N = hist_ts.size();
    if (N >= 0xffffffffull) throw AccelError(BF_ERR_CAPACITY, "StreamEngine::get_accumulated: more than 2^32 - 2 events");
    // chains of events at the same pixel: previous / next event of g's pixel in arrival order
    const uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> prev(N, NONE), next(N, NONE);
    {
        uint32_t max_col = 0;
        for (uint64_t g = 0; g < N; ++g) max_col = hist_col[g] > max_col ? hist_col[g] : max_col;
        uint32_t max_row = 0;
        for (uint64_t g = 0; g < N; ++g) max_row = hist_row[g] > max_row ? hist_row[g] : max_row;
        std::vector<uint32_t> last((size_t)(max_row + 1) * (max_col + 1), NONE);
        for (uint64_t g = 0; g < N; ++g) {
            uint32_t &l = last[(size_t)hist_row[g] * (max_col + 1) + hist_col[g]];
            prev[g] = l;
            if (l != NONE) next[l] = (uint32_t)g;
            l = (uint32_t)g;
        }
    }
    std::vector<std::vector<uint8_t>> mark(K);
    size_t copies = 0;
    for (size_t i = 0; i < K; ++i) {
        mark[i].assign((size_t)kept[i].n, 0);
        copies += (size_t)kept[i].n;
        for (uint64_t p = 0; p < kept[i].n && hist_ts[kept[i].first + p] < kept[i].start_time; ++p)   // slice-local t == -1
            if (hist_ts[kept[i].first + p] + 1 == kept[i].start_time) mark[i][(size_t)p] = 1;
    }
    out.timestamp.reserve(N); out.row.reserve(N); out.col.reserve(N); out.u.reserve(N); out.v.reserve(N);
    (void)copies;
    auto mark_later = [&](size_t i, uint64_t c) {   // event c in the slices after i that hold it
        for (size_t j = i + 1; j < K && kept[j].first <= c; ++j)
            if (c < kept[j].first + kept[j].n) mark[j][(size_t)(c - kept[j].first)] = 1;
    };
    auto emit = [&](size_t i, uint64_t g, double eu, double ev) {   // an unmarked event of slice i: mark its later copies, write it
        const uint64_t t = hist_ts[g];
        if (i + 1 < K) {
            mark_later(i, g);
            for (uint32_t c = prev[g]; c != NONE && t - hist_ts[c] < 100000ull; c = prev[c]) mark_later(i, c);   // dt < 0.1 ms
            for (uint32_t c = next[g]; c != NONE && hist_ts[c] == t; c = next[c]) mark_later(i, c);             // same instant, arrived later
        }
        out.timestamp.push_back(t); out.row.push_back(hist_row[g]); out.col.push_back(hist_col[g]);
        out.u.push_back(eu); out.v.push_back(ev);
    };
    for (size_t i = 0; i < K; ++i) {
        const Kept &s = kept[i];
        // (its t is the raw timestamp -- it never saw set_local_time --, so the t == -1 mark does not apply to it)
        if (s.lead) emit(i, s.first - 1, 0.0, 0.0);
        for (uint64_t p = 0; p < s.n; ++p) {
            if (mark[i][(size_t)p]) continue;
            emit(i, s.first + p, s.block.get()[2 * (size_t)p], s.block.get()[2 * (size_t)p + 1]);
        }
    }
    return out;
}

// The reference's interface: ring size and span as template parameters, like DVS_flow<MAX_SZ, SPAN>.
template <size_t MAX_SZ, sll SPAN> class StreamFlow : public StreamEngine {
public:
    StreamFlow(ull on_ev_change_, ull on_time_change_, ull start_time = 0)
        : StreamEngine(MAX_SZ, SPAN, on_ev_change_, on_time_change_, start_time) {}
};

}  // namespace bf

#endif  // BF_HOST_STREAM_FLOW_H
