// flow_table.h -- the -o table of the stream engine (one row per event: timestamp, row, column, best_u, best_v), built
// two ways that give the same table element for element:
//   * HostFlowAccumulator (set_accumulate): every event seen and every solved slice's flow block are kept, and table()
//     walks them at the end -- DVS_flow::get_accumulated (dvs_flow.h:351-389) with its exact marking rule;
//   * DeviceFlowTable (set_accumulate_device): the same table built on the device slice by slice (bf_emit_slice) -- no
//     per-slice flow block, no history, no walk at the end; memory grows with the output rows only.  The solving worker
//     only enqueues the emit kernels; they store the rows in a pinned output ring, and the engine's deliver() -- in slice
//     order, after the solve -- waits for them and moves the rows into blocks of the table.
#ifndef BF_HOST_FLOW_TABLE_H
#define BF_HOST_FLOW_TABLE_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>
#include <better_flow/event_ring.h>
#include <better_flow/failure_latch.h>
#include <better_flow/slice_farm.h>

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
}

namespace bf {

// What get_accumulated() returns: the -o table, one row per event.
struct FlowTable {
    std::vector<uint64_t> timestamp;   // ns
    std::vector<uint16_t> row, col;
    std::vector<double> u, v;          // best_u, best_v
    size_t size() const { return timestamp.size(); }
};

// The history of a stream and the marking rule over it.  No lock: archive() runs on the producer's thread, keep() in the
// engine's deliver() (one slice at a time, in slice order), table() on the caller's thread after a drain.
class HostFlowAccumulator {
public:
    struct Kept {                 // one solved slice
        uint64_t first, n;
        ull start_time;
        std::shared_ptr<double> block;   // (u, v) pairs of the slice's events
        bool lead;                // the ring was full and its oldest element (event first - 1, which the slice leaves out,
                                  // datastructures.h:71-76) had never been in a slice: the reference's copy of the ring
                                  // (dvs_flow.h:340-345) holds it too, with the zero flow of a fresh Event
    };

    // events [g, end) of the ring, with their logical timestamps, appended in bulk
    void archive(const EventRing &ring, uint64_t g, uint64_t end, ull time_base) {
        const size_t n = (size_t)(end - g), at = hist_ts.size();
        hist_ts.resize(at + n); hist_row.resize(at + n); hist_col.resize(at + n);
        const RingPieces w = ring.pieces(g, n);
        uint64_t *out = hist_ts.data() + at;
        for (const RingPieces::Piece &p : w.p)
            for (size_t i = 0; i < p.n; ++i) *out++ = ring.ts[p.at + i] - time_base;
        ring_copy_out(hist_row.data() + at, (const uint16_t *)ring.row, w);
        ring_copy_out(hist_col.data() + at, (const uint16_t *)ring.col, w);
    }
    void keep(const Kept &k) { kept.push_back(k); }

    // DVS_flow::get_accumulated (dvs_flow.h:351-389): the events of all slices, each once, with the flow of the first
    // slice that solved it.  The marking rule is the reference's: walking the slices in order and, inside a slice, the
    // events oldest -> newest, an unmarked event e marks, in every LATER slice, the events of e's pixel that are not
    // after e in time and less than 0.1 ms before it (Event::operator==, event.h:39-45) -- its own later copies, and on
    // rare occasions another event; marked events are left out.  An event whose slice-local time is exactly -1 counts
    // as marked from the start (the reference uses t == -1 as the mark).
    FlowTable table() const;

private:
    std::vector<uint64_t> hist_ts;           // logical timestamps of every event seen
    std::vector<uint16_t> hist_row, hist_col;
    std::vector<Kept> kept;
};

inline FlowTable HostFlowAccumulator::table() const {
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
    for (size_t i = 0; i < K; ++i) {
        mark[i].assign((size_t)kept[i].n, 0);
        for (uint64_t p = 0; p < kept[i].n && hist_ts[kept[i].first + p] < kept[i].start_time; ++p)   // slice-local t == -1
            if (hist_ts[kept[i].first + p] + 1 == kept[i].start_time) mark[i][(size_t)p] = 1;
    }
    out.timestamp.reserve(N); out.row.reserve(N); out.col.reserve(N); out.u.reserve(N); out.v.reserve(N);
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

// What the emit step needs to know of a slice, built once at its trigger.
struct EmitSlice {
    uint64_t first = 0, n = 0;    // arrival number of its oldest event; events
    ull start_time = 0;
    // the lead: the ring's oldest element, left out of a full ring's slice, that no slice has held -- as Kept::lead
    bool lead = false;
    ull lead_t = 0;
    int lead_row = 0, lead_col = 0;
};

// The rows the device has emitted, slice by slice.  No lock of its own (DeviceFlowTable keeps it under its lock).
struct DeviceFlowRows {
    struct Block {                // one slice's rows (uninitialised storage: every element is written)
        size_t n = 0;
        std::unique_ptr<uint64_t[]> t;
        std::unique_ptr<uint16_t[]> row, col;
        std::unique_ptr<double[]> u, v;
    };
    std::vector<Block> blocks;
    size_t n = 0;                 // rows in all blocks

    FlowTable table() const {
        FlowTable out;
        out.timestamp.resize(n); out.row.resize(n); out.col.resize(n); out.u.resize(n); out.v.resize(n);
        size_t at = 0;
        for (const Block &b : blocks) {
            std::memcpy(out.timestamp.data() + at, b.t.get(), b.n * 8);
            std::memcpy(out.row.data() + at, b.row.get(), b.n * 2);
            std::memcpy(out.col.data() + at, b.col.get(), b.n * 2);
            std::memcpy(out.u.data() + at, b.u.get(), b.n * 8);
            std::memcpy(out.v.data() + at, b.v.get(), b.n * 8);
            at += b.n;
        }
        return out;
    }
    // The table written straight from its blocks as the binary flow file (BFFLSOA1, event_reader.h)
    bool write_binary(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        const uint64_t rows = n;
        bool w = std::fwrite("BFFLSOA1", 1, 8, f) == 8 && std::fwrite(&rows, 8, 1, f) == 1;
        for (const Block &b : blocks) w = w && std::fwrite(b.t.get(), 8, b.n, f) == b.n;
        for (const Block &b : blocks) w = w && std::fwrite(b.row.get(), 2, b.n, f) == b.n;
        for (const Block &b : blocks) w = w && std::fwrite(b.col.get(), 2, b.n, f) == b.n;
        for (const Block &b : blocks) w = w && std::fwrite(b.u.get(), 8, b.n, f) == b.n;
        for (const Block &b : blocks) w = w && std::fwrite(b.v.get(), 8, b.n, f) == b.n;
        return std::fclose(f) == 0 && w;
    }
};

// The table on the device.  One lock, `mu`, for every member below it; `emit` itself is constant after construction.
// enqueue(): the farm's workers, each for the slice it solved; collect(): the engine's deliver(), in slice order.
class DeviceFlowTable {
public:
    // `ctx`: a context on the device of every worker; ring_cap: the event ring's slots.  Throws bf::AccelError.
    DeviceFlowTable(bf_ctx *ctx, size_t ring_cap, FailureLatch &failure_) : failure(failure_) {
        if (!bf_emit_create) throw AccelError(BF_ERR_STATE, "StreamEngine: this C-ABI library has no device-side flow table (bf_emit_create)");
        // (the output ring: a slice emits at most max_sz + 1 rows, and rows wait there only until their slice is delivered)
        const int rc = bf_emit_create(ctx, (int64_t)ring_cap, RES_X, RES_Y, (int64_t)ring_cap, &emit);
        if (rc < 0) throw AccelError(rc, std::string("StreamEngine: bf_emit_create failed: ") + bf_last_error(ctx));
    }
    ~DeviceFlowTable() { (void)bf_emit_destroy(emit); }
    DeviceFlowTable(const DeviceFlowTable &) = delete;
    DeviceFlowTable &operator=(const DeviceFlowTable &) = delete;

    // the emit step of slice `idx`, on the worker that solved it (SliceFarm::Task::on_solved): enqueue only
    void enqueue(uint64_t idx, bf_ctx *ctx, SliceFarm::Result &r, const EmitSlice &s) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return turn == idx; });
        int64_t ticket = -1;
        if (r.rc >= 0 && s.n + (s.lead ? 1 : 0) > 0) {
            for (;;) {
                const int rc = bf_emit_slice(ctx, emit, (int64_t)s.n, s.first, s.start_time, s.lead ? 1 : 0, s.lead_t, s.lead_row, s.lead_col, &ticket);
                if (rc == BF_ERR_CAPACITY && tickets.size() > 0) {   // the output ring holds rows not read yet: wait for deliver()
                    const uint64_t seen = released;
                    const size_t waiting = tickets.size();
                    cv.wait(g, [&] { return released != seen || tickets.size() != waiting; });
                    continue;
                }
                if (rc < 0) { r.rc = rc; r.error = std::string("SliceFarm: emit failed (") + std::to_string(rc) + "): " + bf_last_error(ctx); ticket = -1; }
                break;
            }
        }
        tickets.push_back(ticket);
        ++turn;
        g.unlock();
        cv.notify_all();
    }

    // deliver(), in slice order: the slice's rows out of the output ring into a block of the table
    void collect(bf_ctx *ctx, uint64_t index) {
        int64_t ticket;
        {
            std::lock_guard<std::mutex> g(mu);
            ticket = tickets.front();
        }
        DeviceFlowRows::Block b;
        uint64_t first_row = 0;
        int64_t rows = 0;
        int rc = BF_OK;
        if (ticket >= 0 && (rc = bf_emit_wait(ctx, emit, ticket, &first_row, &rows)) == BF_OK && rows > 0) {
            uint64_t *rt; uint16_t *rr, *rcol; double *ru, *rv; int64_t R;
            (void)bf_emit_output(emit, &rt, &rr, &rcol, &ru, &rv, &R);
            b.n = (size_t)rows;
            b.t.reset(new uint64_t[b.n]); b.row.reset(new uint16_t[b.n]); b.col.reset(new uint16_t[b.n]);
            b.u.reset(new double[b.n]); b.v.reset(new double[b.n]);
            const RingPieces w = ring_pieces(first_row, b.n, (size_t)R);
            ring_copy_out(b.t.get(), rt, w); ring_copy_out(b.row.get(), rr, w); ring_copy_out(b.col.get(), rcol, w);
            ring_copy_out(b.u.get(), ru, w); ring_copy_out(b.v.get(), rv, w);
            (void)bf_emit_release(emit, first_row + (uint64_t)rows);
        }
        if (rc < 0) failure.fail(rc, "StreamEngine: slice " + std::to_string(index) + ": emit: " + bf_last_error(ctx));
        {
            std::lock_guard<std::mutex> g(mu);
            tickets.pop_front();
            if (rc >= 0 && b.n) {
                done.n += b.n;
                released += b.n;
                done.blocks.push_back(std::move(b));
            }
        }
        cv.notify_all();
    }

    void wake() { wake_waiters(mu, cv); }   // (the engine's failure waker)

    // The table, element for element that of HostFlowAccumulator::table(); the binary flow file; its rows.  After a drain.
    FlowTable table() { std::lock_guard<std::mutex> g(mu); return done.table(); }
    bool write_binary(const std::string &path) { std::lock_guard<std::mutex> g(mu); return done.write_binary(path); }
    size_t rows() { std::lock_guard<std::mutex> g(mu); return done.n; }

private:
    FailureLatch &failure;
    bf_emit *emit = nullptr;
    std::mutex mu;                           // enqueueing in slice order; the blocks
    std::condition_variable cv;
    uint64_t turn = 0;                       // index of the next slice to enqueue
    std::deque<int64_t> tickets;             // per slice enqueued, in slice order: its ticket (-1: nothing emitted)
    uint64_t released = 0;                   // rows of the output ring read so far
    DeviceFlowRows done;                     // the slices collected so far
};

}  // namespace bf

#endif  // BF_HOST_FLOW_TABLE_H
