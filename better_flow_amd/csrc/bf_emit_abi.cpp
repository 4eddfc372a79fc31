// bf_emit_abi.cpp -- C-ABI of the device-side -o table (include/bf_accel.h, "per-event flow table on the device"): the state that
// persists from slice to slice (covered plane by ring position, per-pixel tail, running row offset), the pinned output ring the
// kernels of bf_emit.hip write their rows into, and the enqueue / wait / release calls around them.
#include "bf_ctx.h"

namespace {

constexpr int kRecs = 1024;   // slices enqueued and not yet waited for, at most

int bits_for(unsigned long long v) {   // bits needed to hold 0 .. v
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

}  // namespace

struct bf_emit {
    int device = 0;
    unsigned long long cap = 0;             // ring positions of the covered plane
    int rows = 0, cols = 0;
    DevArray<uint8_t> plane;
    DevArray<unsigned long long> tail_t, tail_g;
    DevArray<unsigned long long> d_off;     // running row offset, two words (slice parity)
    DevArray<uint32_t> d_err;
    // scratch for slices of up to t.size() elements (shared by every context: the slices run one after the other on the device)
    DevArray<unsigned long long> t, keys, keys2;
    DevArray<uint32_t> rc, pos;
    DevArray<uint8_t> flag;
    DevArray<uint8_t> temp;                 // the sort's and the scan's temporary storage
    // pinned, device-mapped output ring and per-slice records (first row, rows, error bits, -)
    unsigned long long out_rows = 0;
    MappedArray<uint64_t> out_t;
    MappedArray<uint16_t> out_row, out_col;
    MappedArray<double> out_u, out_v;
    MappedArray<unsigned long long> recs;
    // host bookkeeping, under mu
    std::mutex mu;
    unsigned long long prev_end = 0, prev_first = 0;   // events below prev_end have been in an emitted slice
    long long issued = 0, waited = 0;                   // tickets
    unsigned long long released = 0;                    // rows below this have been consumed
    unsigned long long known_end = 0;                   // exact row offset after the last waited slice
    unsigned long long pending_bound = 0;               // + at most this many rows from enqueued, not yet waited slices
    long long rec_m[kRecs];                             // elements of each slice in flight (its bound)
    Event done[kRecs];                                  // the slice's kernels have finished
    bool have_last = false;
    hipEvent_t last = nullptr;                          // the newest enqueued slice (one of done[], not owned)
};

namespace {

// Scratch for a slice of m elements: an array that holds fewer is replaced by one of k = 1.25 m + 1024 (the slices of a stream
// vary a little), and the temporary storage is sized for k whenever an array was.
int emit_reserve(bf_ctx* c, bf_emit* e, long long m) {
    const size_t k = (size_t)(m + m / 4 + 1024);
    bool fresh = false;
    auto reserve = [&](auto& a) {
        if (a.size() >= (size_t)m) return hipSuccess;
        fresh = true;
        return a.grow(k);
    };
    HIP_TRY(c, reserve(e->t));
    HIP_TRY(c, reserve(e->keys));
    HIP_TRY(c, reserve(e->keys2));
    HIP_TRY(c, reserve(e->rc));
    HIP_TRY(c, reserve(e->pos));
    HIP_TRY(c, reserve(e->flag));
    if (fresh || !e->temp) HIP_TRY(c, e->temp.grow(std::max<size_t>(emit_temp_bytes((long long)k), 1)));
    return BF_OK;
}

int emit_clear(bf_ctx* c, bf_emit* e) {
    const size_t px = (size_t)e->rows * (size_t)e->cols;
    if (e->have_last) HIP_TRY(c, hipEventSynchronize(e->last));
    HIP_TRY(c, hipMemsetAsync(e->plane, 0, (size_t)e->cap, c->stream));
    HIP_TRY(c, hipMemsetAsync(e->tail_g, 0xff, px * 8, c->stream));   // no tail
    HIP_TRY(c, hipMemsetAsync(e->tail_t, 0, px * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(e->d_off, 0, 16, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    e->prev_end = e->prev_first = 0;
    e->issued = e->waited = 0;
    e->released = e->known_end = e->pending_bound = 0;
    e->have_last = false;
    return BF_OK;
}

int create_failed(bf_ctx* c, hipError_t err, const char* what) {
    return fail(c, err == hipErrorOutOfMemory ? BF_ERR_CAPACITY : BF_ERR_HIP, "bf_emit_create: %s: %s", what, hipGetErrorString(err));
}

// bf_emit_slice (held false: the rows' flow is the live slice's, bf_compute_uv's) and bf_global_emit_slice (held true: the held
// flow of the exhaustive search, which must be of these n events); `name`: the entry point's.
int emit_slice(bf_ctx* c, bf_emit* e, const char* name, bool held, int64_t n, uint64_t first, uint64_t start_time, int32_t lead,
               uint64_t lead_t, int32_t lead_row, int32_t lead_col, int64_t* ticket_out) {
    if (!c || !e || !ticket_out) return BF_ERR_ARG;
    *ticket_out = -1;
    GlobalHeldFlow hf;
    if (held) {
        const int hrc = global_held_flow(c, name, &hf);
        if (hrc != BF_OK) return hrc;
        if (hf.n != n) return fail(c, BF_ERR_STATE, "%s: the held flow has %lld events, not %lld", name, hf.n, (long long)n);
    }
    if (c->device != e->device) return fail(c, BF_ERR_ARG, "%s: state on device %d, context on device %d", name, e->device, c->device);
    if (n < 0 || (lead && first == 0)) return fail(c, BF_ERR_ARG, "%s: bad slice (n %lld, first %llu, lead %d)", name, (long long)n,
                                                   (unsigned long long)first, lead);
    const long long m = n + (lead ? 1 : 0);
    std::lock_guard<std::mutex> g(e->mu);
    if ((unsigned long long)m > e->cap)
        return fail(c, BF_ERR_ARG, "%s: %lld elements exceed the ring capacity %llu", name, m, e->cap);
    if (first < e->prev_first)
        return fail(c, BF_ERR_ARG, "%s: slice starts at %llu, before the previous one (%llu)", name, (unsigned long long)first, e->prev_first);
    if (n > 0 && (!c->uploaded || c->n != n))
        return fail(c, BF_ERR_STATE, "%s: the context's slice has %lld events, not %lld", name, c->uploaded ? c->n : 0ll, (long long)n);
    if (lead && (lead_row < 0 || lead_col < 0)) return fail(c, BF_ERR_ARG, "%s: negative lead address", name);
    if (m == 0) return BF_OK;
    // (checked before anything runs: the state is untouched)
    if (e->known_end + e->pending_bound + (unsigned long long)m - e->released > e->out_rows || e->issued - e->waited >= kRecs)
        return fail(c, BF_ERR_CAPACITY, "%s: the output ring (%llu rows) may overflow: release consumed rows first", name, e->out_rows);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = emit_reserve(c, e, m);
    if (rc != BF_OK) return rc;
    EmitSlice a;
    std::memset(&a, 0, sizeof(a));
    const double2* uv = nullptr;
    if (n > 0) {
        if (held) uv = hf.uv;
        else if ((rc = ctx_device_uv(c, &uv)) != BF_OK) return rc;
        const bf_ctx::EvSet& s = c->set[c->cs];
        a.xy = s.xy; a.tloc = s.t; a.perm = c->has_perm ? s.perm : nullptr;
    }
    const long long ticket = e->issued;
    const int slot = (int)(ticket % kRecs);
    a.uv = uv;
    a.n = n; a.lead = lead ? 1 : 0;
    a.first = first; a.cap = e->cap; a.start_time = start_time; a.prev_end = e->prev_end;
    a.last = first + (unsigned long long)n - 1;   // (n == 0: the lead)
    a.lead_t = lead_t; a.lead_row = (uint32_t)lead_row; a.lead_col = (uint32_t)lead_col;
    a.rows = e->rows; a.cols = e->cols;
    a.plane = e->plane; a.tail_t = e->tail_t; a.tail_g = e->tail_g;
    a.t = e->t; a.rc = e->rc; a.flag = e->flag; a.keys = e->keys; a.pos = e->pos;
    a.jbits = bits_for((unsigned long long)m - 1);
    a.kbits = a.jbits + bits_for((unsigned long long)e->rows * (unsigned long long)e->cols - 1);
    a.err = e->d_err;
    a.out_t = (unsigned long long*)e->out_t.get(); a.out_row = e->out_row; a.out_col = e->out_col; a.out_u = e->out_u; a.out_v = e->out_v;
    a.out_rows = e->out_rows;
    a.off_in = e->d_off + (ticket & 1);
    a.off_out = e->d_off + ((ticket + 1) & 1);
    a.rec = e->recs + 4 * slot;
    // after the previous slice, whichever context enqueued it: it wrote the plane, the tail and the offset this one reads
    if (e->have_last) HIP_TRY(c, hipStreamWaitEvent(c->stream, e->last, 0));
    HIP_TRY(c, hipMemsetAsync(e->d_err, 0, 4, c->stream));
    HIP_TRY(c, launch_emit(a, e->keys2, e->temp, e->temp.size(), c->stream));
    HIP_TRY(c, hipEventRecord(e->done[slot], c->stream));
    e->last = e->done[slot];
    e->have_last = true;
    e->rec_m[slot] = m;
    e->pending_bound += (unsigned long long)m;
    e->issued = ticket + 1;
    const unsigned long long end = first + (unsigned long long)n;
    if (end > e->prev_end) e->prev_end = end;
    e->prev_first = first;
    *ticket_out = ticket;
    return BF_OK;
}

}  // namespace

extern "C" {

int bf_emit_create(bf_ctx* c, int64_t ring_cap, int32_t rows, int32_t cols, int64_t out_rows, bf_emit** out) {
    if (!c || !out) return BF_ERR_ARG;
    *out = nullptr;
    if (ring_cap < 1 || rows < 1 || cols < 1 || rows > 65536 || cols > 65536 || (long long)rows * cols > (1ll << 32) || out_rows < 1)
        return fail(c, BF_ERR_ARG, "bf_emit_create: bad ring capacity %lld, sensor %d x %d or output ring %lld", (long long)ring_cap, rows,
                    cols, (long long)out_rows);
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<bf_emit> e(new (std::nothrow) bf_emit);   // (a failure below frees what was made)
    if (!e) return fail(c, BF_ERR_CAPACITY, "bf_emit_create: out of host memory");
    e->device = c->device;
    e->cap = (unsigned long long)ring_cap;
    e->rows = rows;
    e->cols = cols;
    e->out_rows = (unsigned long long)out_rows;
    const size_t px = (size_t)rows * (size_t)cols, R = (size_t)out_rows;
    hipError_t err;
    if ((err = e->plane.grow((size_t)ring_cap)) != hipSuccess) return create_failed(c, err, "covered plane");
    if ((err = e->tail_t.grow(px)) != hipSuccess) return create_failed(c, err, "tail");
    if ((err = e->tail_g.grow(px)) != hipSuccess) return create_failed(c, err, "tail");
    if ((err = e->d_off.grow(2)) != hipSuccess) return create_failed(c, err, "row offset");
    if ((err = e->d_err.grow(1)) != hipSuccess) return create_failed(c, err, "error word");
    // (pinned and mapped: k_emit_rows stores the rows straight into them)
    if ((err = e->out_t.grow(R)) != hipSuccess) return create_failed(c, err, "output ring");
    if ((err = e->out_row.grow(R)) != hipSuccess) return create_failed(c, err, "output ring");
    if ((err = e->out_col.grow(R)) != hipSuccess) return create_failed(c, err, "output ring");
    if ((err = e->out_u.grow(R)) != hipSuccess) return create_failed(c, err, "output ring");
    if ((err = e->out_v.grow(R)) != hipSuccess) return create_failed(c, err, "output ring");
    if ((err = e->recs.grow((size_t)kRecs * 4)) != hipSuccess) return create_failed(c, err, "slice records");
    for (int i = 0; i < kRecs; ++i)
        if ((err = e->done[i].create(hipEventDisableTiming)) != hipSuccess) return create_failed(c, err, "events");
    const int rc = emit_clear(c, e.get());
    if (rc != BF_OK) return rc;
    *out = e.release();
    return BF_OK;
}

int bf_emit_destroy(bf_emit* e) {
    if (!e) return BF_ERR_ARG;
    (void)hipSetDevice(e->device);
    if (e->have_last) (void)hipEventSynchronize(e->last);
    delete e;
    return BF_OK;
}

int bf_emit_reset(bf_ctx* c, bf_emit* e) {
    if (!c || !e) return BF_ERR_ARG;
    if (c->device != e->device) return fail(c, BF_ERR_ARG, "bf_emit_reset: state on device %d, context on device %d", e->device, c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(e->mu);
    return emit_clear(c, e);
}

int bf_emit_output(bf_emit* e, uint64_t** t, uint16_t** row, uint16_t** col, double** u, double** v, int64_t* out_rows) {
    if (!e) return BF_ERR_ARG;
    if (t) *t = e->out_t;
    if (row) *row = e->out_row;
    if (col) *col = e->out_col;
    if (u) *u = e->out_u;
    if (v) *v = e->out_v;
    if (out_rows) *out_rows = (int64_t)e->out_rows;
    return BF_OK;
}

int bf_emit_slice(bf_ctx* c, bf_emit* e, int64_t n, uint64_t first, uint64_t start_time, int32_t lead, uint64_t lead_t,
                  int32_t lead_row, int32_t lead_col, int64_t* ticket_out) {
    return emit_slice(c, e, "bf_emit_slice", false, n, first, start_time, lead, lead_t, lead_row, lead_col, ticket_out);
}

int bf_global_emit_slice(bf_ctx* c, bf_emit* e, int64_t n, uint64_t first, uint64_t start_time, int32_t lead, uint64_t lead_t,
                         int32_t lead_row, int32_t lead_col, int64_t* ticket_out) {
    return emit_slice(c, e, "bf_global_emit_slice", true, n, first, start_time, lead, lead_t, lead_row, lead_col, ticket_out);
}

int bf_emit_wait(bf_ctx* c, bf_emit* e, int64_t ticket, uint64_t* first_row, int64_t* rows) {
    if (!c || !e || !first_row || !rows) return BF_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    if (ticket != e->waited || ticket >= e->issued)
        return fail(c, BF_ERR_ARG, "bf_emit_wait: ticket %lld, the next one to wait for is %lld (%lld issued)", (long long)ticket,
                    (long long)e->waited, (long long)e->issued);
    const int slot = (int)(ticket % kRecs);
    HIP_TRY(c, hipSetDevice(e->device));
    HIP_TRY(c, hipEventSynchronize(e->done[slot]));
    const unsigned long long* r = e->recs + 4 * slot;
    e->waited = ticket + 1;
    e->pending_bound -= (unsigned long long)e->rec_m[slot];
    e->known_end = r[0] + r[1];
    if (r[2]) return fail(c, BF_ERR_ARG, "bf_emit_wait: an event address lies outside the %d x %d sensor (the emit state is undefined now: "
                                         "bf_emit_reset)", e->rows, e->cols);
    *first_row = r[0];
    *rows = (int64_t)r[1];
    return BF_OK;
}

int bf_emit_release(bf_emit* e, uint64_t upto_row) {
    if (!e) return BF_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    if (upto_row > e->known_end || upto_row < e->released) return BF_ERR_ARG;
    e->released = upto_row;
    return BF_OK;
}

}  // extern "C"
