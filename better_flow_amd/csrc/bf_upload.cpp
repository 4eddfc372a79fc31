// bf_upload.cpp -- C-ABI: staging a slice on the device (AccelLib::init_gpu, accel_lib.h:71-115), blocking, from device arrays, and
// asynchronously on the copy stream from pinned arrays or from a structure-of-arrays event ring (DVS_flow::recompute hand-off).
// Every asynchronous upload describes its host columns (UploadSlot::Source) and takes the next of the two staging slots in FIFO
// order: RECORDED ("defer_uploads") until issue() enqueues its copies -- ISSUED -- and, on a context alone on the GPU, its staging
// kernels on the copy stream -- EARLY.  bf_commit_upload stages an ISSUED slot on the compute stream, swaps an EARLY one in, and
// returns it to FREE; drop_uploads returns slots whose upload failed or was abandoned.
#include <optional>
#include <utility>

#include "bf_ctx.h"

using UploadSlot = bf_ctx::UploadSlot;

// k_prepare of n int32 events into dst and the statistics record `stats`, on stream st (bracketed as category 3 when profiled)
static void prepare(bf_ctx* c, const int32_t* dx, const int32_t* dy, const int32_t* dt, long long n, bf_ctx::EvSet& dst,
                    SliceStats* stats, hipStream_t st, bool profiled) {
    std::optional<ProfScope> ps;
    if (profiled) ps.emplace(c, 3);
    launch_prepare(dx, dy, dt, dst.xy, dst.t, dst.p, n, pad_events(n), stats, st);
}

// The staging kernels of slot s's upload on stream st: the widening kernel of its format (absolute timestamps -> slice-local
// 32-bit times, Event::set_local_time; 16-bit addresses -> the slot's int32 columns, same pass; the widening is never
// profiled), then k_prepare into dst and `stats`.
static int stage(bf_ctx* c, UploadSlot& s, hipStream_t st, bf_ctx::EvSet& dst, SliceStats* stats, bool profiled) {
    const UploadSlot::Source& u = s.src;
    if (u.fmt == UploadSlot::TS64)
        launch_local_time(s.ts, u.t0, s.t, u.n, st);
    else if (u.fmt != UploadSlot::LOCAL32)
        launch_local_time16(s.ts, u.fmt == UploadSlot::ADDR16_TS32, s.in16, s.in16 + c->cap_events, u.t0, s.x, s.y, s.t, u.n, st);
    prepare(c, s.x, s.y, s.t, u.n, dst, stats, st, profiled);
    HIP_TRY(c, hipGetLastError());
    return BF_OK;
}

// The slice of n events is staged (or being staged) in set[0]; its statistics are in `stats` once `ev` has completed (null: the
// compute stream).
static int slice_staged(bf_ctx* c, long long n, const SliceStats* stats, hipEvent_t ev) {
    c->n = n;
    c->n_pad = pad_events(n);
    c->stats_src = stats;
    c->stats_event = ev;
    c->slice_uploaded();
    return BF_OK;
}

// Early staging of slot s (no noise ring, a context alone on the GPU): stage() on the COPY stream, behind the copies, into the
// slot's own event arrays and pinned statistics record.  The arrays may have been swapped out of set[0] at an earlier commit:
// the compute stream must be past that commit first (inc_free).
static int stage_early(bf_ctx* c, UploadSlot& s) {
    // (the committed slice's statistics may still sit, unread, in this slot's record -- a caller that uploads two slices ahead
    // before bf_set_cloud: read them before k_prepare overwrites the record)
    int rc = fold_stats(c, s.stats);
    if (rc != BF_OK) return rc;
    if (s.inc_free_valid) HIP_TRY(c, hipStreamWaitEvent(c->up.stream, s.inc_free, 0));
    rc = stage(c, s, c->up.stream, s.inc, s.stats, false);
    if (rc != BF_OK) return rc;
    HIP_TRY(c, hipEventRecord(s.prepared, c->up.stream));
    s.state = UploadSlot::EARLY;
    return BF_OK;
}

// The HIP side of slot s's upload: its copies on the copy stream, behind the staging kernels that last read the slot, up to two
// contiguous pieces per column (no repacking on the host); then its early staging, unless the slice has a noise ring (that goes
// through d_noise, which the running slice may still read: staged at the commit) or the context is co-scheduled (kernels on the
// copy stream need a hardware queue of their own, and the runtime gives a process four -- with four "co_schedule"d chains in
// flight, eight kernel-carrying streams shared them and the warm regime fell from 5.3 to 3.2 Gevents/s).
static int issue(bf_ctx* c, UploadSlot& s) {
    const UploadSlot::Source& u = s.src;
    const size_t ne = (size_t)c->cap_events;
    const bool addr16 = u.fmt == UploadSlot::ADDR16_TS64 || u.fmt == UploadSlot::ADDR16_TS32;
    if (s.staged_valid) HIP_TRY(c, hipStreamWaitEvent(c->up.stream, s.staged, 0));
    if (u.fmt != UploadSlot::LOCAL32) HIP_TRY(c, s.ts.grow(ne));
    if (addr16) HIP_TRY(c, s.in16.grow(2 * ne));
    if (u.noise) HIP_TRY(c, s.noise.grow(ne));
    const size_t ab = addr16 ? 2 : 4, tb = (u.fmt == UploadSlot::TS64 || u.fmt == UploadSlot::ADDR16_TS64) ? 8 : 4;
    const struct { void* dev; const void* host; size_t bytes; } cols[4] = {   // (per event)
        {addr16 ? (void*)s.in16.get() : (void*)s.x.get(), u.x, ab},
        {addr16 ? (void*)(s.in16 + ne) : (void*)s.y.get(), u.y, ab},
        {u.fmt == UploadSlot::LOCAL32 ? (void*)s.t.get() : (void*)s.ts.get(), u.ts, tb},
        {s.noise.get(), u.noise, 1}};
    const long long n0 = (u.first + u.n <= u.cap) ? u.n : u.cap - u.first, n1 = u.n - n0;   // [first, first + n0) then [0, n1)
    for (const auto& k : cols) {
        if (!k.host) continue;
        char* dev = static_cast<char*>(k.dev);
        const char* host = static_cast<const char*>(k.host);
        HIP_TRY(c, hipMemcpyAsync(dev, host + u.first * k.bytes, n0 * k.bytes, hipMemcpyHostToDevice, c->up.stream));
        if (n1 > 0) HIP_TRY(c, hipMemcpyAsync(dev + n0 * k.bytes, host, n1 * k.bytes, hipMemcpyHostToDevice, c->up.stream));
    }
    HIP_TRY(c, hipEventRecord(s.copy_done, c->up.stream));
    s.state = UploadSlot::ISSUED;
    return (u.noise || c->opt_co_schedule) ? BF_OK : stage_early(c, s);
}

// Every asynchronous upload: the checks, the next slot, and its HIP calls now -- or, "defer_uploads", only its description,
// issued by issue_deferred_uploads.  An upload whose HIP calls fail gives its slot back.
static int upload_async(bf_ctx* c, const UploadSlot::Source& u) {
    if (!c) return BF_ERR_ARG;
    if (u.n <= 0 || u.cap <= 0 || u.first < 0 || u.first >= u.cap || u.n > u.cap || !u.x || !u.y || !u.ts)
        return u.fmt == UploadSlot::LOCAL32 ? fail(c, BF_ERR_ARG, "bad event arrays")
                                            : fail(c, BF_ERR_ARG, "bad ring slice (cap %lld, first %lld, n %lld)", u.cap, u.first, u.n);
    if (u.n > c->cap_events) return fail(c, BF_ERR_CAPACITY, "n=%lld exceeds capacity %lld", u.n, c->cap_events);
    if (c->up.count >= 2) return fail(c, BF_ERR_STATE, "two uploads are already pending");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = streaming_setup(c);
    if (rc != BF_OK) return rc;
    const int k = c->up.count++;
    UploadSlot& s = c->up.at(k);
    s.src = u;
    s.state = UploadSlot::RECORDED;
    if (c->opt_defer_uploads) return BF_OK;
    rc = issue(c, s);
    if (rc != BF_OK) drop_uploads(c, k);
    return rc;
}

int streaming_setup(bf_ctx* c) {
    const size_t ne = (size_t)c->cap_events;
    HIP_TRY(c, c->up.stream.create(hipStreamNonBlocking));
    for (UploadSlot& s : c->up.slot) {
        for (Event* e : {&s.copy_done, &s.staged, &s.prepared, &s.inc_free}) HIP_TRY(c, e->create(hipEventDisableTiming));
        for (DevArray<int32_t>* a : {&s.x, &s.y, &s.t}) HIP_TRY(c, a->grow(ne));
        HIP_TRY(c, s.inc.xy.grow(ne));
        HIP_TRY(c, s.inc.t.grow(ne));
        HIP_TRY(c, s.inc.p.grow(ne));
        HIP_TRY(c, s.stats.grow(kPrepBlocks));
    }
    return BF_OK;
}

int issue_deferred_uploads(bf_ctx* c) {
    for (int k = 0; k < c->up.count; ++k) {
        UploadSlot& s = c->up.at(k);
        if (s.state != UploadSlot::RECORDED) continue;
        const int rc = issue(c, s);
        if (rc != BF_OK) {   // (the uploads ahead of it stay pending and committable)
            drop_uploads(c, k);
            return rc;
        }
    }
    return BF_OK;
}

void drop_uploads(bf_ctx* c, int k) {
    for (int j = k; j < c->up.count; ++j) c->up.at(j).state = UploadSlot::FREE;
    c->up.count = k;
}

extern "C" {

// ---- slice set-up ---------------------------------------------------------------------

static int stage_common(bf_ctx* c, const int32_t* dx, const int32_t* dy, const int32_t* dt, long long n) {
    prepare(c, dx, dy, dt, n, c->set[0], c->d_stats, c->stream, true);
    HIP_TRY(c, hipGetLastError());
    return slice_staged(c, n, c->h_stats, nullptr);
}

int bf_upload_events(bf_ctx* c, const int32_t* fr_x, const int32_t* fr_y, const int32_t* t_ns,
                     const uint8_t* noise, int64_t n) {
    if (!c) return BF_ERR_ARG;
    if (n < 0 || (n > 0 && (!fr_x || !fr_y || !t_ns))) return fail(c, BF_ERR_ARG, "bad event arrays");
    if (n > c->cap_events) return fail(c, BF_ERR_CAPACITY, "n=%lld exceeds capacity %lld", (long long)n, c->cap_events);
    if (c->up.count > 0)   // (the blocking upload stages through slot 0, which a pending asynchronous upload may own)
        return fail(c, BF_ERR_STATE, "bf_upload_events while %d asynchronous upload(s) are pending", c->up.count);
    HIP_TRY(c, hipSetDevice(c->device));
    UploadSlot& s = c->up.slot[0];
    if (s.staged_valid) HIP_TRY(c, hipStreamWaitEvent(c->stream, s.staged, 0));
    const size_t nb = (size_t)n * sizeof(int32_t);
    if (n > 0) {
        HIP_TRY(c, hipMemcpyAsync(s.x, fr_x, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(s.y, fr_y, nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(s.t, t_ns, nb, hipMemcpyHostToDevice, c->stream));
    }
    c->has_noise = false;
    if (noise && n > 0) {
        HIP_TRY(c, hipMemsetAsync(c->d_noise, 0, (size_t)pad_events(n), c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_noise, noise, (size_t)n, hipMemcpyHostToDevice, c->stream));
        c->has_noise = true;
    }
    int rc = stage_common(c, s.x, s.y, s.t, n);
    if (rc != BF_OK) return rc;
    // host arrays are only borrowed for the duration of the call
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BF_OK;
}

int bf_host_alloc(bf_ctx* c, int64_t bytes, void** out) {
    if (!c || !out || bytes <= 0) return BF_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable));   // (portable: a slice farm uploads from one ring to several devices)
    return BF_OK;
}

int bf_host_free(bf_ctx* c, void* ptr) {
    if (!c) return BF_ERR_ARG;
    if (ptr) HIP_TRY(c, hipHostFree(ptr));
    return BF_OK;
}

int bf_upload_events_async(bf_ctx* c, const int32_t* fr_x, const int32_t* fr_y, const int32_t* t_ns, int64_t n) {
    return upload_async(c, {fr_x, fr_y, t_ns, nullptr, n, 0, n, 0, UploadSlot::LOCAL32});
}

int bf_upload_ring_async(bf_ctx* c, const int32_t* ring_x, const int32_t* ring_y, const uint64_t* ring_ts, const uint8_t* ring_noise,
                         int64_t cap, int64_t first, int64_t n, uint64_t t0) {
    return upload_async(c, {ring_x, ring_y, ring_ts, ring_noise, cap, first, n, t0, UploadSlot::TS64});
}

int bf_upload_ring16_async(bf_ctx* c, const uint16_t* ring_row, const uint16_t* ring_col, const uint64_t* ring_ts,
                           const uint8_t* ring_noise, int64_t cap, int64_t first, int64_t n, uint64_t t0) {
    return upload_async(c, {ring_row, ring_col, ring_ts, ring_noise, cap, first, n, t0, UploadSlot::ADDR16_TS64});
}

int bf_upload_ring16t32_async(bf_ctx* c, const uint16_t* ring_row, const uint16_t* ring_col, const uint32_t* ring_t32,
                              const uint8_t* ring_noise, int64_t cap, int64_t first, int64_t n, uint64_t t0) {
    return upload_async(c, {ring_row, ring_col, ring_t32, ring_noise, cap, first, n, t0, UploadSlot::ADDR16_TS32});
}

int bf_upload_events16_async(bf_ctx* c, const uint16_t* fr_x, const uint16_t* fr_y, const int32_t* t_ns, int64_t n) {
    // (slice-local times are their own low 32 bits relative to t0 = 0)
    return upload_async(c, {fr_x, fr_y, t_ns, nullptr, n, 0, n, 0, UploadSlot::ADDR16_TS32});
}

int bf_wait_uploads(bf_ctx* c) {
    if (!c) return BF_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    {
        const int rc = issue_deferred_uploads(c);
        if (rc != BF_OK) return rc;
    }
    if (c->up.stream) HIP_TRY(c, hipStreamSynchronize(c->up.stream));
    return BF_OK;
}

int bf_commit_upload(bf_ctx* c) {
    if (!c) return BF_ERR_ARG;
    if (c->up.count == 0) return fail(c, BF_ERR_STATE, "no upload is pending");
    HIP_TRY(c, hipSetDevice(c->device));
    {   // ("defer_uploads": whatever is still only recorded goes out now, oldest first)
        const int rc = issue_deferred_uploads(c);
        if (rc != BF_OK) return rc;
    }
    UploadSlot& s = c->up.at(0);
    const long long n = s.src.n;
    c->has_noise = false;
    int rc;
    if (s.state == UploadSlot::EARLY) {
        // Staged already (copy stream): the compute stream waits for that, set[0] takes the slot's arrays -- a pointer swap; the
        // arrays that leave set[0] may still be in use by what the compute stream holds (the previous slice's last kernels), so
        // the next staging into them waits for this point of the compute stream -- and the statistics are the slot's record.
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s.prepared, 0));
        std::swap(c->set[0].xy, s.inc.xy);
        std::swap(c->set[0].t, s.inc.t);
        std::swap(c->set[0].p, s.inc.p);
        HIP_TRY(c, hipEventRecord(s.inc_free, c->stream));
        s.inc_free_valid = true;
        s.staged_valid = false;   // (the copy stream itself orders the slot's next copies behind its staging kernels)
        rc = slice_staged(c, n, s.stats, s.prepared);
        // the statistics are usually there already (the staging ran under the previous slice's solve): read them now, so that
        // the slot's record is free for the next upload whoever issues it, and bf_set_cloud has nothing to wait for
        if (rc == BF_OK && hipEventQuery(s.prepared) == hipSuccess) rc = fold_stats(c);
    } else {
        // the staging kernels (compute stream) wait for the copies; nothing blocks on the host
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s.copy_done, 0));
        if (s.src.noise) {   // Event::noise of the slice (padding: not noise, like the blocking upload's)
            HIP_TRY(c, hipMemsetAsync(c->d_noise, 0, (size_t)pad_events(n), c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->d_noise, s.noise, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            c->has_noise = true;
        }
        rc = stage(c, s, c->stream, c->set[0], c->d_stats, true);
        if (rc == BF_OK) rc = slice_staged(c, n, c->h_stats, nullptr);
        // the slot may be refilled once the staging kernels above have read it
        HIP_TRY(c, hipEventRecord(s.staged, c->stream));
        s.staged_valid = true;
    }
    s.state = UploadSlot::FREE;
    c->up.head++;
    c->up.count--;
    return rc;
}

int bf_upload_events_device(bf_ctx* c, const int32_t* d_fr_x, const int32_t* d_fr_y, const int32_t* d_t_ns,
                            int64_t n) {
    if (!c) return BF_ERR_ARG;
    if (n < 0 || (n > 0 && (!d_fr_x || !d_fr_y || !d_t_ns))) return fail(c, BF_ERR_ARG, "bad event arrays");
    if (n > c->cap_events) return fail(c, BF_ERR_CAPACITY, "n=%lld exceeds capacity %lld", (long long)n, c->cap_events);
    HIP_TRY(c, hipSetDevice(c->device));
    c->has_noise = false;
    return stage_common(c, d_fr_x, d_fr_y, d_t_ns, n);
}

}  // extern "C"
