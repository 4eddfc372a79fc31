// event_ring.h -- the stream engine's event ring: the reference's CircularArray of Event records (datastructures.h:6-115)
// as a structure of arrays in PINNED memory, handed to the device without a copy on the host.
//
// Three parallel arrays (u64 timestamp, u16 row, u16 column: 12 bytes per event, the column layout of the binary event
// file), an Event::noise ring used lazily, and -- if per-event flow is wanted -- a ring of (u, v) pairs.  Event number g
// (its arrival number) lives in slot g % cap; a stretch [g, g + n) of at most cap events is one or two contiguous pieces
// of every array, which is what a DMA (bf_upload_ring16_async), a memcpy and a producer writing in place all want.
// The ring knows nothing of triggers, slices or threads: who may touch which slots when is the engine's business
// (stream_flow.h).
#ifndef BF_HOST_EVENT_RING_H
#define BF_HOST_EVENT_RING_H

#include <better_flow/accel_lib.h>
#include <better_flow/common.h>

#include <cstring>
#include <utility>

namespace bf {

// The one or two contiguous stretches of a ring of `cap` slots that hold elements [g, g + n), n <= cap: p[0] from
// slot g % cap, p[1] (possibly empty) from slot 0.
struct RingPieces {
    struct Piece { size_t at, n; } p[2];
};
inline RingPieces ring_pieces(uint64_t g, size_t n, size_t cap) {
    const size_t slot = (size_t)(g % cap), n0 = n < cap - slot ? n : cap - slot;
    return RingPieces{{{slot, n0}, {0, n - n0}}};
}
// ring -> linear / linear -> ring / one byte value over the stretch; `per`: array elements per ring element
template <class T> inline void ring_copy_out(T *dst, const T *ring, const RingPieces &w, size_t per = 1) {
    std::memcpy(dst, ring + per * w.p[0].at, per * w.p[0].n * sizeof(T));
    std::memcpy(dst + per * w.p[0].n, ring, per * w.p[1].n * sizeof(T));
}
template <class T> inline void ring_copy_in(T *ring, const T *src, const RingPieces &w, size_t per = 1) {
    std::memcpy(ring + per * w.p[0].at, src, per * w.p[0].n * sizeof(T));
    std::memcpy(ring, src + per * w.p[0].n, per * w.p[1].n * sizeof(T));
}
inline void ring_fill(uint8_t *ring, const RingPieces &w, int value) {
    std::memset(ring + w.p[0].at, value, w.p[0].n);
    std::memset(ring, value, w.p[1].n);
}

// One pinned host array (bf_host_alloc), freed with the object.  The context is only the library's handle for the call:
// pinned host memory is not tied to it, but it must still be alive when the array goes.
template <class T> class PinnedArray {
public:
    PinnedArray() {}
    PinnedArray(bf_ctx *ctx, size_t n, bool zeroed) : ctx_(ctx) {
        void *p = nullptr;
        const int rc = bf_host_alloc(ctx, (int64_t)(n * sizeof(T)), &p);
        if (rc < 0) throw AccelError(rc, std::string("StreamEngine: pinned allocation failed: ") + bf_last_error(ctx));
        p_ = (T *)p;
        if (zeroed) std::memset(p_, 0, n * sizeof(T));
    }
    ~PinnedArray() { if (p_) (void)bf_host_free(ctx_, p_); }
    PinnedArray(PinnedArray &&o) noexcept : ctx_(o.ctx_), p_(o.p_) { o.p_ = nullptr; }
    PinnedArray &operator=(PinnedArray &&o) noexcept { std::swap(ctx_, o.ctx_); std::swap(p_, o.p_); return *this; }
    operator T *() const { return p_; }

private:
    bf_ctx *ctx_ = nullptr;
    T *p_ = nullptr;
};

// Move-only; an empty ring (cap == 0) until built.  No lock: see the engine for which thread owns which slots.
struct EventRing {
    size_t cap = 0;               // MAX_SZ + lookahead
    PinnedArray<uint64_t> ts;     // ABSOLUTE timestamps (logical time + the engine's time base)
    PinnedArray<uint16_t> row, col;
    PinnedArray<uint8_t> noise;   // Event::noise, all zero until a slice is flagged
    PinnedArray<double> uv;       // (best_u, best_v) pairs, or null

    EventRing() {}
    EventRing(bf_ctx *ctx, size_t cap_, bool with_flow)
        : cap(cap_), ts(ctx, cap_, false), row(ctx, cap_, false), col(ctx, cap_, false), noise(ctx, cap_, true) {
        if (with_flow) uv = PinnedArray<double>(ctx, 2 * cap_, true);
    }

    size_t slot(uint64_t g) const { return (size_t)(g % cap); }
    ull logical(uint64_t g, ull time_base) const { return ts[slot(g)] - time_base; }
    RingPieces pieces(uint64_t g, size_t n) const { return ring_pieces(g, n, cap); }
};

}  // namespace bf

#endif  // BF_HOST_EVENT_RING_H
