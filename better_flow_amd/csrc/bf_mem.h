// bf_mem.h -- owning handles for the HIP resources of the C-ABI's host side (bf_ctx, GlobalSearch, bf_emit): device arrays,
// pinned host arrays, events and streams.  Private to the host files (through bf_ctx.h); no kernel source includes it.
//
// Every handle is move-only, releases what it holds when it dies, and converts to its raw pointer / handle, so that argument
// builders and launchers read as with raw pointers.  The rules, decided here and nowhere else:
//   - grow(n) keeps an array that holds n elements already and replaces it otherwise.  A grow that fails leaves the handle
//     empty (size 0), never holding a freed pointer.
//   - Memory is freed only after the device has been waited for (replaced by grow, or at destruction): queued work of any
//     stream of the current device may still use it.  (hipFree is documented to do the same; nothing here relies on that.)
//     The owners still synchronize their own streams before they let go (bf_destroy, bf_emit_destroy).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bf_mem {

// device memory (hipMalloc) or, Pinned, host memory (hipHostMalloc with Flags)
template <class T, bool Pinned, unsigned Flags = hipHostMallocDefault>
class Array {
  public:
    Array() = default;
    Array(const Array&) = delete;
    Array& operator=(const Array&) = delete;
    Array(Array&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Array& operator=(Array&& o) noexcept {
        if (this != &o) {
            if (p_) (void)hipDeviceSynchronize();
            release();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~Array() {
        if (p_) (void)hipDeviceSynchronize();
        release();
    }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }   // elements held

    // At least n elements.  *fresh (if given): the array was (re)allocated by this call, its content is undefined.
    hipError_t grow(size_t n, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        if (n <= n_) return hipSuccess;
        if (p_) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return e;
            release();
        }
        void* q = nullptr;
        hipError_t e;
        if constexpr (Pinned) e = hipHostMalloc(&q, n * sizeof(T), Flags);
        else e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q);
        n_ = n;
        if (fresh) *fresh = true;
        return hipSuccess;
    }

  private:
    void release() {   // (the device has been waited for)
        if (p_) {
            if constexpr (Pinned) (void)hipHostFree(p_);
            else (void)hipFree(p_);
        }
        p_ = nullptr;
        n_ = 0;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using DevArray = Array<T, false>;
template <class T> using HostArray = Array<T, true>;                          // pinned
template <class T> using MappedArray = Array<T, true, hipHostMallocMapped>;   // pinned, the device reads / writes it in place

class Event {
  public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~Event() { reset(); }

    operator hipEvent_t() const { return e_; }
    // creates the event unless the handle has one
    hipError_t create(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) e_ = e;
        return r;
    }

  private:
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipEvent_t e_ = nullptr;
};

// a stream the handle created (and destroys), or one it borrows from the caller
class Stream {
  public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (own_ && s_) (void)hipStreamDestroy(s_);
    }

    operator hipStream_t() const { return s_; }
    // creates an owned stream unless the handle has one
    hipError_t create(unsigned flags) {
        if (s_) return hipSuccess;
        hipStream_t s = nullptr;
        const hipError_t r = hipStreamCreateWithFlags(&s, flags);
        if (r == hipSuccess) { s_ = s; own_ = true; }
        return r;
    }
    void borrow(hipStream_t s) { s_ = s; own_ = false; }

  private:
    hipStream_t s_ = nullptr;
    bool own_ = false;
};

}  // namespace bf_mem
