// failure_latch.h -- the failure state of a stream engine and its components: the first failure reported wins, and it is
// rethrown on the caller's thread as bf::AccelError.
//
// Several threads report (the farm's workers through deliver(), the device flow table, the frame pipeline) and several
// wait on a condition of their own that a failure must end (the producer in reserve(), a worker waiting for a frame
// slot).  fail() is the one place that writes the code and the text, under the latch's own lock; then it calls the
// waker set with on_failure(), which notifies every such condition variable.  A waiter tests failed() in its predicate
// under ITS lock, and its waker takes that lock once before notifying (wake_waiters) -- so a failure latched between the
// test and the wait is not missed.
#ifndef BF_HOST_FAILURE_LATCH_H
#define BF_HOST_FAILURE_LATCH_H

#include <better_flow/accel_lib.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>

namespace bf {

// Wake the threads waiting on `cv` under `mu` for something that changed WITHOUT `mu` held (a latched failure).
inline void wake_waiters(std::mutex &mu, std::condition_variable &cv) {
    { std::lock_guard<std::mutex> g(mu); }
    cv.notify_all();
}

class FailureLatch {
public:
    // Set before any thread can report.  Called once, by the reporter of the first failure, with no lock of the latch held;
    // reporters hold no lock that it takes.
    void on_failure(std::function<void()> waker) { waker_ = std::move(waker); }

    bool failed() const { return failed_.load(); }   // (lock-free: the producer tests it per reserve())

    void fail(int rc, const std::string &text) {
        {
            std::lock_guard<std::mutex> g(mu_);
            if (failed_) return;
            code_ = rc; text_ = text;
            failed_ = true;
        }
        if (waker_) waker_();
    }

    void rethrow() const {
        if (!failed_) return;
        std::lock_guard<std::mutex> g(mu_);
        throw AccelError(code_, text_);
    }

private:
    mutable std::mutex mu_;       // code_, text_ (written once, before failed_ turns true)
    std::atomic<bool> failed_{false};
    int code_ = 0;
    std::string text_;
    std::function<void()> waker_;   // set before the threads start, constant afterwards
};

}  // namespace bf

#endif  // BF_HOST_FAILURE_LATCH_H
