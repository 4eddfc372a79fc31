// bf::FailureLatch (better_flow/failure_latch.h), the seam through which the stream engine, its device flow table and
// its frame pipeline report a failure: two reporters race to fail() while two threads wait the way the engine's
// reserve() and the frame pipeline's render() wait -- each on a condition variable of its own, under a lock of its own,
// with latch.failed() in the predicate.  Checked every round: the first failure wins (code and text of ONE reporter,
// unchanged by a later fail()), rethrow() throws exactly it, the waker ran once, and both waiters came back (a waiter
// that is not woken hangs the program: the caller's time limit).  Needs no device and no C-ABI library.
#include <better_flow/failure_latch.h>

#include <cstdio>
#include <thread>

int main() {
    int bad = 0;
    auto check = [&](bool ok, const char *what, int round) {
        if (!ok) { std::printf("FAIL round %d: %s\n", round, what); ++bad; }
    };
    {   // in sequence: nothing to throw before a failure; the second report changes nothing
        bf::FailureLatch latch;
        bool threw = false;
        try { latch.rethrow(); } catch (...) { threw = true; }
        check(!threw && !latch.failed(), "a fresh latch has not failed", -1);
        latch.fail(-3, "first");
        latch.fail(-4, "second");
        try { latch.rethrow(); } catch (const bf::AccelError &e) { threw = e.code == -3 && std::string(e.what()) == "first"; }
        check(threw && latch.failed(), "the first of two reports is rethrown", -1);
    }
    const int rounds = 300;
    for (int round = 0; round < rounds; ++round) {
        bf::FailureLatch latch;
        std::mutex mu_a, mu_b;
        std::condition_variable cv_a, cv_b;
        bool other_reason = false;   // (what the waiters would otherwise wait for; never comes)
        int wakes = 0;
        latch.on_failure([&] { ++wakes; bf::wake_waiters(mu_a, cv_a); bf::wake_waiters(mu_b, cv_b); });
        std::atomic<int> ready{0};
        std::atomic<bool> go{false};
        auto waiter = [&](std::mutex &mu, std::condition_variable &cv) {
            ++ready;
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return latch.failed() || other_reason; });
        };
        auto reporter = [&](int id) {
            ++ready;
            while (!go) std::this_thread::yield();
            latch.fail(-10 - id, "reporter " + std::to_string(id));
        };
        std::thread w0(waiter, std::ref(mu_a), std::ref(cv_a)), w1(waiter, std::ref(mu_b), std::ref(cv_b)), r0(reporter, 0), r1(reporter, 1);
        while (ready < 4) std::this_thread::yield();
        if (round % 2) std::this_thread::sleep_for(std::chrono::microseconds(200));   // (the waiters usually asleep / usually not yet)
        go = true;
        r0.join(); r1.join(); w0.join(); w1.join();
        check(wakes == 1, "the waker runs once, for the first failure", round);
        int code = 0;
        std::string text;
        try { latch.rethrow(); } catch (const bf::AccelError &e) { code = e.code; text = e.what(); }
        check((code == -10 && text == "reporter 0") || (code == -11 && text == "reporter 1"), "code and text of one reporter", round);
        latch.fail(-99, "late");
        try { latch.rethrow(); } catch (const bf::AccelError &e) { check(e.code == code && text == e.what(), "a later report changes nothing", round); }
        check(wakes == 1, "a later report wakes nobody", round);
    }
    if (!bad) std::printf("OK failure latch: %d rounds, 2 reporters, 2 waiters\n", rounds);
    return bad ? 1 : 0;
}
