// test_track_match.cpp -- bf::ObjectTracker::match (better_flow/object_tracker.h) on cases read from standard input, for
// tests/test_host_track.py, which holds every answer to the Python restatement (tests/track_ref.py: match).  A pure function of
// its table: no device, no library.  Built with -fsanitize=address,undefined and run directly.
//
// Input, whitespace separated, any number of cases:  K Kp num den, then K * (Kp + 1) table words, then K inside counts.
// Output, one line per case: the K matched kept groups (-1: none).
#include <better_flow/object_tracker.h>

#include <cstdio>
#include <vector>

int main() {
    int K, Kp;
    unsigned long long num, den;
    int cases = 0;
    while (std::scanf("%d %d %llu %llu", &K, &Kp, &num, &den) == 4) {
        if (K < 0 || Kp < 0 || K > 64 || Kp > 64) return 2;
        std::vector<int32_t> table((size_t)K * (size_t)(Kp + 1)), inside((size_t)K);
        for (int32_t &v : table)
            if (std::scanf("%d", &v) != 1) return 2;
        for (int32_t &v : inside)
            if (std::scanf("%d", &v) != 1) return 2;
        const std::vector<int32_t> m = bf::ObjectTracker::match(table, inside, K, Kp, num, den);
        if ((int)m.size() != K) return 3;
        for (int k = 0; k < K; ++k) std::printf("%s%d", k ? " " : "", (int)m[(size_t)k]);
        std::printf("\n");
        ++cases;
    }
    return cases > 0 ? 0 : 2;
}
