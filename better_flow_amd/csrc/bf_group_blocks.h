// bf_group_blocks.h -- the result blocks of the entries on the K models' vote planes, as layouts: where each named word of a
// block sits, as a pure function of plain numbers -- no bf_ctx, no HIP, nothing but <cstdint> and <cstddef>.  The kernels that
// add into a block (bf_assign.hip, bf_project.hip, bf_merge.hip, bf_track.hip) and the host code that reads it back
// (bf_assign_abi.cpp, bf_track_abi.cpp) ask the same functions, so the two cannot disagree; tests/cpp/test_group_blocks.cpp
// holds the layouts to the documented word order and to literal sizes on the host.
//
// A block is a run of words, table after table, then the tail.  Every function returns an ELEMENT index with the block's
// stride applied: the blocks of 64-bit and of 32-bit words that many work-groups add into keep every word on a 128-byte line of
// its own (stride 16 and 32), because atomics on words of one line queue behind each other.  size(): the
// block's elements; words(): its words, size / stride; word(w): the w-th word in the documented order, for a kernel that flushes
// a compact table of its own in one loop.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BF_BLOCK_FN __host__ __device__ constexpr
#else
#define BF_BLOCK_FN constexpr
#endif

namespace bf {

// bf_assign_groups: 32-bit words, unstrided (one flush per work-group, few words), so plain ints.  count[K + 1] (the last:
// unassigned), then changed, then max_score.
struct AssignBlock {
    static constexpr int kStride = 1;
    static BF_BLOCK_FN int count(int /*K*/, int k) { return k; }   // k = 0 .. K; K: unassigned
    static BF_BLOCK_FN int changed(int K) { return K + 1; }
    static BF_BLOCK_FN int max_score(int K) { return K + 2; }
    static BF_BLOCK_FN int size(int K) { return K + 3; }
};

// bf_project_groups (and the base pass of bf_merge_scores and bf_track_keep): 64-bit words.  Six tables of K -- events, inside,
// pixels_hit, pixels_owned, max, sum_sq -- then unassigned, pixels, sum, sum_sq_total.
struct ProjectBlock {
    static constexpr int kStride = 16, kTables = 6, kTail = 4;
    static BF_BLOCK_FN size_t table(int K, int t, int k) { return (size_t)(t * K + k) * kStride; }
    static BF_BLOCK_FN size_t events(int K, int k) { return table(K, 0, k); }
    static BF_BLOCK_FN size_t inside(int K, int k) { return table(K, 1, k); }
    static BF_BLOCK_FN size_t pixels_hit(int K, int k) { return table(K, 2, k); }
    static BF_BLOCK_FN size_t pixels_owned(int K, int k) { return table(K, 3, k); }
    static BF_BLOCK_FN size_t max(int K, int k) { return table(K, 4, k); }
    static BF_BLOCK_FN size_t sum_sq(int K, int k) { return table(K, 5, k); }
    static BF_BLOCK_FN size_t unassigned(int K) { return (size_t)(kTables * K) * kStride; }
    // the three totals of the image, in the tail's order: i = 0 pixels, 1 sum, 2 sum_sq_total
    static BF_BLOCK_FN size_t total(int K, unsigned i) { return (size_t)(kTables * K + 1 + i) * kStride; }
    static BF_BLOCK_FN size_t pixels(int K) { return total(K, 0); }
    static BF_BLOCK_FN size_t sum(int K) { return total(K, 1); }
    static BF_BLOCK_FN size_t sum_sq_total(int K) { return total(K, 2); }
    static BF_BLOCK_FN size_t size(int K) { return (size_t)(kTables * K + kTail) * kStride; }
    // word w of k_project_vote's compact table -- events[K], unassigned, inside[K] -- for its one flush loop: events(K, w),
    // unassigned(K) or inside(K, w - K - 1), selected as a word number so that the kernel multiplies once
    static BF_BLOCK_FN size_t vote_word(int K, int w) {
        return (size_t)(w < K ? w : (w == K ? kTables * K : K + (w - K - 1))) * kStride;
    }
};

// bf_merge_scores: 64-bit words.  gain[K x K] (word b * K + a: the events of group b under model a), inside[K x K], then sum,
// sum_sq.
struct MergeBlock {
    static constexpr int kStride = 16, kTail = 2;
    static BF_BLOCK_FN size_t gain(int K, int b, int a) { return (size_t)(b * K + a) * kStride; }
    static BF_BLOCK_FN size_t inside(int K, int b, int a) { return (size_t)(K * K + b * K + a) * kStride; }
    // the two totals of the image, in the tail's order: i = 0 sum, 1 sum_sq
    static BF_BLOCK_FN size_t total(int K, unsigned i) { return (size_t)(2 * K * K + i) * kStride; }
    static BF_BLOCK_FN size_t sum(int K) { return total(K, 0); }
    static BF_BLOCK_FN size_t sum_sq(int K) { return total(K, 1); }
    static BF_BLOCK_FN size_t size(int K) { return (size_t)(2 * K * K + kTail) * kStride; }
};

// bf_track_overlap: 32-bit words.  overlap[K x (Kp + 1)] (word k * (Kp + 1) + j; j == Kp: a pixel nobody owns), then outside,
// then unassigned.
struct TrackBlock {
    static constexpr int kStride = 32, kTail = 2;
    static BF_BLOCK_FN size_t word(int w) { return (size_t)w * kStride; }
    static BF_BLOCK_FN int words(int K, int Kp) { return K * (Kp + 1) + kTail; }
    static BF_BLOCK_FN size_t overlap(int /*K*/, int Kp, int k, int j) { return word(k * (Kp + 1) + j); }
    static BF_BLOCK_FN size_t outside(int K, int Kp) { return word(K * (Kp + 1)); }
    static BF_BLOCK_FN size_t unassigned(int K, int Kp) { return word(K * (Kp + 1) + 1); }
    static BF_BLOCK_FN size_t size(int K, int Kp) { return (size_t)words(K, Kp) * kStride; }
};

}  // namespace bf
