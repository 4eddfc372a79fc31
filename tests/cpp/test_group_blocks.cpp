// test_group_blocks.cpp -- the result-block layouts of better_flow_amd/csrc/bf_group_blocks.h on the host: for K in {1, 2, 63, 64}
// (the track block: times Kp in {1, 3, 64}) every named word of a block is distinct, a multiple of the block's stride and below
// size(); together the named words are exactly size / stride; they come in the documented order, table after table, then the
// tail; size at K = 64 is the buffer the kernels were always given, as a literal; and a dozen words are pinned to literals worked
// out from the formulas the kernels and the host used before the layouts existed ((2 K + w) * 16 and the like).
// Stand-alone: g++ -fsanitize=address,undefined tests/cpp/test_group_blocks.cpp (driven by tests/test_group_blocks_cpu.py).
#include <cstdio>
#include <vector>

#include "../../better_flow_amd/csrc/bf_group_blocks.h"

using bf::AssignBlock;
using bf::MergeBlock;
using bf::ProjectBlock;
using bf::TrackBlock;

static int failures = 0;
static long long checked = 0;

static void expect_eq(const char* what, long long got, long long want) {
    ++checked;
    if (got == want) return;
    printf("FAILED %s: got %lld, expected %lld\n", what, got, want);
    ++failures;
}

// `words`: the named words in the documented order.  Each is a multiple of the stride and below size; in that order they are
// 0, stride, 2 stride, ...: so they are distinct, ascending table after table, and together exactly size / stride.
static void check_block(const char* what, const std::vector<size_t>& words, size_t stride, size_t size) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: named words == size / stride", what);
    expect_eq(msg, (long long)words.size(), (long long)(size / stride));
    expect_eq(what, (long long)(size % stride), 0);
    std::vector<char> seen(size / stride, 0);
    for (size_t i = 0; i < words.size(); ++i) {
        const size_t w = words[i];
        ++checked;
        if (w % stride != 0 || w >= size) {
            printf("FAILED %s: word %zu at %zu (stride %zu, size %zu)\n", what, i, w, stride, size);
            ++failures;
            continue;
        }
        if (seen[w / stride]++) {
            printf("FAILED %s: word %zu at %zu names a word twice\n", what, i, w);
            ++failures;
        }
        if (w != i * stride) {
            printf("FAILED %s: word %zu at %zu, the documented order puts it at %zu\n", what, i, w, i * stride);
            ++failures;
        }
    }
}

int main() {
    const int Ks[] = {1, 2, 63, 64}, Kps[] = {1, 3, 64};
    char what[96];
    for (int K : Ks) {
        std::vector<size_t> w;
        // assign: count[0 .. K] (the last: unassigned), changed, max_score
        for (int k = 0; k <= K; ++k) w.push_back((size_t)AssignBlock::count(K, k));
        w.push_back((size_t)AssignBlock::changed(K));
        w.push_back((size_t)AssignBlock::max_score(K));
        snprintf(what, sizeof what, "assign K=%d", K);
        check_block(what, w, AssignBlock::kStride, (size_t)AssignBlock::size(K));

        // project: events, inside, pixels_hit, pixels_owned, max, sum_sq; unassigned, pixels, sum, sum_sq_total
        w.clear();
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::events(K, k));
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::inside(K, k));
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::pixels_hit(K, k));
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::pixels_owned(K, k));
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::max(K, k));
        for (int k = 0; k < K; ++k) w.push_back(ProjectBlock::sum_sq(K, k));
        w.push_back(ProjectBlock::unassigned(K));
        w.push_back(ProjectBlock::pixels(K));
        w.push_back(ProjectBlock::sum(K));
        w.push_back(ProjectBlock::sum_sq_total(K));
        snprintf(what, sizeof what, "project K=%d", K);
        check_block(what, w, ProjectBlock::kStride, ProjectBlock::size(K));
        // (the form k_project_compose flushes its three totals through)
        expect_eq("project total 0 is pixels", (long long)ProjectBlock::total(K, 0), (long long)ProjectBlock::pixels(K));
        expect_eq("project total 1 is sum", (long long)ProjectBlock::total(K, 1), (long long)ProjectBlock::sum(K));
        expect_eq("project total 2 is sum_sq_total", (long long)ProjectBlock::total(K, 2), (long long)ProjectBlock::sum_sq_total(K));

        // (the form k_project_vote flushes its compact table through: events[K], unassigned, inside[K])
        for (int i = 0; i < K; ++i) {
            expect_eq("project vote_word: events", (long long)ProjectBlock::vote_word(K, i), (long long)ProjectBlock::events(K, i));
            expect_eq("project vote_word: inside", (long long)ProjectBlock::vote_word(K, K + 1 + i), (long long)ProjectBlock::inside(K, i));
        }
        expect_eq("project vote_word: unassigned", (long long)ProjectBlock::vote_word(K, K), (long long)ProjectBlock::unassigned(K));

        // merge: gain[b][a], inside[b][a]; sum, sum_sq
        w.clear();
        for (int b = 0; b < K; ++b)
            for (int a = 0; a < K; ++a) w.push_back(MergeBlock::gain(K, b, a));
        for (int b = 0; b < K; ++b)
            for (int a = 0; a < K; ++a) w.push_back(MergeBlock::inside(K, b, a));
        w.push_back(MergeBlock::sum(K));
        w.push_back(MergeBlock::sum_sq(K));
        snprintf(what, sizeof what, "merge K=%d", K);
        check_block(what, w, MergeBlock::kStride, MergeBlock::size(K));
        expect_eq("merge total 0 is sum", (long long)MergeBlock::total(K, 0), (long long)MergeBlock::sum(K));
        expect_eq("merge total 1 is sum_sq", (long long)MergeBlock::total(K, 1), (long long)MergeBlock::sum_sq(K));

        // track: overlap[k][0 .. Kp] (the last: a pixel nobody owns); outside, unassigned
        for (int Kp : Kps) {
            w.clear();
            for (int k = 0; k < K; ++k)
                for (int j = 0; j <= Kp; ++j) w.push_back(TrackBlock::overlap(K, Kp, k, j));
            w.push_back(TrackBlock::outside(K, Kp));
            w.push_back(TrackBlock::unassigned(K, Kp));
            snprintf(what, sizeof what, "track K=%d Kp=%d", K, Kp);
            check_block(what, w, TrackBlock::kStride, TrackBlock::size(K, Kp));
            expect_eq("track words", TrackBlock::words(K, Kp), (long long)w.size());
            // (the contiguous form k_track_overlap flushes its table through)
            for (size_t i = 0; i < w.size(); ++i) expect_eq("track word(w)", (long long)TrackBlock::word((int)i), (long long)w[i]);
        }
    }

    // the strides: a 128-byte line per word of the blocks many work-groups add into
    expect_eq("assign stride", AssignBlock::kStride, 1);
    expect_eq("project stride", ProjectBlock::kStride, 16);
    expect_eq("merge stride", MergeBlock::kStride, 16);
    expect_eq("track stride", TrackBlock::kStride, 32);

    // the buffers at K = 64 (Kp = 64), in elements: 64 + 3; (6 * 64 + 4) * 16; (2 * 64^2 + 2) * 16; (64 * 65 + 2) * 32
    expect_eq("assign size(64)", AssignBlock::size(64), 67);
    expect_eq("project size(64)", (long long)ProjectBlock::size(64), 6208);
    expect_eq("merge size(64)", (long long)MergeBlock::size(64), 131104);
    expect_eq("track size(64, 64)", (long long)TrackBlock::size(64, 64), 133184);

    // spot values, from the formulas the kernels and the host used before
    expect_eq("assign changed(K=5) = K + 1", AssignBlock::changed(5), 6);
    expect_eq("assign max_score(K=64) = K + 2", AssignBlock::max_score(64), 66);
    expect_eq("project inside(K=3, k=2) = (K + k) * 16", (long long)ProjectBlock::inside(3, 2), 80);
    expect_eq("project pixels_hit(K=64, k=63) = (2 K + k) * 16", (long long)ProjectBlock::pixels_hit(64, 63), 3056);
    expect_eq("project pixels_owned(K=2, k=0) = 3 K * 16", (long long)ProjectBlock::pixels_owned(2, 0), 96);
    expect_eq("project max(K=63, k=1) = (4 K + 1) * 16", (long long)ProjectBlock::max(63, 1), 4048);
    expect_eq("project sum_sq(K=2, k=1) = (5 * 2 + 1) * 16", (long long)ProjectBlock::sum_sq(2, 1), 176);
    expect_eq("project unassigned(K=64) = 6 K * 16", (long long)ProjectBlock::unassigned(64), 6144);
    expect_eq("project unassigned(K=1) = 6 K * 16", (long long)ProjectBlock::unassigned(1), 96);
    expect_eq("project sum_sq_total(K=2) = (6 K + 3) * 16", (long long)ProjectBlock::sum_sq_total(2), 240);
    expect_eq("merge gain(K=63, b=62, a=61) = (b K + a) * 16", (long long)MergeBlock::gain(63, 62, 61), 63472);
    expect_eq("merge inside(K=2, b=1, a=0) = (K^2 + b K + a) * 16", (long long)MergeBlock::inside(2, 1, 0), 96);
    expect_eq("merge inside(K=64, b=3, a=5) = (K^2 + b K + a) * 16", (long long)MergeBlock::inside(64, 3, 5), 68688);
    expect_eq("merge sum(K=64) = 2 K^2 * 16", (long long)MergeBlock::sum(64), 131072);
    expect_eq("merge sum_sq(K=2) = (2 K^2 + 1) * 16", (long long)MergeBlock::sum_sq(2), 144);
    expect_eq("track overlap(K=2, Kp=3, k=1, j=3) = (k (Kp + 1) + j) * 32", (long long)TrackBlock::overlap(2, 3, 1, 3), 224);
    expect_eq("track outside(K=2, Kp=3) = K (Kp + 1) * 32", (long long)TrackBlock::outside(2, 3), 256);
    expect_eq("track outside(K=63, Kp=1) = K (Kp + 1) * 32", (long long)TrackBlock::outside(63, 1), 4032);
    expect_eq("track unassigned(K=64, Kp=64) = (K (Kp + 1) + 1) * 32", (long long)TrackBlock::unassigned(64, 64), 133152);

    printf("checked: %lld\n", checked);
    printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
