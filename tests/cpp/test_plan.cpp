// Host-only sweep of the rules that pick the kernel variants of the two-kernel tile-binned loop (better_flow_amd/csrc/bf_plan_rules.h:
// no HIP, no context).  With the MI355X's 256 CUs, over scales 1 .. 9, sensors from 24 x 24 to 1920 x 1200, 1 .. 4M events, both
// homes of the update, the three scatter formats and the margins the tests use, it
//   * asserts that every (head, threads, events per thread, format) tuple the rules return is a compiled instantiation of the
//     scatter kernel (bf_rules::scatter_compiled: what launch_bin_warp_scatter dispatches, everything else is hipErrorInvalidValue),
//   * asserts the converse -- no instantiation is compiled that the rules never ask for,
//   * prints the reachable set, and, given the committed table (tests/variants_reachable.txt), asserts that it equals it.
// usage: test_plan [table]            the sweep
//        test_plan rows < lines       one "H W scale n head fmt margin" per line -> the variants that slice lands on
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "../../better_flow_amd/csrc/bf_plan_rules.h"

using namespace bf_rules;
typedef std::tuple<int, int, int, int> Variant;   // head, threads, events per thread, format

static const int kCus = 256;

static int rows_mode() {
    int H, W, scale, head, fmt, margin;
    long long n;
    while (scanf("%d %d %d %lld %d %d %d", &H, &W, &scale, &n, &head, &fmt, &margin) == 7) {
        const int R = scale * H, C = scale * W;
        const BinShape g = bin_shape(n, R, C, kCus, bin_margin(margin));
        const ScatterSize k1 = scatter_size(fmt, head != 0, g.nbins, n, kCus);
        const bool ok = bin_grid_ok(g, R) && bin_format_ok(g, fmt);
        printf("ok %d k1 %d %d %d %d k3 %d %d %d grid %d %d %d %d\n", ok ? 1 : 0, head ? 1 : 0, k1.threads, k1.per_thread, fmt,
               stencil_half_scale(scale), stencil_mode(fmt), stencil_capped(stencil_tiles(R, C), kCus) ? 1 : 0, g.TSR, g.TS, g.D,
               g.nbins);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "rows")) return rows_mode();
    const int scales[] = {1, 3, 5, 7, 9};
    const int margins[] = {0, 1, 2, 3, 4};   // 0: the constant kBinMargin; the others: "debug_margin" of the GPU tests
    const int formats[] = {0, 2, 3};
    // the sensors of the suite and of BASELINE.json, then a regular grid up to 1920 x 1200
    std::vector<std::pair<int, int>> sensors = {{24, 24},   {65, 67},   {90, 120},  {97, 130},  {129, 193}, {180, 240}, {181, 243},
                                                {260, 346}, {300, 400}, {420, 560}, {480, 440}, {480, 520}, {480, 560}, {480, 640},
                                                {600, 800}, {720, 1280}, {768, 1024}, {1080, 1920}, {1200, 1920}};
    for (int H = 24; H <= 1200; H += 56)
        for (int W = 24; W <= 1920; W += 79) sensors.push_back({H, W});
    std::vector<long long> counts;
    for (double x = 1.0; x < 4.0e6; x *= 1.09) {
        const long long n = (long long)std::floor(x);
        if (counts.empty() || counts.back() != n) counts.push_back(n);
    }
    counts.push_back(4000000);

    std::set<Variant> reached;
    long long slices = 0, failures = 0;
    for (const auto& hw : sensors)
        for (int scale : scales)
            for (int margin : margins)
                for (long long n : counts) {
                    const int R = scale * hw.first, C = scale * hw.second;
                    const BinShape g = bin_shape(n, R, C, kCus, bin_margin(margin));
                    if (g.D > g.TS / 2 || g.D > g.TSR / 2 || g.nbins != g.nbr * g.nbc || g.nbins < 1) {
                        if (failures++ < 20) printf("FAIL bad grid: %d x %d, n %lld, margin %d\n", R, C, n, margin);
                        continue;
                    }
                    if (!bin_grid_ok(g, R)) continue;   // (the slice takes the global-atomics loop)
                    ++slices;
                    for (int fmt : formats) {
                        if (!bin_format_ok(g, fmt)) continue;
                        for (int head = 0; head < 2; ++head) {
                            const ScatterSize k1 = scatter_size(fmt, head != 0, g.nbins, n, kCus);
                            if (!scatter_compiled(head != 0, k1.threads, k1.per_thread, fmt)) {
                                if (failures++ < 20)
                                    printf("FAIL no kernel for head %d threads %d events/thread %d format %d (%d x %d, n %lld, margin %d)\n",
                                           head, k1.threads, k1.per_thread, fmt, R, C, n, margin);
                                continue;
                            }
                            reached.insert(Variant(head, k1.threads, k1.per_thread, fmt));
                        }
                    }
                }
    // the converse: whatever is compiled is reachable
    const int sizes[] = {64, 128, 256, 512, 1024}, per_thread[] = {1, 2, 3, 4, 6, 8, 10, 12, 16};
    int compiled = 0;
    for (int head = 0; head < 2; ++head)
        for (int threads : sizes)
            for (int u : per_thread)
                for (int fmt = 0; fmt <= 3; ++fmt) {
                    if (!scatter_compiled(head != 0, threads, u, fmt)) continue;
                    ++compiled;
                    if (!reached.count(Variant(head, threads, u, fmt))) {
                        ++failures;
                        printf("FAIL compiled but never requested: head %d threads %d events/thread %d format %d\n", head, threads, u, fmt);
                    }
                }
    printf("# %lld binned slices swept; %zu reachable scatter variants, %d compiled (x warp / no warp: %d kernels)\n", slices,
           reached.size(), compiled, 2 * compiled);
    printf("# head threads events_per_thread format\n");
    for (const Variant& v : reached) printf("%d %d %d %d\n", std::get<0>(v), std::get<1>(v), std::get<2>(v), std::get<3>(v));

    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { printf("FAIL cannot read %s\n", argv[1]); return 1; }
        std::set<Variant> table;
        char line[256];
        while (fgets(line, sizeof(line), f)) {
            int a, b, c, d;
            if (line[0] == '#' || sscanf(line, "%d %d %d %d", &a, &b, &c, &d) != 4) continue;
            table.insert(Variant(a, b, c, d));
        }
        fclose(f);
        for (const Variant& v : reached)
            if (!table.count(v)) {
                ++failures;
                printf("FAIL reachable but not in the table: %d %d %d %d\n", std::get<0>(v), std::get<1>(v), std::get<2>(v), std::get<3>(v));
            }
        for (const Variant& v : table)
            if (!reached.count(v)) {
                ++failures;
                printf("FAIL in the table but not reachable: %d %d %d %d\n", std::get<0>(v), std::get<1>(v), std::get<2>(v), std::get<3>(v));
            }
    }
    // the capped stencil build: at 8 tiles of 16 x 64 per CU
    if (stencil_capped(8 * kCus - 1, kCus) || !stencil_capped(8 * kCus, kCus) || stencil_capped(1 << 20, 0) ||
        stencil_tiles(16, 64) != 1 || stencil_tiles(17, 65) != 4) {
        ++failures;
        printf("FAIL stencil_capped / stencil_tiles\n");
    }
    if (failures) { printf("%lld failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
