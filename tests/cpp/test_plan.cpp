// Host-only sweep of the rules that pick the kernel variants of the two-kernel tile-binned loop (better_flow_amd/csrc/bf_plan_rules.h:
// no HIP, no context).  With the MI355X's 256 CUs, over scales 1 .. 9, sensors from 24 x 24 to 1920 x 1200, 1 .. 4M events, both
// homes of the update, the three scatter formats and the margins the tests use, it
//   * asserts that every (head, threads, events per thread, format) tuple the rules return is a compiled instantiation of the
//     scatter kernel (bf_rules::scatter_compiled: what launch_bin_warp_scatter dispatches, everything else is hipErrorInvalidValue),
//   * asserts the converse -- no instantiation is compiled that the rules never ask for,
//   * prints the reachable set, and, given the committed table (tests/variants_reachable.txt), asserts that it equals it.
// ... and sweeps the rule that picks the loop form and the home of the model update (bf_rules::loop_choice) over every
// combination of its options and boolean facts: one form, one home, and only the combinations the driver is written for.
// usage: test_plan [table]            the sweeps
//        test_plan rows < lines       one "H W scale n head fmt margin" per line -> the variants that slice lands on
//        test_plan forms < lines      one case of tests/loop_form_cases.py per line (facts_line) -> "id form name home format"
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

// ---- the loop form (bf_rules::loop_choice) -----------------------------------------------------------------------------------
static const char* const kFormName[] = {"atomic", "binned", "one_kernel", "persistent", "delta"};
static const char* const kHomeName[] = {"tail", "head", "separate"};

// One case of tests/loop_form_cases.py as LoopFacts.  What plan_slice finds possible is restated here for the cases' geometry --
// images far below every size limit, so only the options, the noise mask and the densities decide; the committed table, recorded
// on the device, holds this restatement and the rule together to what plan_slice and plan_run did.  Residency: a grid of fewer
// tiles than the 256 CUs is resident wherever one work-group fits a CU, which launching the kernel at all needs.
static int forms_mode() {
    char id[128];
    int H, W, scale, noise, warm, live, max_iter, binned, fused, persist, delta, sep, compact, split, co, force_split;
    long long n;
    while (scanf("%127s %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d", id, &H, &W, &scale, &n, &noise, &warm, &live, &max_iter, &binned,
                 &fused, &persist, &delta, &sep, &compact, &split, &co, &force_split) == 18) {
        const int R = scale * H, C = scale * W;
        const double P = (double)R * (double)C;
        const BinShape g = bin_shape(n, R, C, kCus, bin_margin(0));
        const bool usable = !force_split && !noise && n > 0;
        LoopFacts f;
        f.opt_binned = binned; f.opt_fused = fused; f.opt_persist = persist; f.opt_delta = delta; f.opt_sep_update = sep;
        f.co_schedule = co != 0;
        f.pixels = P; f.n = n; f.max_iter = max_iter;
        f.has_noise = noise != 0; f.packed = !force_split;
        f.warm = warm != 0; f.live_ctx = live;
        f.grid_ok = binned != 0 && usable && bin_grid_ok(g, R);   // (P <= 9e6: "dense" whatever n)
        f.fused_ok = (fused == 2 || (fused == 1 && 2.0 * (double)n <= P)) && binned != 0 && usable;
        f.fused_shared = f.fused_ok && (fused == 2 || 8.0 * (double)n <= P);
        const int mode = (f.grid_ok && bin_format_ok(g, 2)) ? compact : 0;
        if (mode == 2 || (mode == 1 && 4.0 * (double)n < P)) f.fmt = 2;
        if (f.fmt == 0 && f.grid_ok && split == 2 && bin_format_ok(g, 3)) f.fmt = 3;   // (P < 1.5e6: never by "auto")
        f.resident = ((R + 31) / 32) * ((C + 63) / 64) <= kCus;
        if (P > 1.2e6 || scale / 2 > 4) { printf("FAIL %s: outside the geometry this mode restates\n", id); return 1; }
        const LoopChoice ch = loop_choice(f);
        printf("%s %d %s %s %d\n", id, (int)ch.form, kFormName[(int)ch.form], kHomeName[(int)ch.home], f.grid_ok ? f.fmt : -1);
    }
    return 0;
}

// Every combination of the options and the boolean facts, at a few sizes: one form and one home whatever the facts, and the
// combinations the driver relies on.
static long long sweep_loop_choice() {
    long long failures = 0, swept = 0;
    const long long counts[] = {0, 1000, 30000, 1000000};
    const double pixels[] = {5400.0, 48600.0, 2.0e6, 3.0e8};
    const int caps[] = {-1, 0, 10, 199, 200};
    for (int opts = 0; opts < 243; ++opts)
        for (int bits = 0; bits < 256; ++bits)
            for (int fmt : {0, 2, 3})
                for (int live = 1; live <= 2; ++live)
                    for (long long n : counts)
                        for (double P : pixels)
                            for (int cap : caps) {
                                LoopFacts f;
                                f.opt_binned = opts % 3; f.opt_fused = opts / 3 % 3; f.opt_persist = opts / 9 % 3;
                                f.opt_delta = opts / 27 % 3; f.opt_sep_update = opts / 81 % 3;
                                f.co_schedule = bits & 1; f.has_noise = bits & 2; f.packed = bits & 4; f.warm = bits & 8;
                                f.grid_ok = bits & 16; f.fused_ok = bits & 32; f.fused_shared = bits & 64; f.resident = bits & 128;
                                f.fmt = fmt; f.live_ctx = live; f.n = n; f.pixels = P; f.max_iter = cap;
                                const LoopChoice ch = loop_choice(f);
                                const int form = (int)ch.form;
                                const bool planes = ch.form == LoopForm::atomic || ch.form == LoopForm::delta;
                                const bool one = ch.form == LoopForm::one_kernel || ch.form == LoopForm::persistent;
                                bool ok = form >= BF_LOOP_ATOMIC && form <= BF_LOOP_DELTA && (int)ch.home >= 0 && (int)ch.home <= 2;
                                ok = ok && (!planes || ch.home == UpdateHome::tail) && (!one || ch.home == UpdateHome::head);
                                ok = ok && (ch.home != UpdateHome::separate || (ch.form == LoopForm::binned && f.co_schedule));
                                ok = ok && (ch.form != LoopForm::binned || (f.grid_ok && (ch.home == UpdateHome::head) == !f.co_schedule));
                                ok = ok && (!one || f.fused_ok) && (ch.form != LoopForm::persistent || (!f.co_schedule && live == 1 && f.resident));
                                ok = ok && (ch.form != LoopForm::delta || (!f.has_noise && n > 0));
                                ok = ok && ((ch.form == LoopForm::persistent) == (persistent_ok(f) && !delta_ok(f)));
                                ++swept;
                                if (!ok && failures++ < 20) printf("FAIL loop_choice: opts %d bits %d fmt %d -> form %d home %d\n", opts, bits, fmt, form, (int)ch.home);
                            }
    printf("# %lld fact combinations swept for the loop form\n", swept);
    return failures;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "rows")) return rows_mode();
    if (argc > 1 && !strcmp(argv[1], "forms")) return forms_mode();
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
    failures += sweep_loop_choice();
    if (failures) { printf("%lld failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
