// StreamEngine::get_accumulated_device (the -o table built on the device by bf_emit_slice) against
// StreamEngine::get_accumulated (the host walk over the whole history) on one event stream: the same rows, element for
// element, u / v compared as bits.  Both tables come from one engine, so they see the same slices and the same flow.
//   test_emit <events file> <max_sz> <span_ns> <on_ev> <on_time_ns> <stm_off 0|1> <contexts> <rows> <cols>
// Prints "rows=<n> slices=<k> skipped=<s> diff=<d>" and exits 1 on any difference.  Built by tests/test_flow_output.py.
#include <better_flow/common.h>
#include <better_flow/event_reader.h>
#include <better_flow/stream_flow.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv) {
    if (argc != 10) { std::fprintf(stderr, "usage: test_emit file max_sz span_ns on_ev on_time_ns stm_off contexts rows cols\n"); return 2; }
    std::vector<uint32_t> row, col;
    std::vector<ull> t;
    bf::EventReader reader(argv[1]);
    reader.for_each_event([&](unsigned r, unsigned c, unsigned long long ns) { row.push_back(r); col.push_back(c); t.push_back((ull)ns); });
    bf::sensor().res_x = std::atoi(argv[8]);
    bf::sensor().res_y = std::atoi(argv[9]);
    const int contexts = std::atoi(argv[7]);
    try {
        bf::StreamEngine e((size_t)std::atoll(argv[2]), (sll)std::atoll(argv[3]), (ull)std::atoll(argv[4]), (ull)std::atoll(argv[5]));
        e.set_stm_disable(std::atoi(argv[6]) != 0);
        e.set_want_flow(false);
        e.set_accumulate();
        e.set_accumulate_device();
        if (contexts > 1) e.set_devices({bf::DeviceContext::device()}, contexts);
        e.set_pipelined(true);
        for (size_t k = 0; k < t.size(); k += 4096) {
            const size_t m = t.size() - k < 4096 ? t.size() - k : 4096;
            e.add_events(row.data() + k, col.data() + k, t.data() + k, m);
        }
        e.recompute();
        e.drain();
        const bf::FlowTable a = e.get_accumulated(), b = e.get_accumulated_device();
        size_t diff = a.size() == b.size() ? 0 : 1;
        for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
            const bool same = a.timestamp[i] == b.timestamp[i] && a.row[i] == b.row[i] && a.col[i] == b.col[i] &&
                              std::memcmp(&a.u[i], &b.u[i], 8) == 0 && std::memcmp(&a.v[i], &b.v[i], 8) == 0;
            if (!same && diff++ < 5)
                std::printf("row %zu: host %llu %u %u %.17g %.17g  device %llu %u %u %.17g %.17g\n", i, (unsigned long long)a.timestamp[i],
                            a.row[i], a.col[i], a.u[i], a.v[i], (unsigned long long)b.timestamp[i], b.row[i], b.col[i], b.u[i], b.v[i]);
        }
        std::printf("rows=%zu device_rows=%zu slices=%llu skipped=%llu diff=%zu\n", a.size(), b.size(), (unsigned long long)e.get_slices_done(),
                    (unsigned long long)e.get_slices_skipped(), diff);
        return diff ? 1 : 0;
    } catch (const bf::AccelError &err) {
        std::printf("error: %s\n", err.what());
        return 1;
    }
}
