// StreamEngine with set_accumulate on an event file: one line per slice, "S <first> <n> <start_time> <lead>", then one line
// per row of get_accumulated(), "R <t> <row> <col>" -- for tests/test_flow_output.py to hold the numpy restatements of the
// marking rule (tests/emit_ref.py) to the host walk.  lead: the full ring's oldest element, left out of the slice, that no
// slice has held.  Linked against the CPU stand-in of the C-ABI (tests/shim).
//   test_accumulate_dump <events file> <max_sz> <span_ns> <on_ev> <on_time_ns>
#include <better_flow/common.h>
#include <better_flow/event_reader.h>
#include <better_flow/stream_flow.h>
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    std::vector<uint32_t> row, col;
    std::vector<ull> t;
    bf::EventReader reader(argv[1]);
    reader.for_each_event([&](unsigned r, unsigned c, unsigned long long ns) { row.push_back(r); col.push_back(c); t.push_back((ull)ns); });
    const size_t max_sz = (size_t)std::atoll(argv[2]);
    bf::StreamEngine e(max_sz, (sll)std::atoll(argv[3]), (ull)std::atoll(argv[4]), (ull)std::atoll(argv[5]));
    e.set_want_flow(false);
    e.set_accumulate();
    uint64_t prev_seen = 0;
    e.on_slice([&](const bf::SliceRecord &r) {
        const bool lead = r.ring_size == max_sz && r.first_event >= 1 && r.first_event - 1 >= prev_seen;
        std::printf("S %llu %llu %llu %d\n", (unsigned long long)r.first_event, (unsigned long long)r.events,
                    (unsigned long long)r.start_time, lead ? 1 : 0);
        prev_seen = r.events_seen;
    });
    e.add_events(row.data(), col.data(), t.data(), t.size());
    e.recompute();
    e.drain();
    const bf::FlowTable a = e.get_accumulated();
    for (size_t i = 0; i < a.size(); ++i) std::printf("R %llu %u %u\n", (unsigned long long)a.timestamp[i], a.row[i], a.col[i]);
    return 0;
}
