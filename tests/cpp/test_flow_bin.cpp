// bf::write_flow_binary (better_flow/event_reader.h) on a deterministic table of n rows, for the Python reader
// (better_flow_amd/flowio.py) to read back:  test_flow_bin <path> <n>.  Row i: t = 1e9 + 37 i, row = i % 65536,
// col = (7 i) % 65536, u = i / 3 - 5.5, v = -(i * 0.25) + 1e-300.  Built by tests/test_flow_output.py.
#include <better_flow/event_reader.h>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const size_t n = (size_t)std::atoll(argv[2]);
    std::vector<uint64_t> t(n);
    std::vector<uint16_t> row(n), col(n);
    std::vector<double> u(n), v(n);
    for (size_t i = 0; i < n; ++i) {
        t[i] = 1000000000ull + 37ull * i;
        row[i] = (uint16_t)(i % 65536); col[i] = (uint16_t)((7 * i) % 65536);
        u[i] = (double)i / 3 - 5.5; v[i] = -((double)i * 0.25) + 1e-300;
    }
    return bf::write_flow_binary(argv[1], t, row, col, u, v) ? 0 : 1;
}
