// The arithmetic of the interpolated cell flow field (include/bf_global_field.h) on the host alone: no GPU, no library.
// Reads argv[1]: 18 doubles (a 3 x 3 grid: nx, then ny), 12 validity digits (a 3 x 4 mask), 24 doubles (its nx, then ny; the
// invalid entries may be nan).  Prints the per-axis (a0, a1, w) of every address of a 24-pixel axis for cells of 8, 5, 1 and
// 7 pixels, the field at every pixel of a 24 x 24 sensor under the 3 x 3 grid of 8 x 8-pixel cells as hex doubles, and the
// filled 3 x 4 grid; tests/test_host_field_standalone.py compares them with tests/global_field_ref.py.
#include <bf_global_field.h>

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<double> grid(18), fill(24);
    std::vector<uint8_t> valid(12);
    bool ok = true;
    for (double &v : grid) ok = ok && std::fscanf(f, "%la", &v) == 1;
    for (uint8_t &m : valid) {
        int d = 0;
        ok = ok && std::fscanf(f, "%d", &d) == 1;
        m = (uint8_t)(d != 0);
    }
    for (double &v : fill) ok = ok && std::fscanf(f, "%la", &v) == 1;
    std::fclose(f);
    if (!ok) return 3;

    const uint32_t res = 24;
    for (uint32_t size : {8u, 5u, 1u, 7u}) {
        const uint32_t n_cell = (res + size - 1) / size;
        for (uint32_t x = 0; x < res; ++x) {
            uint32_t a0, a1, w;
            bf_field_axis(x, size, n_cell, &a0, &a1, &w);
            std::printf("axis %u %u %u %u %u\n", size, x, a0, a1, w);
        }
    }
    for (uint32_t x = 0; x < res; ++x)
        for (uint32_t y = 0; y < res; ++y) {
            double nx, ny;
            bf_field_at(x, y, 8, 8, 3, 3, grid.data(), grid.data() + 9, &nx, &ny);
            std::printf("field %u %u %a %a\n", x, y, nx, ny);
        }
    bf_field_fill(3, 4, valid.data(), fill.data(), fill.data() + 12);
    for (int i = 0; i < 12; ++i) std::printf("fill %d %a %a\n", i, fill[(size_t)i], fill[(size_t)i + 12]);
    // no valid cell at all: zeros
    std::vector<uint8_t> none(12, 0);
    bf_field_fill(3, 4, none.data(), fill.data(), fill.data() + 12);
    for (int i = 0; i < 12; ++i) std::printf("none %d %a %a\n", i, fill[(size_t)i], fill[(size_t)i + 12]);
    return 0;
}
