/*
 * bf_global_field.h -- the arithmetic of the interpolated cell flow field (include/bf_accel.h, bf_global_project_field),
 * stated ONCE for the device kernels (compiled by hipcc, -ffp-contract=off), the C-ABI, the host class
 * (better_flow/optimizer_global.h) and the stand-alone test (g++): the per-axis corners and weight of a recorded address
 * between the nominal cell centres, the three-step bilinear interpolation, and, host only, the fill of the cells that
 * carry no answer and compute_uv of a direction.  C++ only; no state.
 */
#ifndef BF_GLOBAL_FIELD_H
#define BF_GLOBAL_FIELD_H

#include <math.h>
#include <stdint.h>

#ifndef BF_HD
#if defined(__HIPCC__)
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD inline
#endif
#endif

/* One axis of the grid: cells of `size` pixels, n_cell of them, cell a with its nominal centre at (a + 0.5) * size - 0.5
 * (a ragged last cell keeps it).  For the address x: p = 2x + 1 - size, D = 2 * size, a0 = floor(p / D), w = p - a0 * D in
 * [0, D); a0 < 0 -> a0 = 0, w = 0; a0 >= n_cell - 1 -> a0 = n_cell - 1, w = 0; a1 = min(a0 + 1, n_cell - 1).  The event
 * lies w / D of the way from centre a0 to centre a1; beyond the outermost centres the field is constant.
 *
 * This form takes the address as (a, r): its cell a = x / size and r = x - a * size in [0, size), which a kernel that walks
 * one cell knows without dividing.  Then 2r + 1 >= size <=> a0 = a, w = 2r + 1 - size; otherwise a0 = a - 1,
 * w = 2r + 1 + size -- the floor division above, case by case.  Unsigned 32-bit throughout: r < 2^16 for an event address
 * (x is 16 bits wide), so 2r + 1 + size < 2^32 for every int32 size. */
BF_HD void bf_field_axis_in_cell(uint32_t a, uint32_t r, uint32_t size, uint32_t n_cell, uint32_t* a0, uint32_t* a1,
                                 uint32_t* w) {
    const uint32_t h = 2u * r + 1u;
    const bool upper = h >= size;                 /* at or beyond the centre of its own cell */
    uint32_t lo = upper ? a : a - 1u, ww = upper ? h - size : h + size;
    if (!upper && a == 0u) { lo = 0u; ww = 0u; }  /* a0 < 0 */
    if (lo >= n_cell - 1u) { lo = n_cell - 1u; ww = 0u; }
    *a0 = lo;
    *a1 = lo + 1u < n_cell ? lo + 1u : n_cell - 1u;
    *w = ww;
}

/* ... for an address x < size * n_cell */
BF_HD void bf_field_axis(uint32_t x, uint32_t size, uint32_t n_cell, uint32_t* a0, uint32_t* a1, uint32_t* w) {
    const uint32_t a = x / size;
    bf_field_axis_in_cell(a, x - a * size, size, n_cell, a0, a1, w);
}

/* The weight of an axis as a double: one conversion each and one division */
BF_HD double bf_field_weight(uint32_t w, uint32_t size) { return (double)w / (double)(2u * size); }

/* n_ab = the grid value at (row a_a, column b_b); tx along the rows, ty along the columns.  Three steps, each one IEEE
 * operation after the other (no contraction), in this order -- it is part of the definition: a uniform grid gives n, and
 * tx == ty == 0 gives n00 (both as values: -0.0 comes back as +0.0). */
BF_HD double bf_field_interp(double n00, double n01, double n10, double n11, double tx, double ty) {
    const double top = n00 + ty * (n01 - n00);
    const double bot = n10 + ty * (n11 - n10);
    return top + tx * (bot - top);
}

/* The field at sensor pixel (x, y) of a grid of n_cell_x x n_cell_y cells of cell_rows x cell_cols pixels, row-major
 * tables.  (The kernels select the four corners from registers instead; the arithmetic is the functions above.) */
BF_HD void bf_field_at(uint32_t x, uint32_t y, uint32_t cell_rows, uint32_t cell_cols, uint32_t n_cell_x, uint32_t n_cell_y,
                       const double* cell_nx, const double* cell_ny, double* nx, double* ny) {
    uint32_t a0, a1, wx, b0, b1, wy;
    bf_field_axis(x, cell_rows, n_cell_x, &a0, &a1, &wx);
    bf_field_axis(y, cell_cols, n_cell_y, &b0, &b1, &wy);
    const double tx = bf_field_weight(wx, cell_rows), ty = bf_field_weight(wy, cell_cols);
    const uint32_t i00 = a0 * n_cell_y + b0, i01 = a0 * n_cell_y + b1, i10 = a1 * n_cell_y + b0, i11 = a1 * n_cell_y + b1;
    *nx = bf_field_interp(cell_nx[i00], cell_nx[i01], cell_nx[i10], cell_nx[i11], tx, ty);
    *ny = bf_field_interp(cell_ny[i00], cell_ny[i01], cell_ny[i10], cell_ny[i11], tx, ty);
}

/* The fill (host only): a cell is valid when valid[i] != 0; every other cell takes (nx, ny) of the valid cell with the
 * smallest da^2 + db^2 in cell indices, the lowest row-major index among equals; without any valid cell, (0, 0).  In
 * place: only invalid cells are written and only valid ones are read.  Cost: invalid x valid cells. */
inline void bf_field_fill(int32_t n_cell_x, int32_t n_cell_y, const uint8_t* valid, double* cell_nx, double* cell_ny) {
    const int64_t nc = (int64_t)n_cell_x * n_cell_y;
    for (int64_t i = 0; i < nc; ++i) {
        if (valid[i]) continue;
        const int64_t a = i / n_cell_y, b = i % n_cell_y;
        int64_t best = -1, best_d = 0;
        for (int64_t j = 0; j < nc; ++j) {
            if (!valid[j]) continue;
            const int64_t da = j / n_cell_y - a, db = j % n_cell_y - b, d = da * da + db * db;
            if (best < 0 || d < best_d) { best = j; best_d = d; }   /* strict: the lowest index among equals */
        }
        cell_nx[i] = best < 0 ? 0.0 : cell_nx[best];
        cell_ny[i] = best < 0 ? 0.0 : cell_ny[best];
    }
}

/* Event::compute_uv (event.h:135-142) of a direction (nx, ny, nz), on the host with the C library's hypot: the expression
 * the C-ABI uses for best_u / best_v (bf_global_get_events, bf_global_project_field), for host code that samples the field
 * itself (OptimizerGlobal::write_field_flo). */
inline void bf_field_uv(double nx, double ny, double nz, double* u, double* v) {
    const double xy_len = hypot(nx, ny);
    const double speed = xy_len / (nz / (1000000000 / (1 * 10000)));
    *u = xy_len == 0 ? 0 : speed * nx / xy_len;
    *v = xy_len == 0 ? 0 : speed * ny / xy_len;
}

#endif /* BF_GLOBAL_FIELD_H */
