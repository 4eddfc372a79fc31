// bf_global.hip -- OptimizerGlobal (optimizer_global.cpp:4-150): a batched sweep of (nx, ny) candidates, each
// scored the way project_all does it, for gfx950.  B candidates per batch, three launches:
//
//   G1  k_global_project : Event::project (event.h:65-70,164-168) of every event under candidate b, the acceptance
//       test of :17-21, and the point form of the saturating scale x scale splat (:23-32): one 32-bit atomic at the
//       splat's centre in point plane b.
//   G2  k_global_tile    : per 32 x 64 tile of the bordered image of candidate b, in LDS: box sum of the points
//       (== the splat), saturation at 255 (each `if (< 255) ++` is order independent: min(255, total)), this build's
//       8-bit Gaussian (ksize = scale, BORDER_REFLECT_101; defined in include/bf_accel.h), and the non-zero sum and
//       count of the metric_wsize^2 window of get_event_score (:82-101) as separable integer sums.  Writes one u32 per
//       pixel: sum in bits 0-19, count in bits 20-31 (metric_wsize <= 63).
//   G3  k_global_fold    : per event, the B candidates IN ORDER: its window word, score = sum / count (double, then
//       float like current_scores), apply_score's strict `>` (event.h:113-121) into the running best, and
//       floor(score * 2^32) = (sum << 32) / count summed per candidate with integer atomics -- S(k), order free.
//
//   G3c k_global_fold_cells + k_global_cells_best replace G3 in bf_global_search_cells: the same per-event fold, walked in
//       cell order, with S(k, cell) summed per work-group on chip ("OptimizerGlobal").
//   P   bf_global_search_cells_pyramid: the candidates of a level are chosen on the device from the per-cell bests
//       (k_global_stride_mark / k_global_seed_mark into a bitmap of the lattice, a popcount-scan-write compaction into the
//       ascending list of k, k_global_cands_from_lattice), scored by the unchanged G1, G2 and G3c; the batch carries the
//       lattice k of each slot (GlobalCells::ks), by which k_global_cells_best breaks ties.
//   PW  bf_global_project_cells: one image of the slice with every event under its own cell's candidate:
//       k_global_project_runs (G1 over the cell-ordered runs, all into plane 0), the unchanged G2 on that one plane, and
//       k_global_score_runs (the score part of G3 per event, summed per cell); no per-event state is touched.  Both take the
//       event's candidate from a source, here the per-cell table (GlobalTableSource).
//   PF  bf_global_project_field: PW, the same two kernels, with the source that interpolates the candidate of every event
//       between the cell centres around its address (GlobalFieldSource; include/bf_global_field.h).
//
//   H   bf_global_hold_field / bf_global_hold_best: the per-event flow kept on the device for the renderers and the -o table
//       (k_global_hold_runs over the runs of PW / PF with their sources; k_global_hold_best from the per-event best state).
//
// Everything is an integer or one IEEE operation of the reference's own expression: results do not depend on the
// order in which work-groups run.  (The one exception is the held flow's (u, v): the device's hypot, see uv_from_n_nz.)
#include <hip/hip_runtime.h>
#include <limits.h>

#include <cstring>   // (rocprim's headers call memset without including it)

#include <rocprim/rocprim.hpp>

#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"
#include "../../include/bf_global_field.h"

namespace bf {

namespace {
constexpr int kGT = 256;        // threads per work-group
constexpr int kGTR = 32;        // G2 tile rows
constexpr int kGTC = 64;        // G2 tile columns
constexpr uint32_t kCntShift = 20;
constexpr uint32_t kSumMask = (1u << kCntShift) - 1u;

__device__ __forceinline__ int reflect101g(int i, int n) {   // cv::BORDER_REFLECT_101
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// optimizer_global.cpp:17-21 for one event under one candidate; false when rejected
__device__ __forceinline__ bool global_pixel(const GlobalGeom& g, const GlobalCand& c, uint32_t v, int32_t t, double& pr_x,
                                             double& pr_y, int& X, int& Y) {
    const float ft = (float)t;
    pr_x = pr_from_p(v & 0xffffu, c.kx * ft);
    pr_y = pr_from_p(v >> 16, c.ky * ft);
    X = trunc_x86(pr_x * (double)g.scale - (double)g.xs);
    Y = trunc_x86(pr_y * (double)g.scale - (double)g.ys);
    return !((X >= g.sx - g.scale) || (X < 0) || (Y >= g.sy - g.scale) || (Y < 0));
}
}  // namespace

__global__ __launch_bounds__(kGT) void k_global_project(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                        long long n, GlobalGeom g, const GlobalCand* __restrict__ cands,
                                                        uint32_t* __restrict__ pts) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    double pr_x, pr_y;
    int X, Y;
    if (!global_pixel(g, cands[b], xy[i], t[i], pr_x, pr_y, X, Y)) return;
    const int off = g.scale / 2 + g.mw / 2;   // :23-24: the splat's centre in the bordered image
    atomicAdd(&pts[(size_t)b * g.plane + (size_t)(X + off) * (size_t)g.Cb + (size_t)(Y + off)], 1u);
}

// LDS layout (rows x columns, H = scale / 2, W = metric_wsize / 2):
//   P  points          [r0 - W - 2H, r0 + TR + W + 2H) x [c0 - W - 2H, ...)  u32   (later reused for the row sums)
//   N  counts          [r0 - W - H,  r0 + TR + W + H)  x ...                  u16   (value at the REFLECTED pixel)
//   V  blurred, packed [r0 - W,      r0 + TR + W)      x ...                  u32   v | (v != 0) << 20
//   Hs row sums        [r0 - W,      r0 + TR + W)      x [c0, c0 + TC)        u32   (in P's space)
template <int H>
__global__ __launch_bounds__(kGT) void k_global_tile(const uint32_t* __restrict__ pts, GlobalGeom g,
                                                     uint32_t* __restrict__ win, uint8_t* __restrict__ img_out) {
    extern __shared__ uint32_t s_g[];
    const int W = g.mw / 2;
    const int Rb = g.Rb, Cb = g.Cb, tid = threadIdx.x, b = blockIdx.z;
    const int r0 = blockIdx.y * kGTR, c0 = blockIdx.x * kGTC;
    const int VR = kGTR + 2 * W, VC = kGTC + 2 * W;
    const int NR = VR + 2 * H, NC = VC + 2 * H;
    const int PR = NR + 2 * H, PC = NC + 2 * H;
    uint32_t* sP = s_g;
    uint32_t* sV = s_g + PR * PC;
    uint16_t* sN = reinterpret_cast<uint16_t*>(sV + VR * VC);
    const uint32_t* plane = pts + (size_t)b * g.plane;
    const int pr0 = r0 - W - 2 * H, pc0 = c0 - W - 2 * H;
    for (int idx = tid; idx < PR * PC; idx += kGT) {
        const int lr = idx / PC, lc = idx - lr * PC;
        const int gr = pr0 + lr, gc = pc0 + lc;
        sP[idx] = (gr >= 0 && gr < Rb && gc >= 0 && gc < Cb) ? plane[(size_t)gr * Cb + gc] : 0u;
    }
    __syncthreads();
    // counts: min(255, box sum of the points) at the reflected pixel (so that the blur below is a plain convolution);
    // a reflected box that leaves the tile's point window reads the plane itself
    const int nr0 = r0 - W - H, nc0 = c0 - W - H;
    for (int idx = tid; idx < NR * NC; idx += kGT) {
        const int lr = idx / NC, lc = idx - lr * NC;
        const int gr = reflect101g(nr0 + lr, Rb), gc = reflect101g(nc0 + lc, Cb);
        uint32_t acc = 0;
        const int ar = gr - H - pr0, ac = gc - H - pc0;
        if (ar >= 0 && ar + 2 * H < PR && ac >= 0 && ac + 2 * H < PC) {
#pragma unroll
            for (int da = 0; da <= 2 * H; ++da)
#pragma unroll
                for (int db = 0; db <= 2 * H; ++db) acc += sP[(ar + da) * PC + ac + db];
        } else {
            for (int da = -H; da <= H; ++da)
                for (int db = -H; db <= H; ++db) {
                    const int rr = gr + da, cc = gc + db;
                    if (rr >= 0 && rr < Rb && cc >= 0 && cc < Cb) acc += plane[(size_t)rr * Cb + cc];
                }
        }
        sN[idx] = (uint16_t)(acc < 255u ? acc : 255u);   // optimizer_global.cpp:27-31
    }
    __syncthreads();
    // this build's 8-bit Gaussian (scale 1: none, :34-36); outside the image 0 (no event window reaches there)
    constexpr int kTap[4][7] = {{1, 0, 0, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0, 0}, {1, 4, 6, 4, 1, 0, 0}, {2, 7, 14, 18, 14, 7, 2}};
    constexpr int kNorm[4] = {1, 4, 16, 64};
    constexpr int n2 = kNorm[H] * kNorm[H];
    for (int idx = tid; idx < VR * VC; idx += kGT) {
        const int lr = idx / VC, lc = idx - lr * VC;
        const int gr = r0 - W + lr, gc = c0 - W + lc;
        uint32_t pv = 0;
        if (gr >= 0 && gr < Rb && gc >= 0 && gc < Cb) {
            int acc = 0;
#pragma unroll
            for (int a = 0; a <= 2 * H; ++a) {
                int row = 0;
#pragma unroll
                for (int bb = 0; bb <= 2 * H; ++bb) row += kTap[H][bb] * (int)sN[(lr + a) * NC + lc + bb];
                acc += kTap[H][a] * row;
            }
            const uint32_t v = (uint32_t)((acc + n2 / 2) / n2);
            pv = v | ((v != 0u ? 1u : 0u) << kCntShift);
            if (img_out && lr >= W && lr < W + kGTR && lc >= W && lc < W + kGTC) img_out[(size_t)gr * Cb + gc] = (uint8_t)v;
        }
        sV[idx] = pv;
    }
    __syncthreads();
    // window sums, separable: along the columns into P's space, then along the rows
    uint32_t* sH = sP;
    for (int idx = tid; idx < VR * kGTC; idx += kGT) {
        const int lr = idx / kGTC, lc = idx - lr * kGTC;
        uint32_t acc = 0;
        for (int d = 0; d <= 2 * W; ++d) acc += sV[lr * VC + lc + d];
        sH[idx] = acc;
    }
    __syncthreads();
    uint32_t* out = win + (size_t)b * g.plane;
    for (int idx = tid; idx < kGTR * kGTC; idx += kGT) {
        const int lr = idx / kGTC, lc = idx - lr * kGTC;
        const int gr = r0 + lr, gc = c0 + lc;
        if (gr >= Rb || gc >= Cb) continue;
        uint32_t acc = 0;
        for (int d = 0; d <= 2 * W; ++d) acc += sH[(lr + d) * kGTC + lc];
        out[(size_t)gr * Cb + gc] = acc;
    }
}

// The running best of one event (apply_score, event.h:113-121), in registers while a batch is folded.
struct GlobalBest {
    double mx = 0, nx = 0, ny = 0, nz = 0, pr_x = 0, pr_y = 0;
    bool changed = false;
    __device__ __forceinline__ void load(const GlobalEventState& st, long long e) {
        mx = st.max_score[e]; nx = st.best_nx[e]; ny = st.best_ny[e]; nz = st.best_nz[e];
        pr_x = st.best_pr_x[e]; pr_y = st.best_pr_y[e];
    }
    __device__ __forceinline__ void store(const GlobalEventState& st, long long e) const {
        if (!changed) return;
        st.max_score[e] = mx; st.best_nx[e] = nx; st.best_ny[e] = ny; st.best_nz[e] = nz;
        st.best_pr_x[e] = pr_x; st.best_pr_y[e] = pr_y;
    }
};

// An accepted event at pixel (X, Y) of window plane b: its window word, the float score f (into scores_out when asked),
// and its return value, the event's share of S: floor(score * 2^32).
__device__ __forceinline__ unsigned long long global_score_pixel(const GlobalGeom& g, int b, int X, int Y,
                                                                 const uint32_t* __restrict__ win,
                                                                 float* __restrict__ scores_out, float& f) {
    const int off = g.scale / 2 + g.mw / 2;
    unsigned long long contrib = 0;
    const uint32_t w = win[(size_t)b * g.plane + (size_t)(X + off) * (size_t)g.Cb + (size_t)(Y + off)];
    const uint32_t sum = w & kSumMask, cnt = w >> kCntShift;
    const double score = cnt == 0u ? 0.0 : (double)sum / (double)cnt;   // get_event_score, :99
    f = (float)score;                                                    // current_scores (CV_32FC1)
    if (cnt) contrib = ((unsigned long long)sum << 32) / (unsigned long long)cnt;
    if (scores_out) scores_out[(size_t)X * (size_t)g.sy + (size_t)Y] = f;   // the same value from every event there
    return contrib;
}

// One event (v, ti) under candidate c, slot b of the batch: its window word, the score into the running best, and its
// return value, the event's share of S: floor(score * 2^32), 0 when the candidate rejects the event.
__device__ __forceinline__ unsigned long long global_fold_event(const GlobalGeom& g, const GlobalCand& c, int b, uint32_t v,
                                                                int32_t ti, const uint32_t* __restrict__ win,
                                                                float* __restrict__ scores_out, GlobalBest& best) {
    unsigned long long contrib = 0;
    double pr_x, pr_y;
    int X, Y;
    if (global_pixel(g, c, v, ti, pr_x, pr_y, X, Y)) {
        float f;
        contrib = global_score_pixel(g, b, X, Y, win, scores_out, f);
        if ((double)f > best.mx) {   // apply_score, event.h:113-121
            best.mx = f; best.nx = c.nx; best.ny = c.ny; best.nz = c.nz; best.pr_x = pr_x; best.pr_y = pr_y;
            best.changed = true;
        }
    }
    return contrib;
}

__global__ __launch_bounds__(kGT) void k_global_fold(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                     const uint32_t* __restrict__ perm, long long n, GlobalGeom g,
                                                     const GlobalCand* __restrict__ cands, int nb,
                                                     const uint32_t* __restrict__ win, GlobalEventState st,
                                                     unsigned long long* __restrict__ S, float* __restrict__ scores_out) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    const bool live = i < n;
    const long long e = live ? (perm ? (long long)perm[i] : i) : 0;   // the event's upload index
    uint32_t v = 0;
    int32_t ti = 0;
    GlobalBest best;
    if (live) {
        v = xy[i]; ti = t[i];
        best.load(st, e);
    }
    for (int b = 0; b < nb; ++b) {
        const unsigned long long contrib = live ? global_fold_event(g, cands[b], b, v, ti, win, scores_out, best) : 0;
        const unsigned long long tot = (unsigned long long)wave_total_dpp((long long)contrib);
        if ((threadIdx.x & 63) == 63 && tot) atomicAdd(&S[b], tot);
    }
    best.store(st, e);
}

// ---- the per-cell objective S(k, cell) (include/bf_accel.h) ----
// Membership is by the event's recorded address; the grid is anchored at sensor pixel (0, 0).
__device__ __forceinline__ uint32_t cell_of(uint32_t v, const GlobalCellGrid& cg) {
    return ((v & 0xffffu) / (uint32_t)cg.cell_rows) * (uint32_t)cg.n_cell_y + (v >> 16) / (uint32_t)cg.cell_cols;
}

__global__ __launch_bounds__(kGT) void k_global_cell_count(const uint32_t* __restrict__ xy, long long n, GlobalCellGrid cg,
                                                           uint32_t* __restrict__ count) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cell_of(xy[i], cg);
    if (c < (uint32_t)cg.n_cells) atomicAdd(&count[c], 1u);   // (the host checked the bounding box: always)
}

// The slot inside a cell is whichever the atomic hands out: the order of a cell's events is arbitrary, and nothing
// downstream depends on it (per-event state is indexed by upload index, every sum is an integer).
__global__ __launch_bounds__(kGT) void k_global_cell_order(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                           const uint32_t* __restrict__ perm, long long n, GlobalCellGrid cg,
                                                           const uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cursor,
                                                           uint32_t* __restrict__ cxy, int32_t* __restrict__ ct,
                                                           uint32_t* __restrict__ cidx) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = xy[i];
    const uint32_t c = cell_of(v, cg);
    if (c >= (uint32_t)cg.n_cells) return;
    const uint32_t j = cell_start[c] + atomicAdd(&cursor[c], 1u);
    if (j >= cell_start[c + 1]) return;   // (never: cell_start is the scan of this very count)
    cxy[j] = v; ct[j] = t[i];
    cidx[j] = perm ? perm[i] : (uint32_t)i;
}

// k_global_fold per event (the same global_fold_event), over a run of at most T events of ONE cell: the
// work-group's total of every candidate goes into the batch block [cell][b] with one 64-bit atomic (none when it is 0).
// T == 64: the wave's total is the work-group's.  T == 256: lane 63 of each wave parks its totals in LDS, and after one
// barrier thread b adds the four of candidate b.
template <int T>
__global__ __launch_bounds__(T) void k_global_fold_cells(GlobalCells cl, GlobalGeom g, const GlobalCand* __restrict__ cands,
                                                         int nb, const uint32_t* __restrict__ win, GlobalEventState st) {
    constexpr int kWaves = T / 64;
    __shared__ unsigned long long s_part[kWaves > 1 ? kGlobalCellStride * kWaves : 1];
    const uint32_t cell = cl.run_cell[blockIdx.x];
    const uint32_t j = cl.run_start[blockIdx.x] + threadIdx.x;
    const bool live = j < cl.cell_start[cell + 1];
    unsigned long long* out = cl.block + (size_t)cell * kGlobalCellStride;
    long long e = 0;   // the event's upload index
    uint32_t v = 0;
    int32_t ti = 0;
    GlobalBest best;
    if (live) {
        v = cl.xy[j]; ti = cl.t[j]; e = (long long)cl.idx[j];
        best.load(st, e);
    }
    for (int b = 0; b < nb; ++b) {
        const unsigned long long contrib = live ? global_fold_event(g, cands[b], b, v, ti, win, nullptr, best) : 0;
        const unsigned long long tot = (unsigned long long)wave_total_dpp((long long)contrib);
        if ((threadIdx.x & 63) == 63) {
            if (kWaves == 1) {
                if (tot) atomicAdd(&out[b], tot);
            } else {
                s_part[b * kWaves + (threadIdx.x >> 6)] = tot;
            }
        }
    }
    best.store(st, e);
    if (kWaves > 1) {
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            unsigned long long tot = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) tot += s_part[threadIdx.x * kWaves + w];
            if (tot) atomicAdd(&out[threadIdx.x], tot);
        }
    }
}

// ---- the interpolated field (include/bf_accel.h, bf_global_project_field): every event under the flow interpolated
// between the cell centres around its recorded address (include/bf_global_field.h) ----
// The run's cell (ca, cb) is the same for every lane, and every event of it has its upper-left corner a0 in {ca - 1, ca},
// b0 in {cb - 1, cb}: the four corners lie in the 3 x 3 neighbourhood of the cell, clamped at the borders of the grid
// (where bf_field_axis_in_cell clamps too).  Those 18 doubles are read through wave-uniform addresses into scalar
// registers; a lane picks its corners from them with selects -- no per-event gather from the tables.
struct GlobalFieldNbhd {
    double nx[3][3], ny[3][3];
    uint32_t ca, cb;
    __device__ __forceinline__ void load(const GlobalCellGrid& cg, uint32_t n_cell_x, uint32_t cell,
                                         const double* __restrict__ cell_nx, const double* __restrict__ cell_ny) {
        const uint32_t n_cell_y = (uint32_t)cg.n_cell_y;
        ca = cell / n_cell_y; cb = cell - ca * n_cell_y;
        const uint32_t ra[3] = {ca > 0u ? ca - 1u : 0u, ca, ca + 1u < n_cell_x ? ca + 1u : n_cell_x - 1u};
        const uint32_t rb[3] = {cb > 0u ? cb - 1u : 0u, cb, cb + 1u < n_cell_y ? cb + 1u : n_cell_y - 1u};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                nx[i][j] = cell_nx[ra[i] * n_cell_y + rb[j]];
                ny[i][j] = cell_ny[ra[i] * n_cell_y + rb[j]];
            }
    }
    // (nx_e, ny_e) of the event at address v, and the projection's (kx, ky) of it: make_cand's expressions
    __device__ __forceinline__ GlobalCand at(const GlobalCellGrid& cg, uint32_t n_cell_x, uint32_t v, double nz) const {
        uint32_t a0, a1, wx, b0, b1, wy;
        bf_field_axis_in_cell(ca, (v & 0xffffu) - ca * (uint32_t)cg.cell_rows, (uint32_t)cg.cell_rows, n_cell_x, &a0, &a1, &wx);
        bf_field_axis_in_cell(cb, (v >> 16) - cb * (uint32_t)cg.cell_cols, (uint32_t)cg.cell_cols, (uint32_t)cg.n_cell_y, &b0, &b1,
                              &wy);
        const double tx = bf_field_weight(wx, (uint32_t)cg.cell_rows), ty = bf_field_weight(wy, (uint32_t)cg.cell_cols);
        // a0 == ca: rows (1, 2) of the neighbourhood, else a0 == ca - 1 >= 0: rows (0, 1); a1 is the second of the pair
        // either way (row 2 is min(ca + 1, n_cell_x - 1)).  Likewise the columns.
        const bool ha = a0 == ca, hb = b0 == cb;
        double cx[2][2], cy[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double rx[3], ry[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                rx[j] = ha ? nx[i + 1][j] : nx[i][j];
                ry[j] = ha ? ny[i + 1][j] : ny[i][j];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                cx[i][j] = hb ? rx[j + 1] : rx[j];
                cy[i][j] = hb ? ry[j + 1] : ry[j];
            }
        }
        GlobalCand c;
        c.nx = bf_field_interp(cx[0][0], cx[0][1], cx[1][0], cx[1][1], tx, ty);
        c.ny = bf_field_interp(cy[0][0], cy[0][1], cy[1][0], cy[1][1], tx, ty);
        c.nz = nz;
        c.kx = (float)((double)(float)c.nx / nz);
        c.ky = (float)((double)(float)c.ny / nz);
        return c;
    }
};

// ---- the projections over cell runs (include/bf_accel.h): bf_global_project_cells and bf_global_project_field ----
// Where the candidate of an event comes from is a source: a plain struct passed to the kernel by value, with
//   Run               what it keeps per run, in registers;
//   load(run, cell)   once per work-group: the run's cell is the same for every lane, so its reads go through wave-uniform
//                     addresses;
//   at(run, v)        the candidate of the event at address v;
//   store_event(...)  whatever it writes per event of the slice, accepted or not (the projecting kernel only).
// The kernels below are instantiated per (run length, source): nothing about the source is decided while they run.

// The per-cell table (bf_global_project_cells): every event under its own cell's candidate.
struct GlobalTableSource : GlobalCandTable {
    using Run = GlobalCand;
    __device__ __forceinline__ void load(Run& run, uint32_t cell) const { run = cell_cands[cell]; }
    __device__ __forceinline__ GlobalCand at(const Run& run, uint32_t) const { return run; }
    __device__ __forceinline__ void store_event(const GlobalCand&, const uint32_t*, uint32_t) const {}
};

// The interpolated field (bf_global_project_field): the neighbourhood of the run's cell, then the candidate per event.
// ev_nx / ev_ny (null: not asked for): (nx_e, ny_e) of the event at its upload index.
struct GlobalFieldSource : GlobalCandField {
    using Run = GlobalFieldNbhd;
    __device__ __forceinline__ void load(Run& run, uint32_t cell) const { run.load(cg, n_cell_x, cell, cell_nx, cell_ny); }
    __device__ __forceinline__ GlobalCand at(const Run& run, uint32_t v) const { return run.at(cg, n_cell_x, v, nz); }
    __device__ __forceinline__ void store_event(const GlobalCand& c, const uint32_t* __restrict__ idx, uint32_t j) const {
        if (!ev_nx) return;
        const uint32_t e = idx[j];   // the event's upload index
        ev_nx[e] = c.nx; ev_ny[e] = c.ny;
    }
};

// The total of `contrib` over the work-group of T threads, all of which call this, into *out with one 64-bit atomic (none
// when it is 0).  T == 64: the wave's total is the work-group's.  T == 256: lane 63 of each wave parks its total in LDS,
// and after one barrier thread 0 adds the four.
template <int T>
__device__ __forceinline__ void global_group_total(unsigned long long contrib, unsigned long long* __restrict__ out) {
    constexpr int kWaves = T / 64;
    __shared__ unsigned long long s_part[kWaves];
    const unsigned long long tot = (unsigned long long)wave_total_dpp((long long)contrib);
    if (kWaves == 1) {
        if (threadIdx.x == 63 && tot) atomicAdd(out, tot);
    } else {
        if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = tot;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long all = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) all += s_part[w];
            if (all) atomicAdd(out, all);
        }
    }
}

// G1 over the runs of k_global_fold_cells, one work-group per run; all cells splat into plane 0.
template <int T, class Src>
__global__ __launch_bounds__(T) void k_global_project_runs(GlobalCells cl, GlobalGeom g, Src src, uint32_t* __restrict__ pts) {
    const uint32_t cell = cl.run_cell[blockIdx.x];
    typename Src::Run run;
    src.load(run, cell);
    const uint32_t j = cl.run_start[blockIdx.x] + threadIdx.x;
    if (j >= cl.cell_start[cell + 1]) return;
    const uint32_t v = cl.xy[j];
    const GlobalCand c = src.at(run, v);
    src.store_event(c, cl.idx, j);
    double pr_x, pr_y;
    int X, Y;
    if (!global_pixel(g, c, v, cl.t[j], pr_x, pr_y, X, Y)) return;
    const int off = g.scale / 2 + g.mw / 2;   // the splat's centre, as in k_global_project
    atomicAdd(&pts[(size_t)(X + off) * (size_t)g.Cb + (size_t)(Y + off)], 1u);
}

// G3 over the same runs: per event global_score_pixel at its pixel under its candidate, recomputed (window plane 0), then
// the work-group's total into cell_sums[cell].  The per-event state is neither read nor written.
template <int T, class Src>
__global__ __launch_bounds__(T) void k_global_score_runs(GlobalCells cl, GlobalGeom g, Src src, const uint32_t* __restrict__ win,
                                                         float* __restrict__ scores_out,
                                                         unsigned long long* __restrict__ cell_sums) {
    const uint32_t cell = cl.run_cell[blockIdx.x];
    typename Src::Run run;
    src.load(run, cell);
    const uint32_t j = cl.run_start[blockIdx.x] + threadIdx.x;
    unsigned long long contrib = 0;
    if (j < cl.cell_start[cell + 1]) {
        const uint32_t v = cl.xy[j];
        double pr_x, pr_y;
        int X, Y;
        float f;
        if (global_pixel(g, src.at(run, v), v, cl.t[j], pr_x, pr_y, X, Y))
            contrib = global_score_pixel(g, 0, X, Y, win, scores_out, f);
    }
    global_group_total<T>(contrib, &cell_sums[cell]);
}

// ---- the held flow (include/bf_accel.h): bf_global_hold_field and bf_global_hold_best ----
// What one event keeps under candidate c: the products of Event::apply_project at position j of the source order, and
// (nx, ny) and compute_uv of them (uv_from_n_nz, with the candidate's own nz) at its upload index e.
__device__ __forceinline__ void global_hold_event(const GlobalHeld& h, const GlobalCand& c, int32_t t, long long j, long long e) {
    const float ft = (float)t;
    h.p[j] = make_float2(c.kx * ft, c.ky * ft);   // (global_pixel's products: pr_from_p of them is its pr)
    const double2 n = make_double2(c.nx, c.ny);
    h.nxny[e] = n;
    h.uv[e] = uv_from_n_nz(n, c.nz);
}

// k_global_project_runs without the pixel: over the same runs, the candidate of every event from the same source, kept
// instead of splatted.
template <int T, class Src>
__global__ __launch_bounds__(T) void k_global_hold_runs(GlobalCells cl, Src src, GlobalHeld h) {
    const uint32_t cell = cl.run_cell[blockIdx.x];
    typename Src::Run run;
    src.load(run, cell);
    const uint32_t j = cl.run_start[blockIdx.x] + threadIdx.x;
    if (j >= cl.cell_start[cell + 1]) return;
    global_hold_event(h, src.at(run, cl.xy[j]), cl.t[j], (long long)j, (long long)cl.idx[j]);
}

// The per-event best state, one thread per slot: the candidate is the event's (best_nx, best_ny, best_nz), kx / ky by
// make_cand's expression.  An event no candidate was accepted for holds k_global_reset's (0, 0, 127): zero products, pr = fr.
__global__ __launch_bounds__(kGT) void k_global_hold_best(const uint32_t* __restrict__ xy, const int32_t* __restrict__ t,
                                                          const uint32_t* __restrict__ perm, long long n, GlobalEventState st,
                                                          GlobalHeld h) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    if (i >= n) return;
    const long long e = perm ? (long long)perm[i] : i;
    GlobalCand c;
    c.nx = st.best_nx[e]; c.ny = st.best_ny[e]; c.nz = st.best_nz[e];
    c.kx = (float)((double)(float)c.nx / c.nz);
    c.ky = (float)((double)(float)c.ny / c.nz);
    h.xy[i] = xy[i]; h.idx[i] = (uint32_t)e;
    global_hold_event(h, c, t[i], i, e);
}

// One batch's block [cell][b], kGlobalCellStride threads per cell (8 cells per work-group).  Slot b is lattice point
// k = ks[b], or k0 + b without a list.  The cell's best of the batch is its largest sum, lowest k among equals, and it
// replaces the running best when it is larger, or as large with a lower k: the exhaustive rule (largest S, then lowest k)
// over whatever has been evaluated, in any order.  The surface column [cell][k0 + b] gets its copy, the block is left
// zero for the next batch, and the batch's S(k) = the sum over cells: over the work-group's 8 cells in LDS, then one
// integer atomic per candidate.
//
// On an ascending sweep (bf_global_search_cells: k0 = 0, 32, ...) this is folding the sums in order with strict `>`:
//   - inside a batch k rises with b, so "lowest k among equals" is the first largest.  A lane past nb carries sum 0 and
//     kGlobalNoCand, above every k (< 2^26): it loses a tie against any live lane, and lane 0 is always live (nb >= 1),
//     so the winner's k is a candidate's;
//   - every k of a later batch exceeds the running best_k, so an equal sum never replaces it: only a larger one does;
//   - best_k starts at kGlobalNoCand and best_sum at 0, so the first batch always sets best_k: to its first largest, which
//     for a cell without events, or whose sums are all zero, is k 0 -- and all later zeros leave it there.
__global__ __launch_bounds__(kGT) void k_global_cells_best(GlobalCells cl, int nb, unsigned long long* __restrict__ S) {
    constexpr int kCellsPerGroup = kGT / kGlobalCellStride;
    __shared__ unsigned long long s_v[kGT];
    const int b = threadIdx.x % kGlobalCellStride;
    const long long cell = (long long)blockIdx.x * kCellsPerGroup + threadIdx.x / kGlobalCellStride;
    const bool live = cell < cl.n_cells && b < nb;
    unsigned long long v = 0;
    uint32_t k = kGlobalNoCand;
    if (live) {
        unsigned long long* p = cl.block + (size_t)cell * kGlobalCellStride + b;
        v = *p;
        if (v) *p = 0;
        k = cl.ks ? cl.ks[b] : (uint32_t)(cl.k0 + b);
        if (cl.surface) cl.surface[(size_t)cell * (size_t)cl.n_cand + (size_t)(cl.k0 + b)] = (long long)v;
    }
    s_v[threadIdx.x] = v;
    for (int d = kGlobalCellStride / 2; d > 0; d >>= 1) {   // (the 32 lanes of a cell are one half of a wave)
        const unsigned long long ov = __shfl_xor(v, d, kGlobalCellStride);
        const uint32_t ok = __shfl_xor(k, d, kGlobalCellStride);
        if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
    if (b == 0 && cell < cl.n_cells) {
        const unsigned long long bv = cl.best_sum[cell];
        if (v > bv || (v == bv && k < cl.best_k[cell])) {
            cl.best_sum[cell] = v;
            cl.best_k[cell] = k;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
        unsigned long long tot = 0;
#pragma unroll
        for (int c = 0; c < kCellsPerGroup; ++c) tot += s_v[c * kGlobalCellStride + threadIdx.x];
        if (tot) atomicAdd(&S[threadIdx.x], tot);
    }
}

// ---- the candidate set of a pyramid level (include/bf_accel.h) ----
// One thread per strided lattice point; the OR is a vector atomic, so the bitmap does not depend on the order.
__global__ __launch_bounds__(kGT) void k_global_stride_mark(GlobalLattice lt, long long stride, long long m_x, long long m_y,
                                                            uint32_t* __restrict__ level) {
    const long long q = (long long)blockIdx.x * kGT + threadIdx.x;
    if (q >= m_x * m_y) return;
    const long long k = (q / m_y) * stride * lt.n_y + (q % m_y) * stride;   // (i, j) < (n_x, n_y): m = ceil(n / stride)
    atomicOr(&level[k >> 5], 1u << (k & 31));
}

// One thread per (cell, a, b), |a|, |b| <= radius.
__global__ __launch_bounds__(kGT) void k_global_seed_mark(GlobalLattice lt, long long stride, int radius, long long total,
                                                          const uint32_t* __restrict__ cell_start,
                                                          const unsigned long long* __restrict__ best_sum,
                                                          const uint32_t* __restrict__ best_k, const int32_t* __restrict__ seed,
                                                          const uint32_t* __restrict__ evaluated, uint32_t* __restrict__ level) {
    const long long q = (long long)blockIdx.x * kGT + threadIdx.x;
    if (q >= total) return;
    const int w = 2 * radius + 1;
    const long long cell = q / (w * w);
    const int ab = (int)(q - cell * (w * w));
    const int a = ab / w - radius, b = ab % w - radius;
    if (cell_start[cell + 1] == cell_start[cell]) return;   // no event
    long long kc;
    if (best_sum[cell] > 0) {
        kc = (long long)best_k[cell];
    } else {
        if (!seed || seed[cell] < 0) return;
        kc = (long long)seed[cell];
    }
    const long long i = kc / lt.n_y + (long long)a * stride, j = kc % lt.n_y + (long long)b * stride;
    if (i < 0 || i >= lt.n_x || j < 0 || j >= lt.n_y) return;   // clipped
    const long long k = i * lt.n_y + j;
    const uint32_t bit = 1u << (k & 31);
    if (evaluated[k >> 5] & bit) return;
    atomicOr(&level[k >> 5], bit);
}

__global__ __launch_bounds__(kGT) void k_global_bitmap_count(const uint32_t* __restrict__ level, long long n_words,
                                                             uint32_t* __restrict__ cnt) {
    const long long w = (long long)blockIdx.x * kGT + threadIdx.x;
    if (w > n_words) return;
    cnt[w] = w < n_words ? (uint32_t)__popc(level[w]) : 0u;   // (entry n_words: the scan leaves the total there)
}

// One thread per word, which it alone reads and writes.
__global__ __launch_bounds__(kGT) void k_global_bitmap_list(uint32_t* __restrict__ level, uint32_t* __restrict__ evaluated,
                                                            long long n_words, const uint32_t* __restrict__ offs,
                                                            uint32_t* __restrict__ list) {
    const long long w = (long long)blockIdx.x * kGT + threadIdx.x;
    if (w >= n_words) return;
    uint32_t bits = level[w];
    if (!bits) return;
    evaluated[w] |= bits;
    level[w] = 0u;
    uint32_t at = offs[w];
    while (bits) {
        const int bit = __ffs((int)bits) - 1;
        list[at++] = (uint32_t)(w * 32 + bit);
        bits &= bits - 1u;
    }
}

__global__ __launch_bounds__(kGT) void k_global_cands_from_lattice(GlobalLattice lt, const uint32_t* __restrict__ list,
                                                                   long long m, const GlobalAxis* __restrict__ tab_x,
                                                                   const GlobalAxis* __restrict__ tab_y, double nz,
                                                                   GlobalCand* __restrict__ cands) {
    const long long q = (long long)blockIdx.x * kGT + threadIdx.x;
    if (q >= m) return;
    const long long k = (long long)list[q];
    const GlobalAxis x = tab_x[k / lt.n_y], y = tab_y[k % lt.n_y];
    GlobalCand c;
    c.nx = x.n; c.ny = y.n; c.nz = nz; c.kx = x.k; c.ky = y.k;
    cands[q] = c;
}

// Event(x, y, t) of the reference (event.h:31-35): max_score 0, best_pr = fr; best (nx, ny) = 0 (best_u / best_v 0)
__global__ __launch_bounds__(kGT) void k_global_reset(const uint32_t* __restrict__ xy, const uint32_t* __restrict__ perm,
                                                      long long n, GlobalEventState st) {
    const long long i = (long long)blockIdx.x * kGT + threadIdx.x;
    if (i >= n) return;
    const long long e = perm ? (long long)perm[i] : i;
    const uint32_t v = xy[i];
    st.max_score[e] = 0.0; st.best_nx[e] = 0.0; st.best_ny[e] = 0.0; st.best_nz[e] = 127.0;
    st.best_pr_x[e] = (double)(v & 0xffffu); st.best_pr_y[e] = (double)(v >> 16);
}

size_t global_tile_lds(int scale, int mw) {
    const int H = scale / 2, W = mw / 2;
    const int VR = kGTR + 2 * W, VC = kGTC + 2 * W;
    const int NR = VR + 2 * H, NC = VC + 2 * H;
    const int PR = NR + 2 * H, PC = NC + 2 * H;
    size_t p = (size_t)PR * PC;
    const size_t hs = (size_t)VR * kGTC;
    if (hs > p) p = hs;
    return (p + (size_t)VR * VC) * 4 + (size_t)NR * NC * 2;
}

void launch_global_reset(const uint32_t* xy, const uint32_t* perm, long long n, const GlobalEventState& st, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_global_reset, dim3((unsigned)((n + kGT - 1) / kGT)), dim3(kGT), 0, s, xy, perm, n, st);
}

namespace {
// G2 over nb point planes (scale <= 7: the caller checked); < 0 as launch_global_batch
int launch_global_tile(const GlobalGeom& g, int nb, const uint32_t* pts, uint32_t* win, uint8_t* img_out, hipStream_t s) {
    void (*k)(const uint32_t*, GlobalGeom, uint32_t*, uint8_t*) =
        g.scale / 2 == 0 ? k_global_tile<0> : (g.scale / 2 == 1 ? k_global_tile<1> : (g.scale / 2 == 2 ? k_global_tile<2> : k_global_tile<3>));
    const size_t lds = global_tile_lds(g.scale, g.mw);
    if (lds > 160 * 1024) return -3;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -2;
    const dim3 grid((unsigned)((g.Cb + kGTC - 1) / kGTC), (unsigned)((g.Rb + kGTR - 1) / kGTR), (unsigned)nb);
    hipLaunchKernelGGL(k, grid, dim3(kGT), lds, s, pts, g, win, img_out);
    return 0;
}
// A kernel over the cell runs, compiled for both run lengths: one work-group of cells.run_len (64 or kGT) threads per run.
template <class T> struct AsIs { using type = T; };   // (the argument types come from the kernel, not from the call)
template <class... A>
void launch_over_runs(const GlobalCells& cells, hipStream_t s, void (*k64)(A...), void (*k256)(A...), typename AsIs<A>::type... args) {
    const bool one_wave = cells.run_len == 64;
    hipLaunchKernelGGL(one_wave ? k64 : k256, dim3((unsigned)cells.n_runs), dim3(one_wave ? 64 : kGT), 0, s, args...);
}

template <class Src>
int launch_runs(const GlobalCells& cells, const GlobalGeom& g, const Src& src, uint32_t* pts, uint32_t* win, uint8_t* img_out,
                float* scores_out, unsigned long long* cell_sums, hipStream_t s) {
    if (cells.n_runs <= 0 || g.Rb <= 0 || g.Cb <= 0) return 0;
    if (g.scale / 2 > 3) return -1;
    launch_over_runs(cells, s, k_global_project_runs<64, Src>, k_global_project_runs<kGT, Src>, cells, g, src, pts);
    const int tr = launch_global_tile(g, 1, pts, win, img_out, s);
    if (tr != 0) return tr;
    launch_over_runs(cells, s, k_global_score_runs<64, Src>, k_global_score_runs<kGT, Src>, cells, g, src, win, scores_out, cell_sums);
    return 0;
}
}  // namespace

int launch_global_batch(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalGeom& g,
                        const GlobalCand* cands, int nb, uint32_t* pts, uint32_t* win, uint8_t* img_out,
                        const GlobalEventState& st, unsigned long long* S, float* scores_out, const GlobalCells* cells,
                        hipStream_t s) {
    if (nb <= 0 || n <= 0 || g.Rb <= 0 || g.Cb <= 0) return 0;
    if (g.scale / 2 > 3) return -1;
    if (cells && nb > kGlobalCellStride) return -1;
    const unsigned eg = (unsigned)((n + kGT - 1) / kGT);
    hipLaunchKernelGGL(k_global_project, dim3(eg, (unsigned)nb), dim3(kGT), 0, s, xy, t, n, g, cands, pts);
    const int tr = launch_global_tile(g, nb, pts, win, img_out, s);
    if (tr != 0) return tr;
    if (!cells) {
        hipLaunchKernelGGL(k_global_fold, dim3(eg), dim3(kGT), 0, s, xy, t, perm, n, g, cands, nb, win, st, S, scores_out);
        return 0;
    }
    launch_over_runs(*cells, s, k_global_fold_cells<64>, k_global_fold_cells<kGT>, *cells, g, cands, nb, win, st);
    constexpr int per = kGT / kGlobalCellStride;
    const dim3 cgrid((unsigned)((cells->n_cells + per - 1) / per));
    hipLaunchKernelGGL(k_global_cells_best, cgrid, dim3(kGT), 0, s, *cells, nb, S);
    return 0;
}

int launch_global_runs(const GlobalCells& cells, const GlobalGeom& g, const GlobalCandTable& src, uint32_t* pts, uint32_t* win,
                       uint8_t* img_out, float* scores_out, unsigned long long* cell_sums, hipStream_t s) {
    return launch_runs(cells, g, GlobalTableSource{src}, pts, win, img_out, scores_out, cell_sums, s);
}

int launch_global_runs(const GlobalCells& cells, const GlobalGeom& g, const GlobalCandField& src, uint32_t* pts, uint32_t* win,
                       uint8_t* img_out, float* scores_out, unsigned long long* cell_sums, hipStream_t s) {
    return launch_runs(cells, g, GlobalFieldSource{src}, pts, win, img_out, scores_out, cell_sums, s);
}

void launch_global_hold(const GlobalCells& cells, const GlobalCandTable& src, const GlobalHeld& h, hipStream_t s) {
    if (cells.n_runs <= 0) return;
    launch_over_runs(cells, s, k_global_hold_runs<64, GlobalTableSource>, k_global_hold_runs<kGT, GlobalTableSource>, cells,
                     GlobalTableSource{src}, h);
}

void launch_global_hold(const GlobalCells& cells, const GlobalCandField& src, const GlobalHeld& h, hipStream_t s) {
    if (cells.n_runs <= 0) return;
    launch_over_runs(cells, s, k_global_hold_runs<64, GlobalFieldSource>, k_global_hold_runs<kGT, GlobalFieldSource>, cells,
                     GlobalFieldSource{src}, h);
}

void launch_global_hold_best(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalEventState& st,
                             const GlobalHeld& h, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_global_hold_best, dim3((unsigned)((n + kGT - 1) / kGT)), dim3(kGT), 0, s, xy, t, perm, n, st, h);
}

void launch_global_stride_mark(const GlobalLattice& lt, long long stride, uint32_t* level, hipStream_t s) {
    const long long m_x = (lt.n_x + stride - 1) / stride, m_y = (lt.n_y + stride - 1) / stride;
    if (m_x * m_y <= 0) return;
    hipLaunchKernelGGL(k_global_stride_mark, dim3((unsigned)((m_x * m_y + kGT - 1) / kGT)), dim3(kGT), 0, s, lt, stride, m_x, m_y,
                       level);
}

void launch_global_seed_mark(const GlobalLattice& lt, long long stride, int radius, int n_cells, const uint32_t* cell_start,
                             const unsigned long long* best_sum, const uint32_t* best_k, const int32_t* seed,
                             const uint32_t* evaluated, uint32_t* level, hipStream_t s) {
    const long long w = 2 * radius + 1, total = (long long)n_cells * w * w;   // <= 2^16 * 129^2: the grid fits 32 bits
    if (total <= 0) return;
    hipLaunchKernelGGL(k_global_seed_mark, dim3((unsigned)((total + kGT - 1) / kGT)), dim3(kGT), 0, s, lt, stride, radius, total,
                       cell_start, best_sum, best_k, seed, evaluated, level);
}

size_t global_scan_temp_bytes(long long n_words) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)(n_words + 1),
                                  rocprim::plus<uint32_t>());
    return b;
}

hipError_t launch_global_bitmap_scan(const uint32_t* level, long long n_words, uint32_t* cnt, uint32_t* offs, void* temp,
                                     size_t temp_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_global_bitmap_count, dim3((unsigned)((n_words + 1 + kGT - 1) / kGT)), dim3(kGT), 0, s, level, n_words, cnt);
    return rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)cnt, offs, 0u, (size_t)(n_words + 1),
                                   rocprim::plus<uint32_t>(), s);
}

void launch_global_bitmap_list(uint32_t* level, uint32_t* evaluated, long long n_words, const uint32_t* offs, uint32_t* list,
                               hipStream_t s) {
    hipLaunchKernelGGL(k_global_bitmap_list, dim3((unsigned)((n_words + kGT - 1) / kGT)), dim3(kGT), 0, s, level, evaluated, n_words,
                       offs, list);
}

void launch_global_cands_from_lattice(const GlobalLattice& lt, const uint32_t* list, long long m, const GlobalAxis* tab_x,
                                      const GlobalAxis* tab_y, double nz, GlobalCand* cands, hipStream_t s) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_global_cands_from_lattice, dim3((unsigned)((m + kGT - 1) / kGT)), dim3(kGT), 0, s, lt, list, m, tab_x, tab_y,
                       nz, cands);
}

void launch_global_cell_count(const uint32_t* xy, long long n, const GlobalCellGrid& cg, uint32_t* count, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_global_cell_count, dim3((unsigned)((n + kGT - 1) / kGT)), dim3(kGT), 0, s, xy, n, cg, count);
}

void launch_global_cell_order(const uint32_t* xy, const int32_t* t, const uint32_t* perm, long long n, const GlobalCellGrid& cg,
                              const uint32_t* cell_start, uint32_t* cursor, uint32_t* cxy, int32_t* ct, uint32_t* cidx,
                              hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_global_cell_order, dim3((unsigned)((n + kGT - 1) / kGT)), dim3(kGT), 0, s, xy, t, perm, n, cg, cell_start,
                       cursor, cxy, ct, cidx);
}

}  // namespace bf
