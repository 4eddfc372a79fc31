// bf_flowimg.hip -- the per-pixel flow field of a slice and its colour coding, EventFile::color_flow_img
// (event_file.h:318-350), on the device; the rule is stated in include/bf_accel.h (bf_flow_field, bf_color_flow_img) and
// DESIGN.md section 12.  The C-ABI around these kernels is in bf_flow_abi.cpp.
//
//   F1 k_flow_owner   one thread per event: the pixel (int)pr of a non-noise event (pr from the resident f32 products, as
//                     k_proj_count forms it; C truncation with the x86 answer for NaN / out-of-range), then ONE 32-bit
//                     integer atomic of the event's UPLOAD index into the res_x x res_y owner plane -- atomicMin when the
//                     first uploaded event owns a pixel, atomicMax when the last one does.  The plane starts at 0xffffffff,
//                     which is the identity of the unsigned minimum and, read as -1, of the signed maximum.  An integer
//                     minimum / maximum does not depend on the order the work-groups run in.
//   F2 k_flow_field   one thread per pixel: the owner's (nx, ny) gathered from the upload-ordered array, (u, v) by uv_from_n
//                     -- the expression of k_compute_uv, so the field is bf_compute_uv's value at the owner as bits --, then
//                     whichever of the outputs were asked for: owner index, f64 (u, v), the .flo pair, the H / S bytes
//                     (bf_flow_hs) and the B, G, R bytes (bf_hsv_to_bgr_u8, the conversion of the colour-coded time image).
//   F2' k_flow_field_uv  F2 with the owner's (u, v) read from an upload-ordered array instead of derived from (nx, ny): the
//                     bf_global_* renders of a held flow (bf_global_hold_field / bf_global_hold_best).
//   k_flow_frame_compose  the flow frame: compensated projection image | colour-coded flow | raw projection image, written in
//                     the byte layouts of the files, one thread per output dword (like k_frame_compose, without a resize: every
//                     tile already has the frame's resolution).
#include <hip/hip_runtime.h>
#include <limits.h>

#include "bf_device.h"
#include "bf_device_fns.h"
#include "bf_kernels.h"

namespace bf {

namespace {

constexpr uint32_t kNoOwner = 0xffffffffu;

__global__ __launch_bounds__(kThreads) void k_flow_owner(const uint32_t* __restrict__ xy, const float2* __restrict__ p,
                                                         const uint32_t* __restrict__ perm, const uint8_t* __restrict__ noise,
                                                         long long n, int res_x, int res_y, int first,
                                                         uint32_t* __restrict__ owner) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t up = perm ? perm[i] : (uint32_t)i;
    if (noise && noise[up]) return;                                       // event_file.h:322
    const uint32_t v = xy[i];
    const float2 q = p[i];
    const int x = trunc_x86(pr_from_p(v & 0xffffu, q.x));                 // :324-325 (int x = e.best_pr_x)
    const int y = trunc_x86(pr_from_p(v >> 16, q.y));
    if ((x >= res_x) || (x < 0) || (y >= res_y) || (y < 0)) return;       // :327
    uint32_t* at = owner + ((size_t)x * (size_t)res_y + (size_t)y);
    if (first) atomicMin(at, up);
    else atomicMax(reinterpret_cast<int*>(at), (int)up);
}

__global__ __launch_bounds__(kThreads) void k_flow_field(const uint32_t* __restrict__ owner, const double2* __restrict__ nxny,
                                                         long long px, FlowFieldOut o) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= px) return;
    const uint32_t w = owner[i];
    const bool has = w != kNoOwner;
    double2 uv = make_double2(0.0, 0.0);
    if (has && nxny) uv = uv_from_n(nxny[w]);                             // (no warp has run: Event::reset, zero flow)
    if (o.owner) o.owner[i] = has ? (int32_t)w : -1;
    if (o.u) o.u[i] = uv.x;
    if (o.v) o.v[i] = uv.y;
    if (o.flo) o.flo[i] = has ? make_float2((float)uv.y, (float)uv.x) : make_float2(1e9f, 1e9f);   // horizontal = v, vertical = u
    if (o.hs || o.bgr) {
        int H = 0, S = 0;                                                 // cv::Scalar(0, 0, 255), :319
        if (has) bf_flow_hs(uv.x, uv.y, &H, &S);                          // :330-338
        if (o.hs) { o.hs[2 * i] = (uint8_t)H; o.hs[2 * i + 1] = (uint8_t)S; }
        if (o.bgr) bf_hsv_to_bgr_u8(H, S, 255, o.bgr + 3 * i);
    }
}

// k_flow_field for a flow that is (u, v) already (the held flow of the exhaustive search, whose nz is the candidate's own):
// the owner's pair is copied, not derived; every output as there.
__global__ __launch_bounds__(kThreads) void k_flow_field_uv(const uint32_t* __restrict__ owner, const double2* __restrict__ uvs,
                                                            long long px, FlowFieldOut o) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= px) return;
    const uint32_t w = owner[i];
    const bool has = w != kNoOwner;
    double2 uv = make_double2(0.0, 0.0);
    if (has && uvs) uv = uvs[w];
    if (o.owner) o.owner[i] = has ? (int32_t)w : -1;
    if (o.u) o.u[i] = uv.x;
    if (o.v) o.v[i] = uv.y;
    if (o.flo) o.flo[i] = has ? make_float2((float)uv.y, (float)uv.x) : make_float2(1e9f, 1e9f);
    if (o.hs || o.bgr) {
        int H = 0, S = 0;
        if (has) bf_flow_hs(uv.x, uv.y, &H, &S);
        if (o.hs) { o.hs[2 * i] = (uint8_t)H; o.hs[2 * i + 1] = (uint8_t)S; }
        if (o.bgr) bf_hsv_to_bgr_u8(H, S, 255, o.bgr + 3 * i);
    }
}

// one channel (0 B, 1 G, 2 R) of frame pixel (r, c); c in [0, 3 C)
__device__ __forceinline__ uint32_t flow_frame_byte(const FlowFrameCompose& a, int r, int c, int ch) {
    const int tile = c / a.C, cc = c - tile * a.C;
    const size_t at = (size_t)r * a.C + cc;
    return tile == 1 ? a.flow[3 * at + ch] : (tile == 0 ? a.left[at] : a.right[at]);
}

__global__ void __launch_bounds__(256) k_flow_frame_compose(FlowFrameCompose a) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = 3 * a.C;
    const long long pixels = (long long)a.R * W;
    if (a.ppm && d < a.ppm_dwords) {                      // flat RGB: byte b = pixel b / 3, channel 2 - b % 3
        uint32_t w = 0;
        const long long b0 = 4 * d;
        long long p = b0 / 3;
        int k = (int)(b0 - 3 * p);
        for (int i = 0; i < 4; ++i) {
            if (p < pixels) w |= flow_frame_byte(a, (int)(p / W), (int)(p % W), 2 - k) << (8 * i);   // (the last dword's tail)
            if (++k == 3) { k = 0; ++p; }
        }
        reinterpret_cast<uint32_t*>(a.ppm)[d] = w;
    }
    if (a.avi && d < a.avi_dwords) {                      // rows of `stride` bytes, bottom-up, BGR, zero padding
        const long long b0 = 4 * d;
        const int line = (int)(b0 / a.stride), o = (int)(b0 - (long long)line * a.stride);
        const int r = a.R - 1 - line;
        uint32_t w = 0;
        int c = o / 3, k = o - 3 * (o / 3);
        for (int i = 0; i < 4; ++i) {
            if (c < W) w |= flow_frame_byte(a, r, c, k) << (8 * i);
            if (++k == 3) { k = 0; ++c; }
        }
        reinterpret_cast<uint32_t*>(a.avi)[d] = w;
    }
}

}  // namespace

void launch_flow_owner(const FlowSources& e, int res_x, int res_y, int first, uint32_t* owner, hipStream_t s) {
    if (e.n <= 0) return;
    hipLaunchKernelGGL(k_flow_owner, dim3((unsigned)((e.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, e.xy, e.p, e.perm,
                       e.noise, e.n, res_x, res_y, first, owner);
}

void launch_flow_field(const uint32_t* owner, const double2* nxny, long long px, const FlowFieldOut& o, hipStream_t s) {
    if (px <= 0) return;
    hipLaunchKernelGGL(k_flow_field, dim3((unsigned)((px + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, owner, nxny, px, o);
}

void launch_flow_field_uv(const uint32_t* owner, const double2* uv, long long px, const FlowFieldOut& o, hipStream_t s) {
    if (px <= 0) return;
    hipLaunchKernelGGL(k_flow_field_uv, dim3((unsigned)((px + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, owner, uv, px, o);
}

void launch_flow_frame_compose(const FlowFrameCompose& a, hipStream_t s) {
    long long n = 0;
    if (a.ppm) n = a.ppm_dwords;
    if (a.avi && a.avi_dwords > n) n = a.avi_dwords;
    if (n == 0) return;
    const int threads = 256;
    hipLaunchKernelGGL(k_flow_frame_compose, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, a);
}

}  // namespace bf
