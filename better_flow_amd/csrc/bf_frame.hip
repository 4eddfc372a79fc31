// bf_frame.hip -- the per-slice frame of --img / --video composed on the device (bf_frame_render, bf_frame_abi.cpp): the
// 2 x 2 mosaic of DVS_flow::render_frame (host/better_flow/dvs_flow.h) written straight in the byte layouts of the files.
//
//   k_frame_compose  one thread per output dword.  A byte of the mosaic is one channel of one pixel, and every channel is
//                    computed on its own by frame_writer.h, so a thread derives its four bytes independently:
//                      * grey tiles (projection images, R x C): resize_bilinear is the identity, gray_to_bgr copies the value
//                        into all three channels;
//                      * colour tiles ((R + 3) x (C + 3) BGR): resize_bilinear to R x C with the row / column taps and
//                        weights the host computed once per geometry, in the same float operations and order as
//                        frame_writer.h (the library is built with -ffp-contract=off), rounded half to even (lrint);
//                      * mosaic_2x2: compensated tiles on top, raw below; grey left, colour right.
//                    PPM payload: top-down RGB, the bytes after the "P6" header.  AVI payload: bottom-up BGR rows padded to a
//                    multiple of 4 bytes, the padding zero (AviWriter::write).  With both layouts on, one launch writes both.
// Stores are whole dwords, consecutive lanes at consecutive addresses: the destinations are pinned, device-mapped frame
// slots, so the bytes cross the host link once.
#include <hip/hip_runtime.h>

#include "bf_kernels.h"

namespace bf {

namespace {

// one channel (0 B, 1 G, 2 R) of mosaic pixel (r, c)
__device__ __forceinline__ uint32_t frame_byte(const FrameCompose& a, int r, int c, int ch) {
    const int lower = r >= a.R, right = c >= a.C;
    const int rr = lower ? r - a.R : r, cc = right ? c - a.C : c;
    if (!right) return a.gray[lower][(size_t)rr * a.C + cc];
    const uint8_t* s = a.colour[lower];
    const int r0 = a.row0[rr], r1 = a.row1[rr], c0 = a.col0[cc], c1 = a.col1[cc];
    const float wr = a.row_w[rr], wc = a.col_w[cc];
    const size_t sc = (size_t)a.CC * 3;
    const float p00 = (float)s[r0 * sc + (size_t)c0 * 3 + ch], p01 = (float)s[r0 * sc + (size_t)c1 * 3 + ch];
    const float p10 = (float)s[r1 * sc + (size_t)c0 * 3 + ch], p11 = (float)s[r1 * sc + (size_t)c1 * 3 + ch];
    const float top = p00 + (p01 - p00) * wc;
    const float bot = p10 + (p11 - p10) * wc;
    const float v = top + (bot - top) * wr;
    return v <= 0.f ? 0u : (v >= 255.f ? 255u : (uint32_t)(int)__builtin_rintf(v));
}

__global__ void __launch_bounds__(256) k_frame_compose(FrameCompose a) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = 2 * a.C;                                // mosaic columns
    if (a.ppm && d < a.ppm_dwords) {                      // flat RGB: byte b = pixel b / 3, channel 2 - b % 3
        uint32_t w = 0;
        const long long b0 = 4 * d;
        long long p = b0 / 3;
        int k = (int)(b0 - 3 * p);
        for (int i = 0; i < 4; ++i) {
            w |= frame_byte(a, (int)(p / W), (int)(p % W), 2 - k) << (8 * i);
            if (++k == 3) { k = 0; ++p; }
        }
        reinterpret_cast<uint32_t*>(a.ppm)[d] = w;
    }
    if (a.avi && d < a.avi_dwords) {                      // rows of `stride` bytes, bottom-up, BGR, zero padding
        const long long b0 = 4 * d;
        const int line = (int)(b0 / a.stride), o = (int)(b0 - (long long)line * a.stride);
        const int r = 2 * a.R - 1 - line;
        uint32_t w = 0;
        int c = o / 3, k = o - 3 * (o / 3);
        for (int i = 0; i < 4; ++i) {
            if (c < W) w |= frame_byte(a, r, c, k) << (8 * i);
            if (++k == 3) { k = 0; ++c; }
        }
        reinterpret_cast<uint32_t*>(a.avi)[d] = w;
    }
}

}  // namespace

void launch_frame_compose(const FrameCompose& a, hipStream_t s) {
    long long n = 0;
    if (a.ppm) n = a.ppm_dwords;
    if (a.avi && a.avi_dwords > n) n = a.avi_dwords;
    if (n == 0) return;
    const int threads = 256;
    hipLaunchKernelGGL(k_frame_compose, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, s, a);
}

}  // namespace bf
