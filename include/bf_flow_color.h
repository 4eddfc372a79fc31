/*
 * bf_flow_color.h -- the per-pixel colour arithmetic of the rendered images, stated ONCE for the device kernels (compiled
 * by hipcc, -ffp-contract=off) and for the host front end's compositions (g++): HSV -> BGR of include/bf_accel.h's
 * bf_color_time_img / bf_color_flow_img comments, the x86 double -> uchar conversion, and the hue / saturation of a flow
 * vector (EventFile::color_flow_img, event_file.h:330-338).  C++ only; no state.
 */
#ifndef BF_FLOW_COLOR_H
#define BF_FLOW_COLOR_H

#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD inline
#endif

BF_HD uint8_t bf_unit_to_u8(float x) {
    const float v = x * 255.0f;
    return (uint8_t)(v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)rintf(v)));
}

// HSV (H in [0, 180), S, V in [0, 255]) -> B, G, R; float32, no contraction.
BF_HD void bf_hsv_to_bgr_u8(int H, int S, int V, uint8_t* bgr) {
    const float s = (float)S * (1.0f / 255.0f), v = (float)V * (1.0f / 255.0f);
    float h = (float)H * (6.0f / 180.0f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    sector = ((sector % 6) + 6) % 6;
    float tab[4];
    tab[0] = v;
    tab[1] = v * (1.0f - s);
    tab[2] = v * (1.0f - s * h);
    tab[3] = v * (1.0f - s * (1.0f - h));
    int ib, ig, ir;
    switch (sector) {
        case 0: ib = 1; ig = 3; ir = 0; break;
        case 1: ib = 1; ig = 0; ir = 2; break;
        case 2: ib = 3; ig = 0; ir = 1; break;
        case 3: ib = 0; ig = 2; ir = 1; break;
        case 4: ib = 0; ig = 1; ir = 3; break;
        default: ib = 2; ig = 1; ir = 0; break;
    }
    float b = tab[0], gg = tab[0], r = tab[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k < 4; ++k) {
        b = ib == k ? tab[k] : b;
        gg = ig == k ? tab[k] : gg;
        r = ir == k ? tab[k] : r;
    }
    bgr[0] = bf_unit_to_u8(b); bgr[1] = bf_unit_to_u8(gg); bgr[2] = bf_unit_to_u8(r);
}

// `uchar c = <double>` as the reference's x86-64 build does it: cvttsd2si to int32 (NaN and anything outside the int32
// range give INT_MIN), then the low byte.  -3.0 -> 253, -inf -> 0, NaN -> 0, 300.0 -> 44.
// (`int x = <double>` is cvttsd2si there; csrc/bf_device_fns.h's trunc_x86 is this function)
BF_HD int bf_double_to_int_x86(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }
BF_HD int bf_double_to_uchar_x86(double v) { return (int)(unsigned char)bf_double_to_int_x86(v); }

// The hue and saturation bytes EventFile::color_flow_img stores for a flow vector (u, v) (event_file.h:330-338), all in
// double: speed = hypot(u, v); angle = speed != 0 ? (atan2(v, u) + 3.1416) * 180 / 3.1416 : 0; log_spd = std::min(255.0,
// log(speed) / log(1.025)) -- std::min(a, b) is `b < a ? b : a`, so a NaN quotient gives 255 --; H = uchar(angle / 2),
// S = uchar(log_spd).  log(1.025) is the double 0.024692612590371414 (0x1.949052e1d202ep-6).
BF_HD void bf_flow_hs(double u, double v, int* H, int* S) {
    const double speed = hypot(u, v);
    double angle = 0;
    if (speed != 0) angle = (atan2(v, u) + 3.1416) * 180 / 3.1416;
    const double q = log(speed) / 0.024692612590371414;
    const double log_spd = q < 255.0 ? q : 255.0;
    *H = bf_double_to_uchar_x86(angle / 2);
    *S = bf_double_to_uchar_x86(log_spd);
}

#endif /* BF_FLOW_COLOR_H */
