// Per-face table arithmetic shared by the device kernels (face_tables.hip) and a host harness (tests/face_tables_harness.cpp): the
// enlarged square ROI and rounded crop box of get_all_outputs (reference synergy3DMM.py:178-185, utils/inference.py:98) for FLOAT32
// detections, and the Lanczos-4 tap table of one destination index (synergynet_amd/inference.py _lanczos4_taps).  Every function
// restates the host arithmetic with the same rounding points and the same order of operations, so the integers are the same; that
// needs floating-point contraction OFF (hipcc contracts by default: an FMA in (dx + 0.5) * scale - 0.5 moves `pos`), which the
// pragma at the head of each function does for this code alone.  Plain C++: compiles with or without HIP.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FT_HD __host__ __device__
#else
#define FT_HD
#endif

namespace syn {

constexpr int kFtDst = 120;         // destination side of the crop resize (utils/params.py:34)

// status bits of ft_roi_box: where the host path raises ValueError('degenerate detection box')
enum { FT_NONFINITE = 1, FT_TOO_LARGE = 2, FT_EMPTY = 4 };

// One destination index dx of the resize side -> 120: first source tap (crop coordinates, may lie outside: the crop kernel clamps)
// and the eight 11-bit fixed-point weights.  side >= 1.
FT_HD inline void ft_lanczos4_tap(int side, int dx, int *ofs, int16_t *coef /*[8]*/) {
#pragma clang fp contract(off)
    const double scale = (double)side / 120.0;
    const float pos = (float)(((double)dx + 0.5) * scale - 0.5);
    const float fl = floorf(pos);
    const float fx = pos - fl;                      // exact in float32, < 1
    *ofs = (int)fl - 3;
    if (fx < FLT_EPSILON) {                         // the source position IS a sample: weight 1 on tap 3
        for (int i = 0; i < 8; ++i) coef[i] = 0;
        coef[3] = 2048;
        return;
    }
    const double s45 = 0.70710678118654752440084436210485, pi = 3.141592653589793;
    const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const float x3 = fx + 3.0f;
    const double y0 = -(double)x3 * pi * 0.25;
    const double s0 = sin(y0), c0 = cos(y0);
    float c[8];
    float tot = 0.f;
    for (int i = 0; i < 8; ++i) {
        const double y = -(double)(x3 - (float)i) * pi * 0.25;
        c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        tot = tot + c[i];                           // sequential float32 sum, tap 0 first
    }
    const float inv = 1.0f / tot;
    for (int i = 0; i < 8; ++i) {
        float v = rintf((c[i] * inv) * 2048.0f);
        v = v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v);
        coef[i] = (int16_t)v;
    }
}

// One float32 detection (x1, y1, x2, y2, score) -> roi (sx, sy, ex, ey, score) in float32, box = rint(roi[0:4]) and the crop sides.
// Returns 0, or the FT_* bits of a degenerate face: then box = (0, 0, 1, 1) and both sides are 1 (roi keeps its float values).
FT_HD inline int ft_roi_box(const float *det, float *roi /*[5]*/, int *box /*[4]*/, int *w, int *h) {
#pragma clang fp contract(off)
    const float x1 = det[0], y1 = det[1], x2 = det[2], y2 = det[3];
    const float hc = (y1 + y2) / 2.0f;
    const float wc = (x1 + x2) / 2.0f;
    const float margin = floorf(((y2 - y1) * 1.2f) * 0.5f);      // 1.2f: a double 1.2 moves the margin by one for some heights
    roi[0] = wc - margin;
    roi[1] = hc - margin;
    roi[2] = wc + margin;
    roi[3] = hc + margin;
    roi[4] = det[4];
    int status = 0;
    float b[4];
    for (int i = 0; i < 4; ++i) {
        b[i] = rintf(roi[i]);                                    // ties to even, like round() and numpy's rint
        if (!(fabsf(b[i]) <= FLT_MAX)) status |= FT_NONFINITE;   // inf or NaN
        else if (fabsf(b[i]) > 1073741824.0f) status |= FT_TOO_LARGE;
    }
    if (!status) {
        const long long ww = (long long)b[2] - (long long)b[0], hh = (long long)b[3] - (long long)b[1];
        if (ww <= 0 || hh <= 0 || ww > 2147483647ll || hh > 2147483647ll) status |= FT_EMPTY;
        else {
            for (int i = 0; i < 4; ++i) box[i] = (int)b[i];
            *w = (int)ww;
            *h = (int)hh;
        }
    }
    if (status) {
        box[0] = 0; box[1] = 0; box[2] = 1; box[3] = 1;
        *w = 1;
        *h = 1;
    }
    return status;
}

}  // namespace syn
