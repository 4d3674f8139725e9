// cv2.resize(INTER_LINEAR) on uint8, per output sample, as OpenCV's fixed-point generic
// path computes it (11-bit weights, 128-bit vector vertical pass + scalar tail -- the same
// restatement as oracle/csrc/oracle.c).  Shared by the ViT patch preprocessing
// (vit_ops.hip k_preprocess_patches) and MixVPR's 320 x 320 preprocessing (mixvpr.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ int16_t sat16(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

__device__ __forceinline__ void axis_lookup(int d, int ssize, int dsize, bool clamp, int& s0, int& s1, int& w0,
                                            int& w1) {
    const double scale = 1.0 / ((double)dsize / ssize);
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    }
    w0 = sat16((int)__builtin_rintf((1.f - f) * 2048.f));
    w1 = sat16((int)__builtin_rintf(f * 2048.f));
    s0 = min(max(s, 0), ssize - 1);
    s1 = min(max(s + 1, 0), ssize - 1);
}

// first element of a resized row (S * C interleaved elements) the vertical pass handles
// with its scalar tail
__device__ __forceinline__ int resize_vec_end(int wb) {
    int x = 0;
    if (wb >= 16) x = ((wb - 16) / 16 + 1) * 16;
    while (x < wb - 8) x += 8;
    return x;
}

// Source channel sc of output pixel (y, x) of the S x S resize of src [H, W, C];
// vend = resize_vec_end(S * C).  Returns the uint8 value.
__device__ __forceinline__ int resize_cv_sample(const uint8_t* src, int H, int W, int C, int S, int y, int x, int sc,
                                                int vend) {
    int sx0, sx1, ax0, ax1, sy0, sy1, by0, by1;
    axis_lookup(x, W, S, true, sx0, sx1, ax0, ax1);
    axis_lookup(y, H, S, false, sy0, sy1, by0, by1);
    const uint8_t* r0 = src + (size_t)sy0 * W * C;
    const uint8_t* r1 = src + (size_t)sy1 * W * C;
    const int h0 = r0[sx0 * C + sc] * ax0 + r0[sx1 * C + sc] * ax1;
    const int h1 = r1[sx0 * C + sc] * ax0 + r1[sx1 * C + sc] * ax1;
    int q;
    if (x * C + sc < vend) {  // universal-intrinsic vertical pass
        const int a0 = sat16(h0 >> 4), a1 = sat16(h1 >> 4);
        int t = (int16_t)(((a0 * by0) >> 16) + ((a1 * by1) >> 16));
        q = (t + 2) >> 2;
    } else {  // scalar tail
        q = (h0 * by0 + h1 * by1 + (1 << 21)) >> 22;
    }
    return min(max(q, 0), 255);
}

// ImageNet normalisation of a uint8 level: float32 u / 255, then float64 (x - mean) / std
__device__ __forceinline__ float imagenet_norm(int c, int u) {
    const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406);
    const double std = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
    const float x = (float)u / 255.0f;
    return (float)(((double)x - mean) / std);
}
