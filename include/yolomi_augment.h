/* Per-pixel arithmetic of ym_augment_u8 (include/yolomi.h), usable from the HIP kernel and from a plain
 * C++ host program: ym_aug_sample(entry, x, y) -> the 8-bit value of output pixel (x, y).  The kernel in
 * csrc/preprocess.hip is a loop around its pieces; tests/augment_host.cpp runs the same function on the CPU, where
 * every source index it forms can be checked.
 *
 * Formats:
 *   positions     int64, YM_AUG_FB = 24 fraction bits.  The 2x3 maps are rounded once on the host from fp64;
 *                 pos = m0 * x + m1 * y + m2 is formed modulo 2^64 (no signed overflow for any table; inside
 *                 the documented coefficient bounds nothing wraps).
 *   weights       the position is rounded to 11 fraction bits (half up): s = floor, a1 = fraction * 2048,
 *                 a0 = 2048 - a1.  s < 0 -> (0, a1 = 0); s >= n - 1 -> (n - 1, a1 = 0); second tap min(s + 1, n - 1):
 *                 taps never leave the source image.
 *   interpolation OpenCV's 8-bit resize: h(r) = p[r][s] * a0 + p[r][s1] * a1;
 *                 v = (((b0 * (h(t) >> 4)) >> 16) + ((b1 * (h(t1) >> 4)) >> 16) + 2) >> 2 clamped to 0..255.
 *                 Integer positions return the source byte; a constant image stays constant.
 *   gain          min((v * gain) >> 16, 255), gain Q16 clamped to [0, 2^23]: truncation and saturation, a
 *                 value LUT.
 * YM_AUG_STRETCH entries take (s, a0, a1) from ym_aug_lin_coeff, the float coefficient rule of OpenCV's resize
 * that ym_resize_linear_u8 uses, so they equal that kernel bit for bit. */
#ifndef YOLOMI_AUGMENT_H
#define YOLOMI_AUGMENT_H

#include <math.h>
#include <stdint.h>

#include "yolomi.h"

#if defined(__HIPCC__)
#define YM_HD __host__ __device__
#else
#define YM_HD
#endif

static_assert(sizeof(ym_aug_tile) == 88 && sizeof(ym_aug_entry) == 432, "ym_aug_entry layout (yolomi/_lib.py)");

/* OpenCV resizeGeneric_ coefficients of output index d (see csrc/preprocess.hip) */
YM_HD static inline void ym_aug_lin_coeff(int d, double scale, int n, int& s, int& a0, int& a1) {
    float f = float((d + 0.5) * scale - 0.5);
    int si = int(floorf(f));
    f -= float(si);
    if (si < 0) { f = 0.f; si = 0; }
    if (si >= n - 1) { f = 0.f; si = n - 1; }
    s = si;
    a0 = int(rintf((1.f - f) * 2048.f));        /* round half to even */
    a1 = int(rintf(f * 2048.f));
}

YM_HD static inline int64_t ym_aug_map(const int64_t* m, int x, int y) {
    return int64_t(uint64_t(m[0]) * uint64_t(int64_t(x)) + uint64_t(m[1]) * uint64_t(int64_t(y)) + uint64_t(m[2]));
}

/* fixed-point position -> tap index and 11-bit weights inside [0, n) */
YM_HD static inline void ym_aug_fix_coeff(int64_t pos, int n, int& s, int& a0, int& a1) {
    const int sh = YM_AUG_FB - 11;
    const int64_t q = (pos >> sh) + ((pos >> (sh - 1)) & 1);     /* round half up; never overflows */
    int64_t si = q >> 11;
    int f = int(q & 2047);
    if (si < 0) { f = 0; si = 0; }
    if (si >= int64_t(n) - 1) { f = 0; si = int64_t(n) - 1; }
    s = int(si);
    a0 = 2048 - f;
    a1 = f;
}

YM_HD static inline int ym_aug_blend(const uint8_t* im, int h0, int w0, int sx, int a0, int a1, int sy, int b0,
                                     int b1) {
    const int sx1 = sx + 1 < w0 ? sx + 1 : w0 - 1, sy1 = sy + 1 < h0 ? sy + 1 : h0 - 1;
    const uint8_t* r0 = im + int64_t(sy) * w0;
    const uint8_t* r1 = im + int64_t(sy1) * w0;
    const int h0v = int(r0[sx]) * a0 + int(r0[sx1]) * a1;
    const int h1v = int(r1[sx]) * a0 + int(r1[sx1]) * a1;
    int v = (((b0 * (h0v >> 4)) >> 16) + ((b1 * (h1v >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* the pieces of ym_aug_sample; the kernel calls them one by one so that a wave whose pixels all fall into one
 * slot can address the tile through scalar registers */

/* YM_AUG_STRETCH entries: ym_resize_linear_u8's value of tile[0].src (before the gain) */
YM_HD static inline int ym_aug_stretch_value(const uint8_t* src, const int64_t* meta, int batch, int S,
                                             const ym_aug_entry* e, int x, int y) {
    const int b = e->tile[0].src;
    if (b < 0 || b >= batch) return e->fill & 255;
    const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
    if (h0 <= 0 || w0 <= 0) return e->fill & 255;
    int sx, a0, a1, sy, b0, b1;
    ym_aug_lin_coeff(x, double(w0) / S, w0, sx, a0, a1);
    ym_aug_lin_coeff(y, double(h0) / S, h0, sy, b0, b1);
    return ym_aug_blend(src + meta[3 * b], h0, w0, sx, a0, a1, sy, b0, b1);
}

/* canvas position of output pixel (x, y) and the slot (quadrant) it falls into */
YM_HD static inline int ym_aug_slot(const ym_aug_entry* e, int x, int y, int64_t& cx, int64_t& cy) {
    cx = ym_aug_map(e->c, x, y);
    cy = ym_aug_map(e->c + 3, x, y);
    return (cx >= e->xc ? 1 : 0) + (cy >= e->yc ? 2 : 0);
}

/* value (before the gain) of output pixel (x, y) at canvas position (cx, cy) in the slot of tile `t` */
YM_HD static inline int ym_aug_tile_value(const uint8_t* src, const int64_t* meta, int batch, int fill,
                                          const ym_aug_tile* t, int64_t cx, int64_t cy, int x, int y) {
    const int b = t->src;
    if (b < 0 || b >= batch || cx < t->x0 || cx >= t->x1 || cy < t->y0 || cy >= t->y1) return fill & 255;
    const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
    if (h0 <= 0 || w0 <= 0) return fill & 255;
    int sx, a0, a1, sy, b0, b1;
    ym_aug_fix_coeff(ym_aug_map(t->m, x, y), w0, sx, a0, a1);
    ym_aug_fix_coeff(ym_aug_map(t->m + 3, x, y), h0, sy, b0, b1);
    return ym_aug_blend(src + meta[3 * b], h0, w0, sx, a0, a1, sy, b0, b1);
}

YM_HD static inline int ym_aug_gain(int gain, int v) {
    int64_t g = gain;
    g = g < 0 ? 0 : (g > (int64_t(1) << 23) ? (int64_t(1) << 23) : g);
    const int64_t w = (int64_t(v) * g) >> 16;
    return int(w > 255 ? 255 : w);
}

/* value of output pixel (x, y), 0 <= x, y < S, of the image `e` describes; src / meta as for ym_resize_linear_u8 */
YM_HD static inline int ym_aug_sample(const uint8_t* src, const int64_t* meta, int batch, int S,
                                      const ym_aug_entry* e, int x, int y) {
    if (e->flags & YM_AUG_STRETCH) return ym_aug_gain(e->gain, ym_aug_stretch_value(src, meta, batch, S, e, x, y));
    int64_t cx, cy;
    const int slot = ym_aug_slot(e, x, y, cx, cy);
    return ym_aug_gain(e->gain, ym_aug_tile_value(src, meta, batch, e->fill, &e->tile[slot], cx, cy, x, y));
}

#endif
