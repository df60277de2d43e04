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
static_assert(sizeof(ym_lb_entry) == 32, "ym_lb_entry layout (yolomi/_lib.py)");
static_assert(sizeof(ym_tile_entry) == 48, "ym_tile_entry layout (yolomi/_lib.py)");

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

/* ---------------------------------------------------------------- 1-4 planes (ym_resize_linear_u8c, ym_augment_u8c)
 * The source is pixel-interleaved (h0, w0, ch).  Everything above that does not touch a source byte (slot, tile
 * and rectangle test, tap indices, weights, fill) is formed once per output pixel into ym_aug_taps; every plane is
 * then ym_aug_blend's arithmetic on bytes `ch` apart, and goes through ym_aug_gain.  With ch == 1 the values are
 * ym_aug_sample's.
 *
 * Hue and saturation (ch == 3, between sampling and the gain) work on the HSV hexcone in integers and keep V:
 *   V = max, m = min, d = V - m; d == 0 leaves the pixel alone
 *   H6 in [0, 6d) the position on the hexcone (sector * d + offset, red first, then green)
 *   H6' = (H6 + ((hue * 6d + 32768) >> 16)) % 6d     hue Q16 fraction of a turn, & 65535: a shift
 *   d'  = min((d * sat) >> 16, V)                    sat Q16, clamped to [0, 2^17]
 *   k = H6' / d, f = H6' - k d, f' = (2 f d' + d) / (2d), m' = V - d'; the sector k places V, m' and m' + f' or V - f'
 * hue = 0, sat = 65536 returns the input bytes.  Against the real-valued hexcone the error is at most 2.5 levels for
 * sat <= 2: 0.5 from the rounded shift scaled by d'/d <= 2, 1 from the truncation of d', 0.5 from f'. */
typedef struct ym_aug_taps {
    const uint8_t* r0;         /* plane 0 of the first pixel of rows sy and min(sy + 1, h0 - 1) */
    const uint8_t* r1;
    int64_t o0, o1;            /* byte offsets of columns sx and min(sx + 1, w0 - 1) in a row */
    int a0, a1, b0, b1;
} ym_aug_taps;

YM_HD static inline void ym_aug_set_taps(const uint8_t* im, int h0, int w0, int ch, int sx, int a0, int a1, int sy,
                                         int b0, int b1, ym_aug_taps& t) {
    const int sx1 = sx + 1 < w0 ? sx + 1 : w0 - 1, sy1 = sy + 1 < h0 ? sy + 1 : h0 - 1;
    const int64_t row = int64_t(w0) * ch;
    t.r0 = im + int64_t(sy) * row;
    t.r1 = im + int64_t(sy1) * row;
    t.o0 = int64_t(sx) * ch;
    t.o1 = int64_t(sx1) * ch;
    t.a0 = a0, t.a1 = a1, t.b0 = b0, t.b1 = b1;
}

/* ym_aug_blend at the taps `t`, plane c */
YM_HD static inline int ym_aug_taps_value(const ym_aug_taps& t, int c) {
    const int h0v = int(t.r0[t.o0 + c]) * t.a0 + int(t.r0[t.o1 + c]) * t.a1;
    const int h1v = int(t.r1[t.o0 + c]) * t.a0 + int(t.r1[t.o1 + c]) * t.a1;
    int v = (((t.b0 * (h0v >> 4)) >> 16) + ((t.b1 * (h1v >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* taps of ym_resize_linear_u8's rule for output pixel (x, y) of the h0 x w0 image at `im` */
YM_HD static inline void ym_aug_lin_taps(const uint8_t* im, int h0, int w0, int ch, int S, int x, int y,
                                         ym_aug_taps& t) {
    int sx, a0, a1, sy, b0, b1;
    ym_aug_lin_coeff(x, double(w0) / S, w0, sx, a0, a1);
    ym_aug_lin_coeff(y, double(h0) / S, h0, sy, b0, b1);
    ym_aug_set_taps(im, h0, w0, ch, sx, a0, a1, sy, b0, b1, t);
}

/* the same for a resize to nw x nh (ym_letterbox_u8c): (x, y) is the pixel of the resized image, 0 <= x < nw,
 * 0 <= y < nh */
YM_HD static inline void ym_aug_lin_taps_wh(const uint8_t* im, int h0, int w0, int ch, int nw, int nh, int x, int y,
                                            ym_aug_taps& t) {
    int sx, a0, a1, sy, b0, b1;
    ym_aug_lin_coeff(x, double(w0) / nw, w0, sx, a0, a1);
    ym_aug_lin_coeff(y, double(h0) / nh, h0, sy, b0, b1);
    ym_aug_set_taps(im, h0, w0, ch, sx, a0, a1, sy, b0, b1, t);
}

/* ym_letterbox_u8c: the `ch` values v[0..ch) of frame pixel (x, y) of image b (`e` its table entry) */
YM_HD static inline void ym_lb_sample_c(const uint8_t* src, const int64_t* meta, int b, int ch, const ym_lb_entry* e,
                                        int fill, int x, int y, int* v) {
    const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
    const bool empty = e->nw <= 0 || e->nh <= 0 || h0 <= 0 || w0 <= 0 || e->h0 != h0 || e->w0 != w0;
    const int64_t u = int64_t(x) - e->left, w = int64_t(y) - e->top;
    if (empty || u < 0 || u >= e->nw || w < 0 || w >= e->nh) {
        for (int c = 0; c < ch; ++c) v[c] = fill & 255;
        return;
    }
    const uint8_t* im = src + meta[3 * b];
    if (e->nw == w0 && e->nh == h0) {
        for (int c = 0; c < ch; ++c) v[c] = im[(w * w0 + u) * ch + c];
        return;
    }
    ym_aug_taps t;
    ym_aug_lin_taps_wh(im, h0, w0, ch, e->nw, e->nh, int(u), int(w), t);
    for (int c = 0; c < ch; ++c) v[c] = ym_aug_taps_value(t, c);
}

/* ---------------------------------------------------------------- tiles (ym_slice_letterbox_u8c)
 * A tile is a tw x th window of a wider image: its rows lie `pitch` bytes apart, and everything else is the
 * letterbox of a stand-alone tw x th image, so the second taps clamp at the window's last column and row.
 * YM_TILE_MIRROR_X / _Y (yolomi.h) reverse the columns / rows of the rendered nw x nh rectangle. */

/* ym_aug_set_taps for the th x tw window at `win` whose rows are `pitch` bytes apart */
YM_HD static inline void ym_aug_set_taps_pitch(const uint8_t* win, int th, int tw, int ch, int64_t pitch, int sx,
                                               int a0, int a1, int sy, int b0, int b1, ym_aug_taps& t) {
    const int sx1 = sx + 1 < tw ? sx + 1 : tw - 1, sy1 = sy + 1 < th ? sy + 1 : th - 1;
    t.r0 = win + int64_t(sy) * pitch;
    t.r1 = win + int64_t(sy1) * pitch;
    t.o0 = int64_t(sx) * ch;
    t.o1 = int64_t(sx1) * ch;
    t.a0 = a0, t.a1 = a1, t.b0 = b0, t.b1 = b1;
}

/* true: the entry names an image of `meta` and a window with pixels that lies inside it; false: the tile is fill */
YM_HD static inline bool ym_tile_valid(const int64_t* meta, int n_images, const ym_tile_entry* e) {
    if (e->src < 0 || e->src >= n_images || e->tw <= 0 || e->th <= 0 || e->nw <= 0 || e->nh <= 0) return false;
    const int64_t h0 = meta[3 * int64_t(e->src) + 1], w0 = meta[3 * int64_t(e->src) + 2];
    return e->x0 >= 0 && e->y0 >= 0 && int64_t(e->x0) + e->tw <= w0 && int64_t(e->y0) + e->th <= h0;
}

/* ym_slice_letterbox_u8c: the `ch` values v[0..ch) of frame pixel (x, y) of the tile `e` describes */
YM_HD static inline void ym_tile_sample_c(const uint8_t* src, const int64_t* meta, int n_images, int ch,
                                          const ym_tile_entry* e, int fill, int x, int y, int* v) {
    int64_t u = int64_t(x) - e->left, w = int64_t(y) - e->top;
    if (!ym_tile_valid(meta, n_images, e) || u < 0 || u >= e->nw || w < 0 || w >= e->nh) {
        for (int c = 0; c < ch; ++c) v[c] = fill & 255;
        return;
    }
    /* mirrored views: only the column / row index that feeds the copy and the coefficients is reflected */
    if (e->edges & YM_TILE_MIRROR_X) u = int64_t(e->nw) - 1 - u;
    if (e->edges & YM_TILE_MIRROR_Y) w = int64_t(e->nh) - 1 - w;
    const int64_t pitch = meta[3 * int64_t(e->src) + 2] * ch;
    const uint8_t* win = src + meta[3 * int64_t(e->src)] + e->y0 * pitch + int64_t(e->x0) * ch;
    if (e->nw == e->tw && e->nh == e->th) {
        for (int c = 0; c < ch; ++c) v[c] = win[w * pitch + u * ch + c];
        return;
    }
    int sx, a0, a1, sy, b0, b1;
    ym_aug_lin_coeff(int(u), double(e->tw) / e->nw, e->tw, sx, a0, a1);
    ym_aug_lin_coeff(int(w), double(e->th) / e->nh, e->th, sy, b0, b1);
    ym_aug_taps t;
    ym_aug_set_taps_pitch(win, e->th, e->tw, ch, pitch, sx, a0, a1, sy, b0, b1, t);
    for (int c = 0; c < ch; ++c) v[c] = ym_aug_taps_value(t, c);
}

/* ym_aug_stretch_value's geometry; false: the pixel shows the fill */
YM_HD static inline bool ym_aug_stretch_taps(const uint8_t* src, const int64_t* meta, int batch, int ch, int S,
                                             const ym_aug_entry* e, int x, int y, ym_aug_taps& t) {
    const int b = e->tile[0].src;
    if (b < 0 || b >= batch) return false;
    const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
    if (h0 <= 0 || w0 <= 0) return false;
    ym_aug_lin_taps(src + meta[3 * b], h0, w0, ch, S, x, y, t);
    return true;
}

/* ym_aug_tile_value's geometry; false: the pixel shows the fill */
YM_HD static inline bool ym_aug_tile_taps(const uint8_t* src, const int64_t* meta, int batch, int ch,
                                          const ym_aug_tile* tl, int64_t cx, int64_t cy, int x, int y,
                                          ym_aug_taps& t) {
    const int b = tl->src;
    if (b < 0 || b >= batch || cx < tl->x0 || cx >= tl->x1 || cy < tl->y0 || cy >= tl->y1) return false;
    const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
    if (h0 <= 0 || w0 <= 0) return false;
    int sx, a0, a1, sy, b0, b1;
    ym_aug_fix_coeff(ym_aug_map(tl->m, x, y), w0, sx, a0, a1);
    ym_aug_fix_coeff(ym_aug_map(tl->m + 3, x, y), h0, sy, b0, b1);
    ym_aug_set_taps(src + meta[3 * b], h0, w0, ch, sx, a0, a1, sy, b0, b1, t);
    return true;
}

/* hue shift and saturation factor on 8-bit (r, g, b) = v[0..2], V kept (the rule is stated above) */
YM_HD static inline void ym_aug_hue_sat(int hue, int sat, int* v) {
    const int r = v[0], g = v[1], b = v[2];
    const int V = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int m = r < g ? (r < b ? r : b) : (g < b ? g : b);
    const int d = V - m;
    if (d == 0) return;
    int H6;
    if (V == r) H6 = g >= b ? g - b : 5 * d + (r - b);
    else if (V == g) H6 = b >= r ? 2 * d + (b - r) : d + (g - r);
    else H6 = r >= g ? 4 * d + (r - g) : 3 * d + (b - g);
    H6 = (H6 + (((hue & 65535) * 6 * d + 32768) >> 16)) % (6 * d);
    sat = sat < 0 ? 0 : (sat > (1 << 17) ? (1 << 17) : sat);
    int d1 = (d * sat) >> 16;
    d1 = d1 < V ? d1 : V;
    const int k = H6 / d, f = H6 - k * d;
    const int f1 = (2 * f * d1 + d) / (2 * d), m1 = V - d1;
    const int up = m1 + f1, dn = V - f1;
    switch (k) {
        case 0: v[0] = V, v[1] = up, v[2] = m1; break;
        case 1: v[0] = dn, v[1] = V, v[2] = m1; break;
        case 2: v[0] = m1, v[1] = V, v[2] = up; break;
        case 3: v[0] = m1, v[1] = dn, v[2] = V; break;
        case 4: v[0] = up, v[1] = m1, v[2] = V; break;
        default: v[0] = V, v[1] = m1, v[2] = dn; break;
    }
}

/* the `ch` planes of a pixel whose geometry is known (`hit` false: fill): blend, hue / sat (`col` may be null;
 * ch == 3 only), gain */
YM_HD static inline void ym_aug_planes(const ym_aug_entry* e, const ym_aug_colour* col, int ch, bool hit,
                                       const ym_aug_taps& t, int* v) {
    for (int c = 0; c < ch; ++c) v[c] = hit ? ym_aug_taps_value(t, c) : (e->fill & 255);
    if (col && ch == 3) ym_aug_hue_sat(col->hue, col->sat, v);
    for (int c = 0; c < ch; ++c) v[c] = ym_aug_gain(e->gain, v[c]);
}

/* the `ch` values v[0..ch) of output pixel (x, y) of the image `e` describes; src / meta as for ym_augment_u8c */
YM_HD static inline void ym_aug_sample_c(const uint8_t* src, const int64_t* meta, int batch, int ch, int S,
                                         const ym_aug_entry* e, const ym_aug_colour* col, int x, int y, int* v) {
    ym_aug_taps t = {};
    bool hit;
    if (e->flags & YM_AUG_STRETCH) {
        hit = ym_aug_stretch_taps(src, meta, batch, ch, S, e, x, y, t);
    } else {
        int64_t cx, cy;
        const int slot = ym_aug_slot(e, x, y, cx, cy);
        hit = ym_aug_tile_taps(src, meta, batch, ch, &e->tile[slot], cx, cy, x, y, t);
    }
    ym_aug_planes(e, col, ch, hit, t, v);
}

/* ---------------------------------------------------------------- MixUp (ym_augment_mix_u8c)
 * A mixed image is two entries sampled at the same output pixel, the primary's a[c] and the partner's p[c], both
 * before hue / sat and gain, blended in integers:
 *   v[c] = (a[c] * r + p[c] * (65536 - r)) >> 16      r Q16, clamped to [0, 65536]; at most 255 * 65536, an int32
 * a == p returns a; r = 65536 returns a and r = 0 returns p; v lies between the two and is the real-valued blend
 * truncated (0 <= real - v < 1), as Ultralytics' (a * r + b * (1 - r)).astype(uint8).  Hue / sat (the image's colour
 * entry) and the gain follow on the blended planes, as Ultralytics applies HSV after MixUp; the gain is the PRIMARY
 * entry's and the partner entry's `gain` is ignored.  An image without a partner is ym_aug_sample_c bit for bit. */
static_assert(sizeof(ym_aug_mix) == 8, "ym_aug_mix layout (yolomi/_lib.py)");

/* ym_aug_sample_c's geometry for either kind of entry; false: the pixel shows the fill */
YM_HD static inline bool ym_aug_entry_taps(const uint8_t* src, const int64_t* meta, int batch, int ch, int S,
                                           const ym_aug_entry* e, int x, int y, ym_aug_taps& t) {
    if (e->flags & YM_AUG_STRETCH) return ym_aug_stretch_taps(src, meta, batch, ch, S, e, x, y, t);
    int64_t cx, cy;
    const int slot = ym_aug_slot(e, x, y, cx, cy);
    return ym_aug_tile_taps(src, meta, batch, ch, &e->tile[slot], cx, cy, x, y, t);
}

/* the `ch` planes of a pixel before hue / sat and gain: the tap blend, or the entry's fill */
YM_HD static inline void ym_aug_raw_planes(const ym_aug_entry* e, int ch, bool hit, const ym_aug_taps& t, int* v) {
    for (int c = 0; c < ch; ++c) v[c] = hit ? ym_aug_taps_value(t, c) : (e->fill & 255);
}

YM_HD static inline int ym_aug_mix_ratio(int r) { return r < 0 ? 0 : (r > 65536 ? 65536 : r); }

/* a, p in 0..255, r = ym_aug_mix_ratio(.) */
YM_HD static inline int ym_aug_mix_blend(int a, int p, int r) { return (a * r + p * (65536 - r)) >> 16; }

/* true: `mix` names an entry of the partner table; false: the image is not mixed and that table is not read */
YM_HD static inline bool ym_aug_mix_valid(const ym_aug_mix* mix, int n_partner) {
    return mix && mix->partner >= 0 && mix->partner < n_partner;
}

/* blended planes `a` (in: the primary's raw planes) and `p` (the partner's) -> a: blend, hue / sat, primary gain */
YM_HD static inline void ym_aug_mix_planes(const ym_aug_entry* e, const ym_aug_colour* col, int ch, int ratio,
                                           const int* p, int* a) {
    const int r = ym_aug_mix_ratio(ratio);
    for (int c = 0; c < ch; ++c) a[c] = ym_aug_mix_blend(a[c], p[c], r);
    if (col && ch == 3) ym_aug_hue_sat(col->hue, col->sat, a);
    for (int c = 0; c < ch; ++c) a[c] = ym_aug_gain(e->gain, a[c]);
}

/* the `ch` values v[0..ch) of output pixel (x, y) of the image whose primary entry is `e`, mix record `mix` (may be
 * null) and colour entry `col` (may be null); `partner` is the compact table of n_partner second entries */
YM_HD static inline void ym_aug_mix_sample_c(const uint8_t* src, const int64_t* meta, int batch, int ch, int S,
                                             const ym_aug_entry* e, const ym_aug_mix* mix,
                                             const ym_aug_entry* partner, int n_partner, const ym_aug_colour* col,
                                             int x, int y, int* v) {
    if (!ym_aug_mix_valid(mix, n_partner)) {
        ym_aug_sample_c(src, meta, batch, ch, S, e, col, x, y, v);
        return;
    }
    const ym_aug_entry* pe = partner + mix->partner;
    ym_aug_taps t = {};
    int w[4];
    bool hit = ym_aug_entry_taps(src, meta, batch, ch, S, e, x, y, t);
    ym_aug_raw_planes(e, ch, hit, t, v);
    hit = ym_aug_entry_taps(src, meta, batch, ch, S, pe, x, y, t);
    ym_aug_raw_planes(pe, ch, hit, t, w);
    ym_aug_mix_planes(e, col, ch, mix->ratio, w, v);
}

#endif
