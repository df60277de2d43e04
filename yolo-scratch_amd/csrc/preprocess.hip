// Image preprocessing for the crater data path (gfx950): stretch-resize of grayscale uint8
// images to S x S with OpenCV's fixed-point INTER_LINEAR arithmetic, then /255 to fp32 NCHW.
//
// Replaces cv2.resize(im, (S, S), interpolation=cv2.INTER_LINEAR) + astype(float32) / 255 in the
// reference loader (/root/reference/yolo_scratch_cuda/datasets/crater_dataset_cuda.py:182-184,
// 253).  The reference does it per image on the CPU in DataLoader workers; here the workers only
// decode, the raw uint8 bytes cross PCIe (1/4 of the fp32 tensor) and one launch resizes the batch.
//
// Arithmetic (OpenCV resizeGeneric_, fixed-point 8U path, INTER_RESIZE_COEF_BITS = 11):
//   fx = float((dx + 0.5) * (W0 / S) - 0.5) in double, sx = floor(fx), fx -= sx;
//   sx < 0 -> (sx, fx) = (0, 0);  sx >= W0 - 1 -> (sx, fx) = (W0 - 1, 0);
//   a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048)  (saturate_cast<short>: round half to even)
//   h(r) = src[r][sx] * a0 + src[r][min(sx + 1, W0 - 1)] * a1            (the same for rows)
//   out = ((b0 * (h(sy) >> 4)) >> 16) + ((b1 * (h(sy1) >> 4)) >> 16) + 2) >> 2, clamped to 0..255
//        (the vertical rounding of OpenCV's SIMD path, which covers every column when S % 16 == 0)
// Images already S x S are copied unchanged (the reference skips the resize there, :183).
// The coefficient rule (ym_aug_lin_coeff) lives in include/yolomi_augment.h, shared with the augmentation.
//
// Training augmentation (ym_augment_u8): the same launch shape with a per-image table entry (ym_aug_entry,
// include/yolomi.h) of up to four mosaic tiles, each with its own 2x3 output-pixel -> source-position map, a
// fill byte and a value gain.  The arithmetic is all integer and lives in include/yolomi_augment.h
// (ym_aug_sample; the formats are stated in that file's header): int64 positions with 24 fraction bits, rounded
// to 11-bit weights, taps clamped to the source image, the interpolation above, gain in Q16.  The kernel below is
// a loop around that function's pieces: blockIdx.y walks images, so the table entry is block-uniform (scalar loads);
// each thread produces four consecutive pixels of the flat S * S image and writes them with one 16-byte store
// (lanes of a wave cover 1 KiB of contiguous output); blockIdx.x grid-strides over the image.
//
// Letterbox (ym_letterbox_u8c, ym_unletterbox_boxes): the same launch shape once more, with a per-image
// table entry (ym_lb_entry) the host computed — the resized size, where it sits in the frame, and the fp32 factors back
// to source pixels.  The device derives no geometry; the pad takes the fill and reads no source byte.
//
// Tiles (ym_slice_letterbox_u8c): the letterbox launch shape over a table of windows (ym_tile_entry) into
// sources that were uploaded once; a tile is the letterbox of its window taken as an image of its own.
#include <algorithm>

#include "common.h"
#include "yolomi_augment.h"

namespace ym {
namespace {

// meta[b] = {byte offset of image b in src, h0, w0}; out (B, 1, S, S) fp32
__global__ void resize_linear_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta, int S,
                                        int64_t total, float* __restrict__ out) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t b = i / (int64_t(S) * S);
        const int p = int(i - b * int64_t(S) * S);
        const int dy = p / S, dx = p - dy * S;
        const uint8_t* im = src + meta[3 * b];
        const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
        int v;
        if (h0 == S && w0 == S) {
            v = im[p];
        } else {
            int sx, a0, a1, sy, b0, b1;
            ym_aug_lin_coeff(dx, double(w0) / S, w0, sx, a0, a1);
            ym_aug_lin_coeff(dy, double(h0) / S, h0, sy, b0, b1);
            const int sx1 = min(sx + 1, w0 - 1), sy1 = min(sy + 1, h0 - 1);
            const uint8_t* r0 = im + int64_t(sy) * w0;
            const uint8_t* r1 = im + int64_t(sy1) * w0;
            const int h0v = int(r0[sx]) * a0 + int(r0[sx1]) * a1;
            const int h1v = int(r1[sx]) * a0 + int(r1[sx1]) * a1;
            v = (((b0 * (h0v >> 4)) >> 16) + ((b1 * (h1v >> 4)) >> 16) + 2) >> 2;
            v = min(max(v, 0), 255);
        }
        out[i] = float(v) / 255.0f;
    }
}

// ym_aug_sample for a block-uniform entry `e`.  A wave covers 256 consecutive pixels, so nearly always one slot:
// then the tile is addressed by the slot of the first lane, a scalar, and its maps, rectangle and source meta
// come through scalar loads instead of ~25 per-lane loads of the same words.
__device__ __forceinline__ int augment_pixel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                             int batch, int S, const ym_aug_entry* __restrict__ e, int x, int y) {
    if (e->flags & YM_AUG_STRETCH) return ym_aug_gain(e->gain, ym_aug_stretch_value(src, meta, batch, S, e, x, y));
    int64_t cx, cy;
    const int slot = ym_aug_slot(e, x, y, cx, cy);
    const int first = __builtin_amdgcn_readfirstlane(slot);
    int v;
    if (__all(slot == first))
        v = ym_aug_tile_value(src, meta, batch, e->fill, &e->tile[first], cx, cy, x, y);
    else
        v = ym_aug_tile_value(src, meta, batch, e->fill, &e->tile[slot], cx, cy, x, y);
    return ym_aug_gain(e->gain, v);
}

// out (B, 1, S, S) fp32; `vec`: S * S % 4 == 0 and out 16-byte aligned, so every group of four is one aligned store
__global__ void augment_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                  const ym_aug_entry* __restrict__ table, int batch, int S, int vec,
                                  float* __restrict__ out) {
    const int SS = S * S;
    const int groups = (SS + 3) >> 2;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const ym_aug_entry* e = table + b;
        float* o = out + int64_t(b) * SS;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int p = g << 2;
            int y = p / S, x = p - y * S;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = p + k < SS ? float(augment_pixel(src, meta, batch, S, e, x, y)) / 255.0f : 0.f;
                if (++x == S) { x = 0; ++y; }
            }
            if (vec) {
                *reinterpret_cast<float4*>(o + p) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p + k < SS) o[p + k] = v[k];
            }
        }
    }
}

// ---- 1-4 planes (ym_resize_linear_u8c, ym_augment_u8c): pixel-interleaved source, planar output.  The launch shape
// is augment_u8_kernel's; a pixel's geometry (slot, tile test, taps, weights) is formed once into ym_aug_taps and
// the CH planes are blended at those taps (bytes CH apart), so a thread ends with CH 16-byte stores, one per plane.

// `v[c][k]`: plane c of the thread's k-th pixel -> out planes at pixel p (SS pixels per plane)
template <int CH>
__device__ __forceinline__ void store_planes(float* __restrict__ o, int SS, int p, int vec, const float (&v)[CH][4]) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        float* oc = o + int64_t(c) * SS;
        if (vec) {
            *reinterpret_cast<float4*>(oc + p) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p + k < SS) oc[p + k] = v[c][k];
        }
    }
}

// out (B, CH, S, S) fp32.  blockIdx.y walks images, so the image's size and the copy / stretch choice are
// block-uniform.
template <int CH>
__global__ void resize_linear_u8c_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta, int batch,
                                         int S, int vec, float* __restrict__ out) {
    const int SS = S * S;
    const int groups = (SS + 3) >> 2;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const uint8_t* im = src + meta[3 * b];
        const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
        const bool copy = h0 == S && w0 == S, empty = h0 <= 0 || w0 <= 0;
        float* o = out + int64_t(b) * CH * SS;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int p = g << 2;
            int y = p / S, x = p - y * S;
            float v[CH][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (p + k < SS && !empty) {
                    if (copy) {
                        const uint8_t* px = im + int64_t(p + k) * CH;
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[c][k] = float(px[c]) / 255.0f;
                    } else {
                        ym_aug_taps t;
                        ym_aug_lin_taps(im, h0, w0, CH, S, x, y, t);
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[c][k] = float(ym_aug_taps_value(t, c)) / 255.0f;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[c][k] = 0.f;
                }
                if (++x == S) { x = 0; ++y; }
            }
            store_planes<CH>(o, SS, p, vec, v);
        }
    }
}

// ym_lb_sample_c (include/yolomi_augment.h) in resize_linear_u8c_kernel's launch shape: out (B, CH, H, W) fp32.
// blockIdx.y walks images, so the table entry, the image's meta and the copy / resize choice are block-uniform
// (scalar loads).  A pixel of the pad takes the fill and touches no source byte.
template <int CH>
__global__ void letterbox_u8c_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                     const ym_lb_entry* __restrict__ table, int batch, int H, int W, float fill,
                                     int vec, float* __restrict__ out) {
    const int HW = H * W;
    const int groups = (HW + 3) >> 2;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const ym_lb_entry e = table[b];
        const uint8_t* im = src + meta[3 * b];
        const int h0 = int(meta[3 * b + 1]), w0 = int(meta[3 * b + 2]);
        const bool empty = e.nw <= 0 || e.nh <= 0 || h0 <= 0 || w0 <= 0 || e.h0 != h0 || e.w0 != w0;
        const bool copy = e.nw == w0 && e.nh == h0;
        float* o = out + int64_t(b) * CH * HW;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int p = g << 2;
            int y = p / W, x = p - y * W;
            float v[CH][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t u = int64_t(x) - e.left, w = int64_t(y) - e.top;
                if (p + k < HW && !empty && u >= 0 && u < e.nw && w >= 0 && w < e.nh) {
                    if (copy) {
                        const uint8_t* px = im + (w * w0 + u) * CH;
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[c][k] = float(px[c]) / 255.0f;
                    } else {
                        ym_aug_taps t;
                        ym_aug_lin_taps_wh(im, h0, w0, CH, e.nw, e.nh, int(u), int(w), t);
#pragma unroll
                        for (int c = 0; c < CH; ++c) v[c][k] = float(ym_aug_taps_value(t, c)) / 255.0f;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[c][k] = fill;
                }
                if (++x == W) { x = 0; ++y; }
            }
            store_planes<CH>(o, HW, p, vec, v);
        }
    }
}

// ym_tile_sample_c (include/yolomi_augment.h) in letterbox_u8c_kernel's launch shape: out (T, CH, H, W) fp32.
// blockIdx.y walks tiles, so the entry, its validity, the window's first byte and the copy / resize choice are
// block-uniform.  The window is addressed as an image whose rows lie the source's pitch apart; a tile that is not valid
// (ym_tile_valid) takes the fill and touches no source byte, so a wrong table cannot cause a read outside an image.
// The pixel groups of one tile.  MIR: a mirrored view (YM_TILE_MIRROR_X / _Y): the column / row index that
// feeds the copy and the coefficients is reflected inside the rectangle.  The choice is made once per tile, outside
// the pixel loop, so tables without the bits run the loop they ran before the bits existed.
template <int CH, bool MIR>
__device__ __forceinline__ void slice_tile_groups(const ym_tile_entry& e, bool valid, bool copy, const uint8_t* win,
                                                  int64_t pitch, double fx, double fy, int W, int HW, int groups,
                                                  float fill, int vec, float* __restrict__ o) {
    [[maybe_unused]] const bool mir_x = (e.edges & YM_TILE_MIRROR_X) != 0, mir_y = (e.edges & YM_TILE_MIRROR_Y) != 0;
    [[maybe_unused]] const int64_t ulast = int64_t(e.nw) - 1, wlast = int64_t(e.nh) - 1;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const int p = g << 2;
        int y = p / W, x = p - y * W;
        float v[CH][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int64_t u = int64_t(x) - e.left, w = int64_t(y) - e.top;
            if (p + k < HW && valid && u >= 0 && u < e.nw && w >= 0 && w < e.nh) {
                if constexpr (MIR) {
                    u = mir_x ? ulast - u : u;
                    w = mir_y ? wlast - w : w;
                }
                if (copy) {
                    const uint8_t* px = win + w * pitch + u * CH;
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[c][k] = float(px[c]) / 255.0f;
                } else {
                    int sx, a0, a1, sy, b0, b1;
                    ym_aug_lin_coeff(int(u), fx, e.tw, sx, a0, a1);
                    ym_aug_lin_coeff(int(w), fy, e.th, sy, b0, b1);
                    ym_aug_taps tp;
                    ym_aug_set_taps_pitch(win, e.th, e.tw, CH, pitch, sx, a0, a1, sy, b0, b1, tp);
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[c][k] = float(ym_aug_taps_value(tp, c)) / 255.0f;
                }
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][k] = fill;
            }
            if (++x == W) { x = 0; ++y; }
        }
        store_planes<CH>(o, HW, p, vec, v);
    }
}

template <int CH>
__global__ void slice_letterbox_u8c_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                           int n_images, const ym_tile_entry* __restrict__ table, int n_tiles, int H,
                                           int W, float fill, int vec, float* __restrict__ out) {
    const int HW = H * W;
    const int groups = (HW + 3) >> 2;
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        const ym_tile_entry e = table[t];
        const bool valid = ym_tile_valid(meta, n_images, &e);
        const bool copy = e.nw == e.tw && e.nh == e.th;
        int64_t pitch = 0;
        const uint8_t* win = src;
        if (valid) {
            pitch = meta[3 * int64_t(e.src) + 2] * CH;
            win = src + meta[3 * int64_t(e.src)] + e.y0 * pitch + int64_t(e.x0) * CH;
        }
        const double fx = valid ? double(e.tw) / e.nw : 0.0, fy = valid ? double(e.th) / e.nh : 0.0;
        float* o = out + int64_t(t) * CH * HW;
        if (e.edges & (YM_TILE_MIRROR_X | YM_TILE_MIRROR_Y))            // block-uniform, like everything of the entry
            slice_tile_groups<CH, true>(e, valid, copy, win, pitch, fx, fy, W, HW, groups, fill, vec, o);
        else
            slice_tile_groups<CH, false>(e, valid, copy, win, pitch, fx, fy, W, HW, groups, fill, vec, o);
    }
}

// one thread per box; blockIdx.y walks images (entry and count through scalar loads)
__global__ void unletterbox_boxes_kernel(const float4* __restrict__ boxes, const int32_t* __restrict__ count,
                                         const ym_lb_entry* __restrict__ table, int batch, int64_t N, float fw,
                                         float fh, float4* __restrict__ out) {
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const ym_lb_entry e = table[b];
        const int64_t n = min(int64_t(count[b]), N);
        const float left = float(e.left), top = float(e.top), w0 = float(e.w0), h0 = float(e.h0);
        for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
            const float4 q = boxes[b * N + i];
            float4 r;
            r.x = fminf(fmaxf(__fmul_rn(__fsub_rn(__fmul_rn(q.x, fw), left), e.sx), 0.f), w0);
            r.y = fminf(fmaxf(__fmul_rn(__fsub_rn(__fmul_rn(q.y, fh), top), e.sy), 0.f), h0);
            r.z = fminf(fmaxf(__fmul_rn(__fsub_rn(__fmul_rn(q.z, fw), left), e.sx), 0.f), w0);
            r.w = fminf(fmaxf(__fmul_rn(__fsub_rn(__fmul_rn(q.w, fh), top), e.sy), 0.f), h0);
            out[b * N + i] = r;
        }
    }
}

// ym_aug_sample_c for a block-uniform entry `e` and colour entry `col` (may be null), with augment_pixel's
// wave-uniform-slot path
template <int CH>
__device__ __forceinline__ void augment_pixel_c(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                int batch, int S, const ym_aug_entry* __restrict__ e,
                                                const ym_aug_colour* __restrict__ col, int x, int y, int* v) {
    ym_aug_taps t = {};
    bool hit;
    if (e->flags & YM_AUG_STRETCH) {
        hit = ym_aug_stretch_taps(src, meta, batch, CH, S, e, x, y, t);
    } else {
        int64_t cx, cy;
        const int slot = ym_aug_slot(e, x, y, cx, cy);
        const int first = __builtin_amdgcn_readfirstlane(slot);
        if (__all(slot == first))
            hit = ym_aug_tile_taps(src, meta, batch, CH, &e->tile[first], cx, cy, x, y, t);
        else
            hit = ym_aug_tile_taps(src, meta, batch, CH, &e->tile[slot], cx, cy, x, y, t);
    }
    ym_aug_planes(e, col, CH, hit, t, v);
}

// out (B, CH, S, S) fp32; `colour` null or one entry per image (CH == 3); `vec` as for augment_u8_kernel (a plane
// is S * S floats, so every plane's groups are aligned when the first plane's are)
template <int CH>
__global__ void augment_u8c_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                   const ym_aug_entry* __restrict__ table, const ym_aug_colour* __restrict__ colour,
                                   int batch, int S, int vec, float* __restrict__ out) {
    const int SS = S * S;
    const int groups = (SS + 3) >> 2;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const ym_aug_entry* e = table + b;
        const ym_aug_colour* col = CH == 3 && colour ? colour + b : nullptr;
        float* o = out + int64_t(b) * CH * SS;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int p = g << 2;
            int y = p / S, x = p - y * S;
            float v[CH][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int u[CH] = {};
                if (p + k < SS) augment_pixel_c<CH>(src, meta, batch, S, e, col, x, y, u);
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][k] = float(u[c]) / 255.0f;
                if (++x == S) { x = 0; ++y; }
            }
            store_planes<CH>(o, SS, p, vec, v);
        }
    }
}

// ---- MixUp (ym_augment_mix_u8c): augment_u8c_kernel's launch shape with a second, compact table of
// partner entries.  The mix record is block-uniform like the entry, so the choice between the two pixel functions
// below is a scalar branch; an image that is not mixed runs augment_pixel_c and never forms a partner address.

// ym_aug_entry_taps for a block-uniform entry `e`, with augment_pixel's wave-uniform-slot path
template <int CH>
__device__ __forceinline__ bool augment_taps_c(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                               int batch, int S, const ym_aug_entry* __restrict__ e, int x, int y,
                                               ym_aug_taps& t) {
    if (e->flags & YM_AUG_STRETCH) return ym_aug_stretch_taps(src, meta, batch, CH, S, e, x, y, t);
    int64_t cx, cy;
    const int slot = ym_aug_slot(e, x, y, cx, cy);
    const int first = __builtin_amdgcn_readfirstlane(slot);
    if (__all(slot == first)) return ym_aug_tile_taps(src, meta, batch, CH, &e->tile[first], cx, cy, x, y, t);
    return ym_aug_tile_taps(src, meta, batch, CH, &e->tile[slot], cx, cy, x, y, t);
}

// ym_aug_mix_sample_c of a mixed image: the two entries one after the other through one ym_aug_taps, each with its
// own slot vote
template <int CH>
__device__ __forceinline__ void augment_mix_pixel_c(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                                    int batch, int S, const ym_aug_entry* __restrict__ e,
                                                    const ym_aug_entry* __restrict__ pe, int ratio,
                                                    const ym_aug_colour* __restrict__ col, int x, int y, int* v) {
    ym_aug_taps t = {};
    int w[CH];
    bool hit = augment_taps_c<CH>(src, meta, batch, S, e, x, y, t);
    ym_aug_raw_planes(e, CH, hit, t, v);
    hit = augment_taps_c<CH>(src, meta, batch, S, pe, x, y, t);
    ym_aug_raw_planes(pe, CH, hit, t, w);
    ym_aug_mix_planes(e, col, CH, ratio, w, v);
}

// out (B, CH, S, S) fp32; `partner` n_partner entries (may be null when 0), `mix` one record per image; the rest as
// for augment_u8c_kernel
template <int CH>
__global__ void augment_mix_u8c_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ meta,
                                       const ym_aug_entry* __restrict__ table,
                                       const ym_aug_entry* __restrict__ partner, int n_partner,
                                       const ym_aug_mix* __restrict__ mix, const ym_aug_colour* __restrict__ colour,
                                       int batch, int S, int vec, float* __restrict__ out) {
    const int SS = S * S;
    const int groups = (SS + 3) >> 2;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const ym_aug_entry* e = table + b;
        const ym_aug_colour* col = CH == 3 && colour ? colour + b : nullptr;
        const bool mixed = ym_aug_mix_valid(mix + b, n_partner);
        const ym_aug_entry* pe = mixed ? partner + mix[b].partner : e;      // e: never read, and inside a table
        const int ratio = mix[b].ratio;
        float* o = out + int64_t(b) * CH * SS;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int p = g << 2;
            int y = p / S, x = p - y * S;
            float v[CH][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int u[CH] = {};
                if (p + k < SS) {
                    if (mixed)
                        augment_mix_pixel_c<CH>(src, meta, batch, S, e, pe, ratio, col, x, y, u);
                    else
                        augment_pixel_c<CH>(src, meta, batch, S, e, col, x, y, u);
                }
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][k] = float(u[c]) / 255.0f;
                if (++x == S) { x = 0; ++y; }
            }
            store_planes<CH>(o, SS, p, vec, v);
        }
    }
}

}  // namespace
}  // namespace ym

using namespace ym;

extern "C" int ym_resize_linear_u8(const uint8_t* src, const int64_t* meta, int batch, int size, float* out,
                                   void* stream) {
    YM_CHECK_ARG(src && meta && out && batch >= 0 && size > 0, "ym_resize_linear_u8: bad arguments");
    const int64_t total = int64_t(batch) * size * size;
    if (total == 0) return YM_OK;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(resize_linear_u8_kernel, dim3(unsigned(blocks)), dim3(256), 0, as_stream(stream), src, meta, size,
                       total, out);
    YM_LAUNCH_CHECK("ym_resize_linear_u8");
    return YM_OK;
}

extern "C" int ym_augment_u8(const uint8_t* src, const int64_t* meta, const ym_aug_entry* table_dev, int batch,
                             int size, float* out, void* stream) {
    YM_CHECK_ARG(src && meta && table_dev && out && batch >= 0 && size > 0 && size <= 32768,
                 "ym_augment_u8: bad arguments");
    if (batch == 0) return YM_OK;
    const int64_t ss = int64_t(size) * size;
    const int64_t groups = (ss + 3) / 4;
    const int vec = ss % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int64_t bx = std::min<int64_t>((groups + 255) / 256, 256);      // per image; larger images grid-stride
    hipLaunchKernelGGL(augment_u8_kernel, dim3(unsigned(bx), unsigned(std::min(batch, 65535))), dim3(256), 0,
                       as_stream(stream), src, meta, table_dev, batch, size, vec, out);
    YM_LAUNCH_CHECK("ym_augment_u8");
    return YM_OK;
}

namespace {

// grid of the per-image launch shape: blockIdx.x covers up to 256 blocks of groups (larger images grid-stride),
// blockIdx.y the images
dim3 image_grid(int batch, int size) {
    const int64_t groups = (int64_t(size) * size + 3) / 4;
    return dim3(unsigned(std::min<int64_t>((groups + 255) / 256, 256)), unsigned(std::min(batch, 65535)));
}

int planes_vec(int size, const float* out) {
    return (int64_t(size) * size) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
}

}  // namespace

extern "C" int ym_resize_linear_u8c(const uint8_t* src, const int64_t* meta, int batch, int ch, int size, float* out,
                                    void* stream) {
    YM_CHECK_ARG(src && meta && out && batch >= 0 && size > 0 && size <= 32768 && ch >= 1 && ch <= 4,
                 "ym_resize_linear_u8c: bad arguments (ch is 1..4)");
    if (batch == 0) return YM_OK;
    const dim3 grid = image_grid(batch, size);
    const int vec = planes_vec(size, out);
#define YM_RESIZE_C(CH)                                                                                          \
    hipLaunchKernelGGL(resize_linear_u8c_kernel<CH>, grid, dim3(256), 0, as_stream(stream), src, meta, batch, size, \
                       vec, out)
    switch (ch) {
        case 1: YM_RESIZE_C(1); break;
        case 2: YM_RESIZE_C(2); break;
        case 3: YM_RESIZE_C(3); break;
        default: YM_RESIZE_C(4); break;
    }
#undef YM_RESIZE_C
    YM_LAUNCH_CHECK("ym_resize_linear_u8c");
    return YM_OK;
}

extern "C" int ym_letterbox_u8c(const uint8_t* src, const int64_t* meta, const ym_lb_entry* table_dev, int batch,
                                int ch, int out_h, int out_w, int fill, float* out, void* stream) {
    YM_CHECK_ARG(src && meta && table_dev && out && batch >= 0 && out_h > 0 && out_h <= 32768 && out_w > 0 &&
                     out_w <= 32768 && ch >= 1 && ch <= 4,
                 "ym_letterbox_u8c: bad arguments (ch is 1..4, out_h and out_w 1..32768)");
    if (batch == 0) return YM_OK;
    const int64_t hw = int64_t(out_h) * out_w;
    const int64_t groups = (hw + 3) / 4;
    const dim3 grid(unsigned(std::min<int64_t>((groups + 255) / 256, 256)), unsigned(std::min(batch, 65535)));
    const int vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const float fv = float(fill & 255) / 255.0f;
#define YM_LETTERBOX_C(CH)                                                                                      \
    hipLaunchKernelGGL(letterbox_u8c_kernel<CH>, grid, dim3(256), 0, as_stream(stream), src, meta, table_dev,   \
                       batch, out_h, out_w, fv, vec, out)
    switch (ch) {
        case 1: YM_LETTERBOX_C(1); break;
        case 2: YM_LETTERBOX_C(2); break;
        case 3: YM_LETTERBOX_C(3); break;
        default: YM_LETTERBOX_C(4); break;
    }
#undef YM_LETTERBOX_C
    YM_LAUNCH_CHECK("ym_letterbox_u8c");
    return YM_OK;
}

extern "C" int ym_slice_letterbox_u8c(const uint8_t* src, const int64_t* meta, int n_images,
                                      const ym_tile_entry* table_dev, int n_tiles, int ch, int out_h, int out_w,
                                      int fill, float* out, void* stream) {
    YM_CHECK_ARG(src && meta && table_dev && out && n_images >= 0 && n_tiles >= 0 && out_h > 0 && out_h <= 32768 &&
                     out_w > 0 && out_w <= 32768 && ch >= 1 && ch <= 4,
                 "ym_slice_letterbox_u8c: bad arguments (ch is 1..4, out_h and out_w 1..32768)");
    if (n_tiles == 0) return YM_OK;
    const int64_t hw = int64_t(out_h) * out_w;
    const int64_t groups = (hw + 3) / 4;
    const dim3 grid(unsigned(std::min<int64_t>((groups + 255) / 256, 256)), unsigned(std::min(n_tiles, 65535)));
    const int vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const float fv = float(fill & 255) / 255.0f;
#define YM_SLICE_C(CH)                                                                                            \
    hipLaunchKernelGGL(slice_letterbox_u8c_kernel<CH>, grid, dim3(256), 0, as_stream(stream), src, meta, n_images, \
                       table_dev, n_tiles, out_h, out_w, fv, vec, out)
    switch (ch) {
        case 1: YM_SLICE_C(1); break;
        case 2: YM_SLICE_C(2); break;
        case 3: YM_SLICE_C(3); break;
        default: YM_SLICE_C(4); break;
    }
#undef YM_SLICE_C
    YM_LAUNCH_CHECK("ym_slice_letterbox_u8c");
    return YM_OK;
}

extern "C" int ym_unletterbox_boxes(const float* boxes, const int32_t* count, const ym_lb_entry* table_dev, int64_t B,
                                    int64_t N, int out_h, int out_w, float* out, void* stream) {
    YM_CHECK_ARG(boxes && count && table_dev && out && B >= 0 && B <= INT32_MAX && N >= 0 && out_h > 0 && out_w > 0,
                 "ym_unletterbox_boxes: bad arguments");
    YM_CHECK_ARG(reinterpret_cast<uintptr_t>(boxes) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
                 "ym_unletterbox_boxes: boxes and out must be 16-byte aligned");
    if (B == 0 || N == 0) return YM_OK;
    const dim3 grid(unsigned(std::min<int64_t>((N + 255) / 256, 1024)), unsigned(std::min<int64_t>(B, 65535)));
    hipLaunchKernelGGL(unletterbox_boxes_kernel, grid, dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4*>(boxes), count, table_dev, int(B), N, float(out_w), float(out_h),
                       reinterpret_cast<float4*>(out));
    YM_LAUNCH_CHECK("ym_unletterbox_boxes");
    return YM_OK;
}

extern "C" int ym_augment_u8c(const uint8_t* src, const int64_t* meta, const ym_aug_entry* table_dev,
                              const ym_aug_colour* colour_dev, int batch, int ch, int size, float* out,
                              void* stream) {
    YM_CHECK_ARG(src && meta && table_dev && out && batch >= 0 && size > 0 && size <= 32768 && ch >= 1 && ch <= 4,
                 "ym_augment_u8c: bad arguments (ch is 1..4)");
    YM_CHECK_ARG(!colour_dev || ch == 3, "ym_augment_u8c: a colour table needs ch == 3 (got %d)", ch);
    if (batch == 0) return YM_OK;
    const dim3 grid = image_grid(batch, size);
    const int vec = planes_vec(size, out);
#define YM_AUGMENT_C(CH)                                                                                       \
    hipLaunchKernelGGL(augment_u8c_kernel<CH>, grid, dim3(256), 0, as_stream(stream), src, meta, table_dev,    \
                       colour_dev, batch, size, vec, out)
    switch (ch) {
        case 1: YM_AUGMENT_C(1); break;
        case 2: YM_AUGMENT_C(2); break;
        case 3: YM_AUGMENT_C(3); break;
        default: YM_AUGMENT_C(4); break;
    }
#undef YM_AUGMENT_C
    YM_LAUNCH_CHECK("ym_augment_u8c");
    return YM_OK;
}

extern "C" int ym_augment_mix_u8c(const uint8_t* src, const int64_t* meta, const ym_aug_entry* table_dev,
                                  const ym_aug_entry* partner_dev, int n_partner, const ym_aug_mix* mix_dev,
                                  const ym_aug_colour* colour_dev, int batch, int ch, int size, float* out,
                                  void* stream) {
    YM_CHECK_ARG(src && meta && table_dev && mix_dev && out && batch >= 0 && size > 0 && size <= 32768 && ch >= 1 &&
                     ch <= 4,
                 "ym_augment_mix_u8c: bad arguments (ch is 1..4)");
    YM_CHECK_ARG(n_partner >= 0 && (partner_dev || n_partner == 0),
                 "ym_augment_mix_u8c: n_partner = %d needs a partner table", n_partner);
    YM_CHECK_ARG(!colour_dev || ch == 3, "ym_augment_mix_u8c: a colour table needs ch == 3 (got %d)", ch);
    if (batch == 0) return YM_OK;
    const dim3 grid = image_grid(batch, size);
    const int vec = planes_vec(size, out);
#define YM_AUGMENT_MIX_C(CH)                                                                                       \
    hipLaunchKernelGGL(augment_mix_u8c_kernel<CH>, grid, dim3(256), 0, as_stream(stream), src, meta, table_dev,    \
                       partner_dev, n_partner, mix_dev, colour_dev, batch, size, vec, out)
    switch (ch) {
        case 1: YM_AUGMENT_MIX_C(1); break;
        case 2: YM_AUGMENT_MIX_C(2); break;
        case 3: YM_AUGMENT_MIX_C(3); break;
        default: YM_AUGMENT_MIX_C(4); break;
    }
#undef YM_AUGMENT_MIX_C
    YM_LAUNCH_CHECK("ym_augment_mix_u8c");
    return YM_OK;
}
