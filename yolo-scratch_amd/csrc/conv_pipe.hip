// Persistent software-pipelined implicit-GEMM convolution for gfx950 (fp16 forward, bf16 data
// gradient, fp32 accumulate) — the large 3x3 / 1x1 layers of the YOLOv11 graph.
//
// Replaces nn.Conv2d forward / input-gradient inside Conv (/root/reference/yolo_scratch_cuda/
// models/yolo11_modules.py:21-33, Detect :221-234) where the GEMM is big enough to fill the chip.
//
// Why a second implicit GEMM (conv.hip keeps the 2-stage one for small / odd shapes): its
// 128 x 128 tiles, one K stage in flight and one barrier + read burst per K step leave the MFMA
// pipes 77 % idle (profiles/r01/pmc_op6): every K step opens with the LDS latency of its fragment
// reads, and 64 B/cycle of staging per CU at peak is more than the TA delivers.  Here:
//  * 256 pixels x 128 channels per tile, 16 waves of 32 x 64 (64-channel tiles: 8 waves of 64 x 32),
//    K steps of 64 (two 32-deep halves):
//    a third fewer staged bytes per FLOP than 128 x 128;
//  * a 3-stage LDS ring filled by LDS-DMA (buffer_load ... lds) with TWO stages in flight, counted
//    vmcnt waits and raw s_barrier (no vmcnt(0) drain in the loop);
//  * the barrier sits in the MIDDLE of a K step: a step reads its second-half fragments, runs the
//    first half's 16 MFMAs, waits for the next stage, barriers, issues the DMA into the buffer it
//    has just finished with, reads the next stage's first-half fragments and runs the second half's
//    16 MFMAs — every LDS read has 16 MFMAs to hide behind, the pipe never waits on a fresh read;
//  * the K offset rides in the buffer instruction's SGPR soffset (channel counts are multiples of
//    64): one DMA costs no VALU inside a tap;
//  * persistent workgroups (one per CU) stream their tiles back to back: the next tile's first
//    stages are in flight during the current tile's epilogue; tiles are grouped per XCD, the
//    channel tiles of one pixel tile on the same XCD (input rows reused from its L2);
//  * BatchNorm statistics accumulate in registers across a workgroup's tiles and are written as
//    one partial row per workgroup (no atomics, fixed order: bit-reproducible).
// The stride-2 data gradient runs as 4 output-parity classes inside the same tile stream, each
// with only the taps that land (as conv.hip).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "conv_epi.h"
#include "conv_pipe.h"
#include "bn_fold.h"
#include "tile.h"

namespace ym {

// selection policy (ym_conv_set_pipe): -1 default (3); 0 never; 1 layers of >= 1024 tiles with >= 128
// output channels, no stride-2 data gradient; 2 every eligible layer of >= 256 tiles; 3 (default) the
// wider rule of pipe_plan (s@640 bs64 step: 2940 img/s vs 2902 for rule 1)
//
// Measured and rejected, with the profile that holds the numbers (the code of every variant is in history at the parent
// of the commit that removed them, where a second build of the library carried them behind setters):
//  * 256 x 128 on 8 waves of 64 x 64 for training: within +-3.5 % of the 16-wave tile (profiles/r05/pipe_wave_tile_ab.txt);
//  * the 32x32x16 MFMA shape, on the same tiles +8..+23 % per layer, on 8 waves of 64 x 64 +1..+14 %, and every fragment
//    read pinned ahead of the MFMAs it covers, -3..+7 % (profiles/r06/pipe_mfma_order_ab.txt);
//  * the nested loop without the carried slot offset (profiles/r06/pipe_loop_ab.txt), the nested loop for the eval
//    instance (profiles/r06/pipe_eval_loop_ab.txt), tap-innermost K order everywhere (profiles/r06/pipe_taporder_ab.txt);
//  * the LDS-transposed epilogue, 2-7 % slower on every forward (profiles/r04/pipe_fwd_reg_epilogue_ab.txt);
//  * the ablation instances (no DMA / no MFMA / one operand's DMA only; wrong results by design) that located the time
//    (profiles/r05/pipe_ablation_ab.txt) and the class-search control path forced everywhere
//    (profiles/r05/pipe_c1_vs_generic_ab.txt).

namespace {

constexpr int PF = 0;   // forward: fp16 x fp16
constexpr int PD = 1;   // data gradient: bf16 x bf16

struct PipeArgs {
    const bf16_t* x; int64_t x_bs, x_ld;     // gathered tensor view (elements)
    const bf16_t* w;                          // [Nout][KH][KW][Kin]
    void* y; int64_t y_bs, y_ld;              // output view
    float* st_sum; float* st_sq;              // [rows][Nout] or null
    int GH, GW, Kin;
    int OH, OW, Nout;
    int KH, KW, stride, pad, N;
    int out_f32, accumulate;
    int os;                                   // 2: stride-2 data gradient (4 parity classes)
    int ntiles;                               // channel tiles
    int mt_pre[5];                            // first m-tile of each class (prefix), mt_pre[ncls] = total
    int ncls;
    BnFoldArgs fold;                          // BatchNorm finalize as the tail (ym_conv_fwd_bn); gamma null = off
};

struct Cls {
    int py, px, OWc, kh0, kw0, nkw, ntap;
    uint32_t OHW;
    int64_t Mc;
};

__device__ __forceinline__ Cls cls_of(const PipeArgs& a, int c) {
    Cls k;
    const int os = a.os;
    k.py = os == 2 ? (c >> 1) : 0;
    k.px = os == 2 ? (c & 1) : 0;
    const int OHc = (a.OH - k.py + os - 1) / os;
    k.OWc = (a.OW - k.px + os - 1) / os;
    k.kh0 = os == 2 ? ((k.py + a.pad) & 1) : 0;
    k.kw0 = os == 2 ? ((k.px + a.pad) & 1) : 0;
    k.nkw = (a.KW - k.kw0 + os - 1) / os;
    k.ntap = ((a.KH - k.kh0 + os - 1) / os) * k.nkw;
    k.OHW = uint32_t(OHc) * uint32_t(k.OWc);
    k.Mc = int64_t(a.N) * k.OHW;
    return k;
}

__device__ __forceinline__ int cls_find(const PipeArgs& a, int mt) {
    int c = 0;
    while (c + 1 < a.ncls && mt >= a.mt_pre[c + 1]) ++c;
    return c;
}

// (image, in-image index, row) of pixel m0 + r, r < 256, given the tile's (tn, tp) = divmod(m0, ohw) (computed
// once per tile): one wrap for the image, the row by the float reciprocal of the row width with one
// correction (x < 2^24) — the generic 32-bit divisions these replace cost ~30 VALU each and ran per pixel
// in every tile's setup and epilogue (12 per lane and tile)
__device__ __forceinline__ void split_pix(uint32_t tn, uint32_t tp, uint32_t r, uint32_t ohw, uint32_t w, float inv_w,
                                          uint32_t& n, uint32_t& pix, uint32_t& row) {
    pix = tp + r;
    n = tn;
    while (pix >= ohw) { pix -= ohw; ++n; }
    uint32_t q = uint32_t(float(pix) * inv_w);
    const int rem = int(pix) - int(q * w);
    q = rem < 0 ? q - 1 : (rem >= int(w) ? q + 1 : q);
    row = q;
}

// issue side of the stage stream: which tile / tap / 64-channel chunk the next LDS-DMA stage
// stages, and the per-lane gather offsets of the current tile and tap.  All control state is
// wave-uniform (scalar registers); per stage the DMAs cost one M0 write each, per tap one
// bounds select per gather row, per tile one pixel decomposition.
// C1 (every launch pipe_plan makes by default: one output class, maps of >= BM pixels): no class search, no
// per-tile divisions — the tile's (image, in-image offset) advance by a constant step with one wrap, the
// buffer resource over the tile's images is built once per tile.  (Round 5: the generic form spent ~3.8 SALU
// and ~3.5 VALU per MFMA, SQ_INSTS_* over op 73, much of it the per-tile class search and 32-bit divisions of
// both the issue and the compute side; its no-MFMA ablation alone ran 107 of the layer's 145 us.)
// TO (round 6, single-class path only): K order of the stage stream.  0: channel chunk innermost — (tap 0, chunk 0),
// (tap 0, chunk 1), .., (tap 1, chunk 0), ..; 1: tap innermost — every tap of channel chunk 0, then of chunk 1, so
// the taps that re-read the same input pixels run back to back and their overlap comes from L2 (one 64-channel
// chunk's footprint per tile instead of every chunk's)
template <int BM, int BN, int NW, int MODE, bool C1 = false, int TO = 0>
struct Issuer {
    static constexpr int AI = BN / 8 / NW, BI = BM / 8 / NW, RB = 128;
    const PipeArgs& a;
    int wave, lrow, lslot, kc;
    uint32_t xld_b;
    int mt_lo, qstride, ntile;
    // stream position
    int i = 0, ti = 0, tj = 0, kci = 0;
    // current tile
    int nrows = 0, nkw = 1, kh0 = 0, kw0 = 0;
    const bf16_t* x_tile = nullptr;
    int x_bytes = 0;
    int bh[BI], bw[BI];
    uint32_t bc[BI], b_off[BI];
    uint32_t a_tap = 0;
    // C1: the staged tile's first pixel (image, in-image offset, flat index) and the per-tile step
    int tn = 0, m0 = 0, step_n = 0, m_step = 0;
    uint32_t tp = 0, step_p = 0, ohw = 1;
    float inv_w = 1.f;
    __amdgpu_buffer_rsrc_t xres_t;

    __device__ Issuer(const PipeArgs& a_, int wave_, int lane, int mt_lo_, int qstride_, int ntile_)
        : a(a_), wave(wave_), lrow(lane >> 3), lslot(lane & 7), kc(a_.Kin >> 6), xld_b(uint32_t(a_.x_ld) * 2u),
          mt_lo(mt_lo_), qstride(qstride_), ntile(ntile_) {
        if constexpr (C1) {
            // a zero-record resource until the first tile_setup: a workgroup without tiles still issues its prologue's
            // (out-of-range) DMAs through it, and an uninitialised descriptor made them real loads (a memory fault at
            // s@640 bs2 under ym_conv_set_select_batch(64), where most of the grid has no tile)
            xres_t = make_rsrc(a.x, 0);
            ohw = uint32_t(a.OH) * uint32_t(a.OW);
            m0 = mt_lo * BM;
            tn = int(uint32_t(m0) / ohw);
            tp = uint32_t(m0) - uint32_t(tn) * ohw;
            m_step = qstride * BM;
            step_n = int(uint32_t(m_step) / ohw);
            step_p = uint32_t(m_step) - uint32_t(step_n) * ohw;
            inv_w = 1.0f / float(a.OW);
            nkw = a.KW;
            nrows = a.KH;
        }
    }

    __device__ __forceinline__ void tile_setup() {
        if constexpr (C1) {
            x_tile = a.x + int64_t(tn) * a.x_bs;
            const int64_t xb = (int64_t(a.N) - tn) * a.x_bs * 2;
            x_bytes = int(xb < 0x7fffffff ? xb : 0x7fffffff);
            const uint64_t xp = reinterpret_cast<uint64_t>(x_tile);
            const uint32_t xlo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(xp))));
            const uint32_t xhi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(xp >> 32))));
            xres_t = make_rsrc(reinterpret_cast<const void*>((uint64_t(xhi) << 32) | xlo),
                               __builtin_amdgcn_readfirstlane(x_bytes));
            const int M = a.N * int(ohw);
#pragma unroll
            for (int j = 0; j < BI; ++j) {
                const int r = (wave * BI + j) * 8 + lrow;
                if (m0 + r < M) {
                    uint32_t pix = tp + uint32_t(r), n = 0;
                    if (pix >= ohw) { pix -= ohw; n = 1; }              // ohw >= BM: at most one wrap
                    uint32_t q = uint32_t(float(pix) * inv_w);
                    const int rem = int(pix) - int(q * uint32_t(a.OW));
                    q = rem < 0 ? q - 1 : (rem >= a.OW ? q + 1 : q);
                    const int oh = int(q), ow = int(pix - q * uint32_t(a.OW));
                    if (MODE == PF) {
                        bh[j] = oh * a.stride - a.pad;
                        bw[j] = ow * a.stride - a.pad;
                    } else {                        // stride-1 data gradient
                        bh[j] = oh + a.pad;
                        bw[j] = ow + a.pad;
                    }
                    bc[j] = n * uint32_t(a.x_bs) * 2u + uint32_t(bh[j] * a.GW + bw[j]) * xld_b +
                            uint32_t(lslot ^ fsw128(r)) * 16u;
                } else {
                    bh[j] = -(1 << 20);             // no tap is in range
                    bw[j] = 0;
                    bc[j] = 0;
                }
            }
            return;
        }
        const int mt = mt_lo + i * qstride;
        const int c = cls_find(a, mt);
        const Cls k = cls_of(a, c);
        nkw = k.nkw;
        nrows = k.ntap / k.nkw;
        kh0 = k.kh0;
        kw0 = k.kw0;
        const int64_t m0l = int64_t(mt - a.mt_pre[c]) * BM;
        const uint32_t nfirst = uint32_t(m0l) / k.OHW, tpl = uint32_t(m0l) - nfirst * k.OHW;
        const float inv_wl = 1.0f / float(k.OWc);
        x_tile = a.x + int64_t(nfirst) * a.x_bs;
        const int64_t xb = (int64_t(a.N) - nfirst) * a.x_bs * 2;
        x_bytes = int(xb < 0x7fffffff ? xb : 0x7fffffff);
#pragma unroll
        for (int j = 0; j < BI; ++j) {
            const int r = (wave * BI + j) * 8 + lrow;
            const int64_t m = m0l + r;
            if (m < k.Mc) {
                uint32_t n, pix, ii;
                split_pix(nfirst, tpl, uint32_t(r), k.OHW, uint32_t(k.OWc), inv_wl, n, pix, ii);
                const int oh = int(ii) * a.os + k.py, ow = int(pix - ii * uint32_t(k.OWc)) * a.os + k.px;
                if (MODE == PF) {
                    bh[j] = oh * a.stride - a.pad;
                    bw[j] = ow * a.stride - a.pad;
                } else {                        // the class's first tap lands on whole pixels
                    bh[j] = (oh + a.pad - k.kh0) >> (a.stride - 1);
                    bw[j] = (ow + a.pad - k.kw0) >> (a.stride - 1);
                }
                bc[j] = (n - nfirst) * uint32_t(a.x_bs) * 2u + uint32_t(bh[j] * a.GW + bw[j]) * xld_b +
                        uint32_t(lslot ^ fsw128(r)) * 16u;
            } else {
                bh[j] = -(1 << 20);             // no tap is in range
                bw[j] = 0;
                bc[j] = 0;
            }
        }
    }

    __device__ __forceinline__ void tap_setup() {
        const int dir = MODE == PF ? 1 : -1;
        const int ost = MODE == PF ? 1 : a.stride;
        const uint32_t delta = uint32_t(dir * (ti * a.GW + tj)) * xld_b;
#pragma unroll
        for (int j = 0; j < BI; ++j) {
            const int gh = bh[j] + dir * ti, gw = bw[j] + dir * tj;
            const bool ok = uint32_t(gh) < uint32_t(a.GH) && uint32_t(gw) < uint32_t(a.GW);
            b_off[j] = ok ? bc[j] + delta : OOB;
        }
        a_tap = C1 ? uint32_t((ti * a.KW + tj) * a.Kin) * 2u
                   : uint32_t(((kh0 + ti * ost) * a.KW + (kw0 + tj * ost)) * a.Kin) * 2u;
    }

    __device__ __forceinline__ void start() {
        if (ntile > 0) {
            tile_setup();
            tap_setup();
        }
    }

    // the DMAs of the stage at the stream position into `st` (straight-line code: the caller interleaves
    // them with MFMAs); `live` false = past the stream's end: out-of-range offsets, nothing is fetched and
    // every step keeps the same DMA count (the counted vmcnt waits stay constant)
    __device__ __forceinline__ void issue_dma(char* st, __amdgpu_buffer_rsrc_t wres, const uint32_t* a_off, bool live) {
        const uint32_t kb = uint32_t(kci) * 128u;
        __amdgpu_buffer_rsrc_t xres;
        if constexpr (C1) {
            xres = xres_t;
        } else {
            // wave-uniform base / size (readfirstlane: else hipcc waterfalls every DMA over the resource)
            const uint64_t xb = reinterpret_cast<uint64_t>(x_tile);
            const uint32_t xlo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(xb))));
            const uint32_t xhi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(xb >> 32))));
            xres = make_rsrc(reinterpret_cast<const void*>((uint64_t(xhi) << 32) | xlo),
                             __builtin_amdgcn_readfirstlane(x_bytes));
        }
#pragma unroll
        for (int j = 0; j < AI; ++j)
            dma16(wres, st + (wave * AI + j) * 1024, live ? a_off[j] : OOB, a_tap + kb);
#pragma unroll
        for (int j = 0; j < BI; ++j)
            dma16(xres, st + BN * RB + (wave * BI + j) * 1024, live ? b_off[j] : OOB, kb);
    }

    // advance the stream position by one stage (new tap: its gather offsets; new tile: its pixels)
    __device__ __forceinline__ void advance() {
        if constexpr (TO == 1) {
            static_assert(C1, "tap-innermost order: single-class path");
            if (++tj == nkw) {
                tj = 0;
                if (++ti == nrows) {
                    ti = 0;
                    if (++kci == kc) {
                        kci = 0;
                        if (++i < ntile) {
                            m0 += m_step;
                            tn += step_n;
                            tp += step_p;
                            if (tp >= ohw) { tp -= ohw; ++tn; }
                            tile_setup();
                        }
                    }
                }
            }
            tap_setup();
            return;
        }
        if (++kci == kc) {
            kci = 0;
            if (++tj == nkw) {
                tj = 0;
                if (++ti == nrows) {
                    ti = 0;
                    if (++i < ntile) {
                        if constexpr (C1) {
                            m0 += m_step;
                            tn += step_n;
                            tp += step_p;
                            if (tp >= ohw) { tp -= ohw; ++tn; }
                        }
                        tile_setup();
                    }
                }
            }
            tap_setup();
        }
    }
};

// The epilogue is register-only (conv_epi.h epilogue_regs: no LDS, so hipcc does not drain the in-flight stages in front
// of it) and the next step's wait leaves its stores in flight — both directions since round 4.
// C1: one output class on maps of >= BM pixels (Issuer's fast path; the stride-2 data gradient's four classes and tiny
// maps take the generic one)
// EV: the eval-mode Conv block instance (ym_conv_fwd_eval at large batches: running-statistics BatchNorm / SiLU /
// residual in the register epilogue, conv_epi.h EvalEpi; a C1 forward without statistics; e is not read otherwise)
// NESTED: loop form.  false (the generic and eval instances): one flat loop over the workgroup's K steps whose body tests
// for a tile's first step (accumulator reset, the wait that leaves the previous epilogue's stores in flight) and last
// step (epilogue) every iteration; true (the C1 training instances since round 6): tiles x K steps as two nested loops —
// the tile's first step peeled with its own wait, the inner loop a bare K step, the ring slot carried as a byte offset
// (an add instead of a multiply) and the stream-end test against a hoisted limit.  ~22 instead of ~33 scalar
// instructions per common K step; same-process layer A/B (profiles/r06/pipe_loop_ab.txt) -1..-5 % on most pipelined
// layers (op 71 fwd -11.6 %), op 73 fwd +1.5 %; the whole step within +-0.2 % (the launches overlap other streams' work
// there).  The eval instance measured within the run-to-run spread either way (profiles/r06/pipe_eval_loop_ab.txt)
// TO: Issuer's K order (tap_inner decides where it is 1)
template <int BM, int BN, int WM, int WN, int MODE, bool C1 = false, bool EV = false, bool NESTED = false, int TO = 0>
__global__ void __launch_bounds__(WM * WN * 64, 1) conv_pipe_kernel(PipeArgs a, EvalArgs e) {
    static_assert(!EV || (C1 && MODE == PF), "the eval instance is a single-class forward");
    static_assert(!NESTED || C1, "the nested loop form is the single-class path's");
    // LDS ring of K stages — stage g computing, g+1 .. g+NS-1 in flight
    constexpr int NS = 3;
    constexpr int RB = 128;                   // 64 K x 2 B per LDS row
    constexpr int NW = WM * WN;
    constexpr int AI = BN / 8 / NW;           // weight DMA instructions per wave per stage
    constexpr int BI = BM / 8 / NW;           // activation DMA instructions per wave per stage
    constexpr int DPS = AI + BI;              // DMAs per wave per stage (the vmcnt unit)
    constexpr int TM = BN / WM / 16;          // 16-channel subtiles per wave (v_mfma_f32_16x16x32)
    constexpr int TN = BM / WN / 16;          // 16-pixel subtiles per wave
    constexpr int STAGE = (BM + BN) * RB;
    static_assert(AI >= 1 && BI >= 1 && TM >= 1 && TN >= 1, "tile too small for 8-row DMA pieces");
    constexpr int WCH = BN / WM;                          // channels per wave
    constexpr int EPS = TM * TN / 2;                      // epilogue stores per lane
    // the ring; the statistics' cross-wave reduction reuses its first bytes after the last tile
    static_assert(NS * STAGE <= 160 * 1024 && 2 * (BM / (BM / WN)) * BN * 4 <= NS * STAGE, "LDS budget");
    __shared__ __attribute__((aligned(16))) char smem[NS * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wc = wave % WN;
    const int fc = lane >> 4, fr = lane & 15;
    const int kc = a.Kin >> 6;                // 64-deep K chunks per tap

    // ---- this workgroup's tiles: channel tile fixed per workgroup, m-tiles of its XCD's range
    const int G8 = int(gridDim.x) >> 3;
    const int xcd = int(blockIdx.x) & 7, q = int(blockIdx.x) >> 3;
    const int nt = q % a.ntiles, qq = q / a.ntiles, qstride = G8 / a.ntiles;
    const int mt_total = a.mt_pre[a.ncls];
    const int per = (mt_total + 7) >> 3;
    const int mt_lo = xcd * per + qq, mt_hi = min(xcd * per + per, mt_total);
    const int ntile = mt_lo < mt_hi ? (mt_hi - mt_lo + qstride - 1) / qstride : 0;
    const int n0 = nt * BN;
    int total = 0;                            // K steps of this workgroup's whole stream
    if (C1) total = ntile * a.KH * a.KW * kc;
    else if (a.ncls == 1) total = ntile * cls_of(a, 0).ntap * kc;
    else
        for (int t = 0; t < ntile; ++t) total += cls_of(a, cls_find(a, mt_lo + t * qstride)).ntap * kc;

    // weight DMA rows (fixed): row r of the A image = output channel n0 + r
    const uint32_t wrow_b = uint32_t(a.KH * a.KW * a.Kin) * 2u;
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.w, int64_t(a.Nout) * wrow_b);
    uint32_t a_off[AI];
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int r = (wave * AI + j) * 8 + (lane >> 3);
        const int ch = n0 + r;
        a_off[j] = ch < a.Nout ? uint32_t(ch) * wrow_b + uint32_t((lane & 7) ^ fsw128(r)) * 16u : OOB;
    }

    // per-lane fragment read offsets inside a stage (subtile i / j adds 16 * RB * i: fsw128 is 16-periodic): lane
    // (fc, fr) reads row fr of the subtile, 16-B chunk kk * 4 + fc of the 128-B row
    uint32_t offA[2], offB[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + fc;
        const int ra = wr * (BN / WM) + fr, rb = wc * (BM / WN) + fr;
        offA[kk] = uint32_t(ra * RB + ((ch ^ fsw128(ra)) << 4));
        offB[kk] = uint32_t(BN * RB + rb * RB + ((ch ^ fsw128(rb)) << 4));
    }
    bf16x8 f0a[TM], f0b[TN], f1a[TM], f1b[TN];
    auto read_frags = [&](bf16x8* fa, bf16x8* fb, int slot_off, int kk) {     // slot_off: the ring slot's byte offset
        const char* As = smem + slot_off + offA[kk];
        const char* Bs = smem + slot_off + offB[kk];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(As + i * 16 * RB);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(Bs + j * 16 * RB);
    };
    f32x4 acc[TM][TN];
    auto mma = [&](const bf16x8* fa, const bf16x8* fb) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (MODE == PF)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, fa[i]),
                                                                        __builtin_bit_cast(f16x8, fb[j]), acc[i][j], 0,
                                                                        0, 0);
                else
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
    };
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    float ssum[TM][4], ssq[TM][4];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) ssum[i][r] = ssq[i][r] = 0.f;

    Issuer<BM, BN, NW, MODE, C1, TO> is(a, wave, lane, mt_lo, qstride, ntile);
    is.start();

    // prologue: stages 0..2 in flight (stages past the stream's end fetch nothing); stage 0 landed
    // everywhere; its first-half fragments read
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        is.issue_dma(smem + s * STAGE, wres, a_off, s < total);
        is.advance();
    }
    vm_wait<(NS - 1) * DPS>();
    step_barrier();
    if (total > 0) read_frags(f0a, f0b, 0, 0);
    int boff = 0;                             // NESTED: the computing slot's byte offset (buf * STAGE)

    // compute side: one K step per iteration; tiles end inside the stream
    int ct = 0, ck = 0, cnk = C1 ? a.KH * a.KW * kc : 0, buf = 0;
    int64_t m0 = 0;
    Cls cc{};
    uint32_t t_n = 0, t_p = 0;                // divmod(m0, OHW) of the computing tile
    float inv_owc = 1.f;
    // C1: the computing tile's first pixel, advanced per tile as the issuer's
    int c_m0 = 0, c_tn = 0;
    uint32_t c_tp = 0;
    if constexpr (C1) {
        c_m0 = mt_lo * BM;
        c_tn = int(uint32_t(c_m0) / is.ohw);
        c_tp = uint32_t(c_m0) - uint32_t(c_tn) * is.ohw;
    }
    const int Mtot = a.N * int(is.ohw);
    // one K step: the second half's fragments read and the first half's MFMAs; the wait and barrier; stage g+NS's DMAs
    // into the freed slot between the second half's MFMAs; the next stage's first-half reads.  keep_epi: a tile's
    // first step after an epilogue, whose stores may stay in flight across the wait; live: stage g+NS is in the stream
    auto kstep = [&](bool keep_epi, bool live) __attribute__((always_inline)) {
        const int cur = NESTED ? boff : buf * STAGE;
        read_frags(f1a, f1b, cur, 1);
        mma(f0a, f0b);
        constexpr int MH = TM * TN;                                                 // MFMAs per half
        // stage g+1 must have landed (own DMAs); stage g+2 may stay in flight (every step issues DPS DMAs,
        // live or not, so the count is constant); in a tile's first step the previous tile's epilogue stores,
        // issued after stage g+2's pieces, may stay in flight too
        if (keep_epi) vm_wait<(NS - 2) * DPS + EPS>();
        else vm_wait<(NS - 2) * DPS>();
        step_barrier();
        // the slot of stage g is free again (every wave's reads of it returned before the barrier): stage
        // g+3's DMAs go out one at a time between the second half's MFMAs (issued in a burst they held both
        // waves of a SIMD off the MFMA pipe for the whole burst), then the next stage's first-half reads
        const int nbuf = buf == NS - 1 ? 0 : buf + 1;
        const int nboff = boff == (NS - 1) * STAGE ? 0 : boff + STAGE;
        is.issue_dma(smem + cur, wres, a_off, live);
        read_frags(f0a, f0b, NESTED ? nboff : nbuf * STAGE, 0);
        mma(f1a, f1b);
#pragma unroll
        for (int d = 0; d < DPS; ++d) {
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                     // one DMA
            __builtin_amdgcn_sched_group_barrier(0x008, MH / (DPS + 1), 0);         // MFMAs
        }
        __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);                   // next-stage reads
        __builtin_amdgcn_sched_group_barrier(0x008, MH - DPS * (MH / (DPS + 1)), 0);
        is.advance();
        if constexpr (NESTED) boff = nboff;
        else buf = nbuf;
    };
    // the tile's epilogue
    auto epilogue = [&]() __attribute__((always_inline)) {
        // epilogue: D[channel][pixel] (a lane holds 4 consecutive channels of one pixel per subtile) is
        // transposed in registers (conv_epi.h epilogue_regs: pairs of 16-pixel subtiles exchanged with
        // v_permlane16_swap), so every store is a 16-B piece of a pixel's contiguous channel run, issued as
        // buffer stores whose out-of-tile pixels fall out of range (no branches, a fixed count per tile)
        {
            const int wch0 = n0 + wr * WCH;
            const int64_t ybytes = (int64_t(a.N - 1) * a.y_bs + int64_t(a.OH) * a.OW * a.y_ld) * 2;
            const __amdgpu_buffer_rsrc_t yres = make_rsrc(a.y, ybytes);
            auto pix_off = [&](int qp) -> uint32_t {
                if constexpr (C1) {
                    // one class, stride-1 output: the output pixel IS the in-image offset (one wrap: ohw >= BM)
                    const int q = wc * (BM / WN) + qp;
                    if (c_m0 + q >= Mtot) return OOB;
                    uint32_t pix = c_tp + uint32_t(q);
                    int n = c_tn;
                    if (pix >= is.ohw) { pix -= is.ohw; ++n; }
                    return uint32_t((int64_t(n) * a.y_bs + int64_t(pix) * a.y_ld + wch0) * 2);
                }
                const int64_t m = m0 + wc * (BM / WN) + qp;
                if (m >= cc.Mc) return OOB;
                uint32_t n, pix, ci_;
                split_pix(t_n, t_p, uint32_t(wc * (BM / WN) + qp), cc.OHW, uint32_t(cc.OWc), inv_owc, n, pix, ci_);
                const int64_t opix = int64_t(ci_ * a.os + cc.py) * a.OW + int64_t(pix - ci_ * uint32_t(cc.OWc)) * a.os + cc.px;
                return uint32_t((int64_t(n) * a.y_bs + opix * a.y_ld + wch0) * 2);
            };
            auto pix_ok = [&](int qp) -> bool {
                if constexpr (C1) return c_m0 + wc * (BM / WN) + qp < Mtot;
                return m0 + wc * (BM / WN) + qp < cc.Mc;
            };
            if constexpr (EV) {
                const EvalEpi ee{e.sc, e.sh, e.act, make_rsrc(e.res, e.res ? e.res_bytes : 0), e.res != nullptr};
                auto res_off = [&](int qp) -> uint32_t {     // pix_off's C1 pixel walk on the residual view's strides
                    const int q = wc * (BM / WN) + qp;
                    if (c_m0 + q >= Mtot) return OOB;
                    uint32_t pix = c_tp + uint32_t(q);
                    int n = c_tn;
                    if (pix >= is.ohw) { pix -= is.ohw; ++n; }
                    return uint32_t((int64_t(n) * e.r_bs + int64_t(pix) * e.r_ld + wch0) * 2);
                };
                epilogue_regs_x<TM, TN>(acc, ssum, ssq, false, lane, wch0, a.Nout, yres, true, false, pix_off, pix_ok,
                                        &ee, res_off);
            } else {
                epilogue_regs<TM, TN>(acc, ssum, ssq, a.st_sum != nullptr, lane, wch0, a.Nout, yres, a.out_f32 == 2,
                                      a.accumulate != 0, pix_off, pix_ok);
            }
        }
    };
    if constexpr (NESTED) {
        int g = 0;
        for (int t = 0; t < ntile; ++t) {
            if (t > 0) {
                c_m0 += is.m_step;
                c_tn += is.step_n;
                c_tp += is.step_p;
                if (c_tp >= is.ohw) { c_tp -= is.ohw; ++c_tn; }
            }
            zero_acc();
            kstep(t > 0, g + NS < total);
            ++g;
            // the stream's last NS stages fetch nothing: live while g < glim
            const int glim = total - NS;
            for (int k = 1; k < cnk; ++k, ++g) kstep(false, g < glim);
            epilogue();
        }
    } else {
        for (int g = 0; g < total; ++g) {
            if (C1 && ck == 0) {
                if (ct > 0) {
                    c_m0 += is.m_step;
                    c_tn += is.step_n;
                    c_tp += is.step_p;
                    if (c_tp >= is.ohw) { c_tp -= is.ohw; ++c_tn; }
                }
                zero_acc();
            } else if (ck == 0) {
                const int mt = mt_lo + ct * qstride;
                const int c = cls_find(a, mt);
                cc = cls_of(a, c);
                m0 = int64_t(mt - a.mt_pre[c]) * BM;
                t_n = uint32_t(m0) / cc.OHW;
                t_p = uint32_t(m0) - t_n * cc.OHW;
                inv_owc = 1.0f / float(cc.OWc);
                cnk = cc.ntap * kc;
                zero_acc();
            }
            kstep(ck == 0 && ct > 0, g + NS < total);
            if (++ck < cnk) continue;
            ck = 0;
            ++ct;

            epilogue();
        }
    }

    if (a.st_sum) {
        // one partial row per workgroup of this channel tile: row = xcd + 8 * qq
        vm_wait<0>();
        __syncthreads();
        float (*red)[WN][BN] = reinterpret_cast<float (*)[WN][BN]>(smem);   // [sum|sq][pixel wave][channel]
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = ssum[i][r], sq = ssq[i][r];
                // over the 16 lanes holding other pixels of the same channel
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    s += __shfl_xor(s, o, 64);
                    sq += __shfl_xor(sq, o, 64);
                }
                if (fr == 0) {
                    const int cl = wr * (BN / WM) + i * 16 + fc * 4 + r;
                    red[0][wc][cl] = s;
                    red[1][wc][cl] = sq;
                }
            }
        __syncthreads();
        const int row = xcd + 8 * qq;
        for (int cl = tid; cl < BN; cl += NW * 64) {
            const int ch = n0 + cl;
            if (ch < a.Nout) {
                float ps = 0.f, pq = 0.f;
#pragma unroll
                for (int w = 0; w < WN; ++w) { ps += red[0][w][cl]; pq += red[1][w][cl]; }
                stat_store(&a.st_sum[int64_t(row) * a.Nout + ch], ps, a.fold.gamma != nullptr);
                stat_store(&a.st_sq[int64_t(row) * a.Nout + ch], pq, a.fold.gamma != nullptr);
            }
        }
        if (a.fold.gamma) bn_fold_tail<BN, NW * 64>(a.fold, a.st_sum, a.st_sq, a.Nout, nt, int(gridDim.x) / a.ntiles, smem);
    }
}

// tile configurations (PipePlan::cfg): 0 the 256 x 128 tile, 1 the 256 x 64 tile.  Training runs 256 x 128 on 16 waves
// of 32 x 64 (four per SIMD, 127 VGPRs): same staging and LDS as 8 waves of 64 x 64, 1.5x the fragment reads, but while
// some waves of a SIMD issue their DMA pieces or wait at the barrier others issue MFMAs — same-process A/B against
// 8 waves: fwd / dgrad 0-7 % faster on every layer measured (1x1 80x80 192->256 -6.8 / -6.2 %, 3x3 40x40 128->128
// -3.3 / -6.7 %, stride-2 80x80 equal).  The 8-wave 256 x 128 tile remains only as the eval instance of cfg 0: the
// 16-wave tile's 127 VGPRs leave no room for the eval epilogue at four waves per SIMD.  256 x 64 runs on 8 waves of
// 64 x 32 everywhere.  (256 x 256 / 512 x 128 tiles on 8 waves of 128 x 64 need 128 accumulator registers per lane and
// spilled 213-439 VGPRs at the 256-register cap of two waves per SIMD: not kept.)
struct Cfg {
    int bm, bn;
};
constexpr Cfg kCfg[] = {{256, 128}, {256, 64}};

// the tap-innermost K order (Issuer TO 1) where it measured faster: stride-2 3x3 forwards reading maps >= 128 wide (op 6,
// 128 -> 128 at 160x160 -> 80x80: -12 % time, -27 % HBM fetch; profiles/r06/pipe_taporder_ab.txt) — there one tile's
// input over every channel chunk overflows its share of the XCD's L2, one chunk's does not.  Elsewhere it measured
// 0..+5 % slower (a tap_setup per K step, and the footprint fits L2 either way)
inline bool tap_inner(const PipeArgs& a) { return a.stride == 2 && a.KH == 3 && a.GW >= 128; }

// the instances the library ships, all of them: per training tile the forward and the data gradient on the generic
// (class-search, flat loop) and the single-class (C1, nested loop) control paths, the C1 forward also tap-innermost;
// per tile one eval instance (C1 forward, flat loop)
enum Inst { FWD_GEN, FWD_C1, FWD_C1_TAP, DGRAD_GEN, DGRAD_C1, EVAL };

void launch(int cfg, Inst inst, const PipeArgs& a, const EvalArgs& e, int grid, hipStream_t st) {
    const dim3 g(grid), w16(1024), w8(512);
    if (cfg == 0) {
        switch (inst) {  //                 BM   BN  WM WN MODE  C1     EV     NESTED TO
            case FWD_GEN:    conv_pipe_kernel<256, 128, 4, 4, PF, false, false, false, 0><<<g, w16, 0, st>>>(a, e); break;
            case FWD_C1:     conv_pipe_kernel<256, 128, 4, 4, PF, true,  false, true,  0><<<g, w16, 0, st>>>(a, e); break;
            case FWD_C1_TAP: conv_pipe_kernel<256, 128, 4, 4, PF, true,  false, true,  1><<<g, w16, 0, st>>>(a, e); break;
            case DGRAD_GEN:  conv_pipe_kernel<256, 128, 4, 4, PD, false, false, false, 0><<<g, w16, 0, st>>>(a, e); break;
            case DGRAD_C1:   conv_pipe_kernel<256, 128, 4, 4, PD, true,  false, true,  0><<<g, w16, 0, st>>>(a, e); break;
            case EVAL:       conv_pipe_kernel<256, 128, 2, 4, PF, true,  true,  false, 0><<<g, w8, 0, st>>>(a, e); break;
        }
    } else {
        switch (inst) {
            case FWD_GEN:    conv_pipe_kernel<256, 64, 1, 8, PF, false, false, false, 0><<<g, w8, 0, st>>>(a, e); break;
            case FWD_C1:     conv_pipe_kernel<256, 64, 1, 8, PF, true,  false, true,  0><<<g, w8, 0, st>>>(a, e); break;
            case FWD_C1_TAP: conv_pipe_kernel<256, 64, 1, 8, PF, true,  false, true,  1><<<g, w8, 0, st>>>(a, e); break;
            case DGRAD_GEN:  conv_pipe_kernel<256, 64, 1, 8, PD, false, false, false, 0><<<g, w8, 0, st>>>(a, e); break;
            case DGRAD_C1:   conv_pipe_kernel<256, 64, 1, 8, PD, true,  false, true,  0><<<g, w8, 0, st>>>(a, e); break;
            case EVAL:       conv_pipe_kernel<256, 64, 1, 8, PF, true,  true,  false, 0><<<g, w8, 0, st>>>(a, e); break;
        }
    }
}

}  // namespace

PipePlan pipe_plan(const ym_conv_desc* d, int dgrad, const ConvPolicy& pol) {
    PipePlan p{};
    const int mode = pol.pipe >= 0 ? pol.pipe : 3;
    if (!d || mode == 0) return p;
    const ConvSide s = side(d, dgrad);
    const int kin = s.kin, nout = s.nout, os = s.os, OH = s.OH, OW = s.OW;
    if (kin % 64 != 0 || nout % 8 != 0) return p;
    if (d->k != 3 && d->k != 1) return p;
    if (d->stride != 1 && d->stride != 2) return p;
    if (dgrad && d->k == 1 && d->stride == 2) return p;
    if (s.in_ld % 8 || s.in_bs % 8 || s.out_ld % 4 || s.out_bs % 4) return p;
    if (!dgrad && d->out_f32 == 1) return p;       // Detect's fp32 bias convs stay on conv.hip
    // rule 1: only where it measured faster in isolation (tools/pipe_check.py): >= 128 output channels
    // (the 256 x 128 tile) and no stride-2 data gradient
    if (mode == 1 && (nout < 128 || os == 2)) return p;
    // 3: the wider rule (A/B runs): every 1x1, and 3x3 with >= 128 output channels or (forward) >= 128
    // input channels, at >= 256 tiles; never the stride-2 data gradient
    if (mode == 3 && (os == 2 || (d->k == 3 && nout < 128 && (dgrad || kin < 128)))) return p;
    // split_pix: in-image pixel indices as exact floats, row estimates within one of the truth
    if (int64_t(OH) * OW >= (int64_t(1) << 24) || OH >= (1 << 16)) return p;
    const int64_t M = pol.select_n(d) * ((OH + os - 1) / os) * ((OW + os - 1) / os) * os * os;
    p.cfg = nout >= 128 ? 0 : 1;
    const int bm = kCfg[p.cfg].bm, bn = kCfg[p.cfg].bn;
    const int ntiles = (nout + bn - 1) / bn;
    const int64_t tiles = (M / bm) * ntiles;
    // enough tiles to keep every CU busy for several tiles (tail imbalance), else conv.hip's kernels
    if (tiles < int64_t(mode >= 2 ? 256 : 1024)) return p;
    // 32-bit buffer offsets relative to a tile's first image
    if (s.in_bs * 2 * (256 / std::max<int64_t>(int64_t(OH / os) * (OW / os), 1) + 2) >= (int64_t(1) << 31)) return p;
    int grid = 256;
    const int unit = 8 * ntiles;
    grid = (grid / unit) * unit;
    if (grid < unit) return p;
    p.grid = grid;
    p.rows = grid / ntiles;
    p.ok = 1;
    return p;
}

// operands, views and map geometry of d's forward (dgrad 0) or data gradient
static void pipe_geometry(PipeArgs& a, const ym_conv_desc* d, int dgrad, const uint16_t* x, const uint16_t* w, void* y) {
    const ConvSide s = side(d, dgrad);
    a.x = x; a.x_bs = s.in_bs; a.x_ld = s.in_ld;
    a.y = y; a.y_bs = s.out_bs; a.y_ld = s.out_ld;
    a.GH = s.GH; a.GW = s.GW; a.Kin = s.kin;
    a.OH = s.OH; a.OW = s.OW; a.Nout = s.nout;
    a.os = s.os;
    a.w = w;
    a.KH = d->k; a.KW = d->k; a.stride = d->stride; a.pad = d->pad; a.N = d->n;
}

int pipe_launch(const PipePlan& p, const ym_conv_desc* d, int dgrad, const uint16_t* x, const uint16_t* w, void* y,
                float* st_sum, float* st_sq, hipStream_t st, const ym_bn_fold* fold) {
    PipeArgs a{};
    const int bm = kCfg[p.cfg].bm, bn = kCfg[p.cfg].bn;
    pipe_geometry(a, d, dgrad, x, w, y);
    a.out_f32 = dgrad ? 0 : d->out_f32;
    a.st_sum = st_sum; a.st_sq = st_sq;
    a.accumulate = d->accumulate;
    a.ntiles = (a.Nout + bn - 1) / bn;
    a.ncls = a.os == 2 ? 4 : 1;
    int acc = 0;
    for (int c = 0; c < a.ncls; ++c) {
        const int py = a.os == 2 ? (c >> 1) : 0, px = a.os == 2 ? (c & 1) : 0;
        const int64_t ohc = (a.OH - py + a.os - 1) / a.os, owc = (a.OW - px + a.os - 1) / a.os;
        a.mt_pre[c] = acc;
        acc += int((int64_t(a.N) * ohc * owc + bm - 1) / bm);
    }
    a.mt_pre[a.ncls] = acc;
    if (!dgrad && st_sum) a.fold = bn_fold_args(fold);
    // the single-class path: one output class on maps of >= BM pixels
    const bool c1 = a.ncls == 1 && int64_t(a.OH) * a.OW >= bm;
    const Inst inst = dgrad ? (c1 ? DGRAD_C1 : DGRAD_GEN) : !c1 ? FWD_GEN : tap_inner(a) ? FWD_C1_TAP : FWD_C1;
    launch(p.cfg, inst, a, EvalArgs{}, p.grid, st);
    return YM_OK;
}

bool pipe_eval_ok(const PipePlan& p, const ym_conv_desc* d) {
    // the eval instance is the single-class (C1) forward: maps of >= BM pixels, the shipped control path
    return p.ok && int64_t(d->oh) * d->ow >= kCfg[p.cfg].bm && d->out_f32 == 2 && !d->accumulate;
}

int pipe_launch_eval(const PipePlan& p, const ym_conv_desc* d, const uint16_t* x, const uint16_t* w, uint16_t* y,
                     const EvalArgs& e, hipStream_t st) {
    if (!pipe_eval_ok(p, d)) return 1;
    PipeArgs a{};
    pipe_geometry(a, d, 0, x, w, y);
    a.out_f32 = 2;
    const int bm = kCfg[p.cfg].bm, bn = kCfg[p.cfg].bn;
    a.ntiles = (a.Nout + bn - 1) / bn;
    a.ncls = 1;
    a.mt_pre[0] = 0;
    a.mt_pre[1] = int((int64_t(a.N) * a.OH * a.OW + bm - 1) / bm);
    launch(p.cfg, EVAL, a, e, p.grid, st);
    return 0;
}

}  // namespace ym
