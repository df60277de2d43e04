// Decode + greedy NMS (class-agnostic as the reference's, or class-aware with a detection cap: DESIGN §18), one
// workgroup per image (gfx950).
//
// Replaces decode_predictions_for_metrics / nms_simple / calculate_iou_batch_simple
// (/root/reference/yolo_scratch_cuda/train_yolo11_cuda.py:265-437).  Bit-exact
// with the reference on tie-free scores: the IoU is evaluated in the same fp32
// op order and this file is compiled with -ffp-contract=off.
//
// Pipeline per call
//   1. rowmax kernel      grid over rows: max/argmax over the C class scores,
//                         `> conf` flag, xywh -> xyxy            (:296-329)
//   2. nms_image kernel   one 1024-thread workgroup per image:
//        a. order-preserving compaction of flagged rows (block scan)
//        b. bitonic sort of 64-bit keys (~score, filtered index): score
//           descending, index ascending (the reference's argsort is unstable;
//           golden inputs are tie-free)                          (:377)
//        c. greedy loop: the head box is broadcast through LDS, every thread
//           tests the boxes it holds in registers, drops IoU > thr, and a
//           block min-reduction finds the next alive head        (:380-397)
//        d. write kept boxes / (img_w, img_h) clamped to [0,1]          (:342-350)
#include <cstdlib>

#include "common.h"
#include "tile.h"

namespace ym {
namespace {

constexpr int NMS_THREADS = 1024;
constexpr int NMS_WAVES = NMS_THREADS / 64;
constexpr int SORT_LDS_KEYS = 16384;   // 128 KiB of keys in LDS
constexpr int REG_ITEMS = 8;           // boxes held in registers per thread (K <= 8192)

struct Ws {
    float4* box;      // [B][N] xyxy of every row
    float* score;     // [B][N]
    int32_t* label;   // [B][N]
    int32_t* flag;    // [B][N]
    int32_t* frow;    // [B][N] filtered index -> row
    uint64_t* keys;   // [B][KP] (global sort path; sorted keys of the bitmask path)
    float4* sbox;     // [B][N] boxes in sorted order      (bitmask path)
    uint64_t* mask;   // [B][N][Wn] suppression bitmask    (bitmask path)
    int32_t* kcount;  // [B] candidates after the filter   (bitmask path)
    int32_t* slabel;  // [B][N] labels in sorted order     (bitmask path of the class-aware entry points only)
};

// Bitmask path (small batches: one image is too little work for one workgroup's greedy loop):
// sort per image, then the upper-triangular IoU > thr bitmask of the sorted candidates over the
// whole GPU, then a chunked greedy scan per image.  Needs the [64][Wn] chunk double buffer in LDS.
constexpr int64_t BM_MAX_B = 8;
constexpr int64_t BM_MAX_WN = 150;            // N <= 9600 (640x640: 8400 anchors)
inline bool bitmask_path(int64_t B, int64_t N) { return B <= BM_MAX_B && (N + 63) / 64 <= BM_MAX_WN && N >= 128; }

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

inline int64_t pow2_at_least(int64_t x) {
    int64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

inline size_t bitmask_bytes(int64_t B, int64_t N) {
    if (!bitmask_path(B, N)) return 0;
    const size_t n = size_t(B) * size_t(N), wn = size_t((N + 63) / 64);
    return align256(n * 16) + align256(n * wn * 8) + align256(size_t(B) * 4);
}

// cls: the class-aware entry points' layout, the class-agnostic one plus the sorted labels at its end
inline Ws carve(void* base, int64_t B, int64_t N, bool cls = false) {
    char* p = static_cast<char*>(base);
    size_t n = size_t(B) * size_t(N);
    Ws w;
    w.box = reinterpret_cast<float4*>(p);   p += align256(n * sizeof(float4));
    w.score = reinterpret_cast<float*>(p);  p += align256(n * sizeof(float));
    w.label = reinterpret_cast<int32_t*>(p); p += align256(n * sizeof(int32_t));
    w.flag = reinterpret_cast<int32_t*>(p); p += align256(n * sizeof(int32_t));
    w.frow = reinterpret_cast<int32_t*>(p); p += align256(n * sizeof(int32_t));
    w.keys = reinterpret_cast<uint64_t*>(p); p += align256(size_t(B) * pow2_at_least(N) * 8);
    w.sbox = nullptr; w.mask = nullptr; w.kcount = nullptr; w.slabel = nullptr;
    if (bitmask_path(B, N)) {
        const size_t wn = size_t((N + 63) / 64);
        w.sbox = reinterpret_cast<float4*>(p);   p += align256(n * 16);
        w.mask = reinterpret_cast<uint64_t*>(p); p += align256(n * wn * 8);
        w.kcount = reinterpret_cast<int32_t*>(p); p += align256(size_t(B) * 4);
        if (cls) w.slabel = reinterpret_cast<int32_t*>(p);
    }
    return w;
}

inline size_t ws_bytes(int64_t B, int64_t N) {
    size_t n = size_t(B) * size_t(N);
    return align256(n * 16) + 4 * align256(n * 4) + align256(size_t(B) * pow2_at_least(N) * 8) + bitmask_bytes(B, N) +
           256;
}

inline size_t ws_bytes_cls(int64_t B, int64_t N) {
    return ws_bytes(B, N) + (bitmask_path(B, N) ? align256(size_t(B) * size_t(N) * 4) : 0);
}

// IoU in the reference's op order (train_yolo11_cuda.py:418-435).
__device__ __forceinline__ float iou_ref(float4 a, float4 b) {
    float x1 = fmaxf(a.x, b.x), y1 = fmaxf(a.y, b.y);
    float x2 = fminf(a.z, b.z), y2 = fminf(a.w, b.w);
    float iw = x2 - x1, ih = y2 - y1;
    iw = iw < 0.0f ? 0.0f : iw;
    ih = ih < 0.0f ? 0.0f : ih;
    float inter = iw * ih;
    float a1 = (a.z - a.x) * (a.w - a.y);
    float a2 = (b.z - b.x) * (b.w - b.y);
    float uni = a1 + a2;
    uni = uni - inter;
    return inter / (uni + 1e-6f);
}

// The match value of greedy merging (ym_decode_nmm_tiles).  YM_MATCH_IOU is iou_ref itself; YM_MATCH_IOS
// divides the same `inter` by the smaller area: a box cut by a tile border matches its whole twin at ~1 whatever its
// share of the whole.
template <int METRIC>
__device__ __forceinline__ float match_ref(float4 a, float4 b) {
    if constexpr (METRIC == YM_MATCH_IOU) {
        return iou_ref(a, b);
    } else {
        float x1 = fmaxf(a.x, b.x), y1 = fmaxf(a.y, b.y);
        float x2 = fminf(a.z, b.z), y2 = fminf(a.w, b.w);
        float iw = x2 - x1, ih = y2 - y1;
        iw = iw < 0.0f ? 0.0f : iw;
        ih = ih < 0.0f ? 0.0f : ih;
        float inter = iw * ih;
        float a1 = (a.z - a.x) * (a.w - a.y);
        float a2 = (b.z - b.x) * (b.w - b.y);
        return inter / (fminf(a1, a2) + 1e-6f);
    }
}

// Order-preserving integer image of a float (unsigned compare = float compare; -0 sorts below +0) and its inverse:
// what the union pass of the MERGE instances takes integer min / max atomics on
__device__ __forceinline__ uint32_t ord_bits(float s) {
    uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ uint32_t desc_bits(float s) {
    uint32_t u = __float_as_uint(s);
    uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending-order bits
    return ~ord;                                                  // descending
}

// ---------------------------------------------------------------- stage 1
// thread per row (C small) — max/argmax with the first maximal index winning; cs: the stride between a row's
// elements (1: row-major rows; A: the anchor-major view of the (B, 4+nc, A) eval output, read coalesced across rows)
__global__ void rowmax_thread_kernel(const float* __restrict__ pred, int64_t B, int64_t N, int64_t C,
                                     int64_t rs, int64_t is, int64_t cs, float conf, Ws w) {
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= B * N) return;
    int64_t b = i / N, n = i - b * N;
    const float* r = pred + b * is + n * rs;
    float mx = r[4 * cs];
    int lab = 0;
    for (int64_t c = 1; c < C; ++c) {
        float v = r[(4 + c) * cs];
        if (v > mx) { mx = v; lab = int(c); }
    }
    float x = r[0], y = r[cs], hw = r[2 * cs] / 2.0f, hh = r[3 * cs] / 2.0f;
    w.box[i] = make_float4(x - hw, y - hh, x + hw, y + hh);
    w.score[i] = mx;
    w.label[i] = lab;
    w.flag[i] = (mx > conf) ? 1 : 0;
}

// wave per row (C large, e.g. the literal (B, 4+nc, A) eval layout)
__global__ void rowmax_wave_kernel(const float* __restrict__ pred, int64_t B, int64_t N, int64_t C,
                                   int64_t rs, int64_t is, int64_t cs, float conf, Ws w) {
    int64_t i = int64_t(blockIdx.x) * (blockDim.x / 64) + threadIdx.x / 64;
    int lane = threadIdx.x & 63;
    if (i >= B * N) return;
    int64_t b = i / N, n = i - b * N;
    const float* r = pred + b * is + n * rs;
    float mx = -INFINITY;
    int64_t lab = INT64_MAX;
    for (int64_t c = lane; c < C; c += 64) {
        float v = r[(4 + c) * cs];
        if (v > mx || (v == mx && c < lab)) { mx = v; lab = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float om = __shfl_xor(mx, o, 64);
        int64_t ol = __shfl_xor(lab, o, 64);
        if (om > mx || (om == mx && ol < lab)) { mx = om; lab = ol; }
    }
    if (lane == 0) {
        float x = r[0], y = r[cs], hw = r[2 * cs] / 2.0f, hh = r[3 * cs] / 2.0f;
        w.box[i] = make_float4(x - hw, y - hh, x + hw, y + hh);
        w.score[i] = mx;
        w.label[i] = int32_t(lab);
        w.flag[i] = (mx > conf) ? 1 : 0;
    }
}

// direct candidates (nms_simple): every box is a candidate; labels (ym_nms_cls, may be null): their low words go
// with the candidate, the greedy kernel compares the caller's 64-bit values
__global__ void direct_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                              const int64_t* __restrict__ labels, int64_t n, Ws w) {
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    w.box[i] = boxes[i];
    w.score[i] = scores[i];
    w.label[i] = labels ? int32_t(labels[i]) : 0;
    w.flag[i] = 1;
}

// ---------------------------------------------------------------- stage 2 helpers
__device__ int block_excl_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wv] = x;
    __syncthreads();
    if (wv == 0) {
        int s = lane < NMS_WAVES ? sh[lane] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            int y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane < NMS_WAVES) sh[lane] = s;
    }
    __syncthreads();
    int before = (wv > 0 ? sh[wv - 1] : 0) + x - v;
    total = sh[NMS_WAVES - 1];
    __syncthreads();
    return before;
}

__device__ int block_min(int v, int* sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    int r = sh[0];
#pragma unroll
    for (int k = 1; k < NMS_WAVES; ++k) r = min(r, sh[k]);
    __syncthreads();
    return r;
}

template <bool IN_LDS>
__device__ void bitonic(uint64_t* keys, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += NMS_THREADS) {
                int l = i ^ j;
                if (l > i) {
                    uint64_t a = keys[i], c = keys[l];
                    bool up = (i & k) == 0;
                    if ((a > c) == up) { keys[i] = c; keys[l] = a; }
                }
            }
            if (IN_LDS) __syncthreads();
            else { __threadfence_block(); __syncthreads(); }
        }
    }
}

// ---------------------------------------------------------------- stage 2
// CLS: class-aware suppression (a candidate is tested against heads of its own label only; labs[row] of type LT is
// the label compared, equality only) and the max_det cap (0: none).  The CLS = false instances ignore both.
//
// Greedy merging (ym_decode_nmm_tiles; launched at clamp_norm = 0, so the union is taken over the boxes as
// stored).  METRIC: the match value (match_ref).  MERGE: every absorbed candidate remembers the kept slot of the head
// that absorbed it (slot[] beside alive[] in the register form, the galive word in the large-K form); after the loop
// one parallel pass counts them into out_merged (may be null) and, with do_union, folds their boxes into the head's
// out_boxes row by integer min / max atomics on ord_bits images.  Nothing is reduced inside the serial loop, and min,
// max and integer adds do not depend on the order in which lanes arrive.  The METRIC = IoU, MERGE = false instances
// are the suppression kernels of before, instruction for instruction.
//
// MEAN (ym_decode_nmw_tiles; MERGE instances only, do_union unused): the head's out_boxes row becomes the
// score-weighted mean of the head and what it absorbed, in fixed point.  The thread that writes kept row k stores the
// head's own terms (q, q c_x1, q c_y1, q c_x2, q c_y2) into acc[5 (base + k) ..]; the absorbed candidates add theirs
// by 64-bit integer atomics in the pass that counts out_merged; a head whose weight sum is still its own q absorbed
// nothing (every q >= 1) and keeps the box as stored.  Integer sums do not depend on the order of arrival.
constexpr int NMW_QS = 12;                 // score -> weight q in [1, 2^12]
constexpr int NMW_CS = 5;                  // coordinate -> c in 1/32 pixel, |c| <= 2^25
constexpr float NMW_CMAX = 1048576.0f;     // |coord| clamp, 2^20: |q c| <= 2^37, and R < 2^26 terms stay below 2^63
constexpr int64_t NMW_MAX_R = int64_t(1) << 26;

__device__ __forceinline__ long long nmw_q(float score) {
    const long long q = llrintf(fminf(fmaxf(score, 0.0f), 1.0f) * float(1 << NMW_QS));
    return q < 1 ? 1 : q;
}
__device__ __forceinline__ long long nmw_c(float v) {
    return llrintf(fminf(fmaxf(v, -NMW_CMAX), NMW_CMAX) * float(1 << NMW_CS));
}

template <bool SORT_ONLY, bool CLS = false, typename LT = int32_t, int METRIC = YM_MATCH_IOU, bool MERGE = false,
          bool MEAN = false>
__global__ void __launch_bounds__(NMS_THREADS)
nms_image_kernel(int64_t N, int64_t KP, float iou_thr, float img_w, float img_h, int clamp_norm, Ws w,
                 int32_t* __restrict__ out_count, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                 int64_t* __restrict__ out_labels, int64_t* __restrict__ out_index,
                 const LT* __restrict__ labs = nullptr, int max_det = 0, int32_t* __restrict__ out_merged = nullptr,
                 int do_union = 0, long long* __restrict__ acc = nullptr) {
    static_assert(!MEAN || MERGE, "the mean is formed in the MERGE pass");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* skeys = reinterpret_cast<uint64_t*>(smem);            // SORT_LDS_KEYS
    __shared__ int sh[NMS_WAVES + 1];
    __shared__ float4 head_box;
    __shared__ LT head_lab;
    __shared__ int kept_pos_count;

    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t base = b * N;

    // a. order-preserving compaction (chunk per thread)
    const int cpt = int((N + NMS_THREADS - 1) / NMS_THREADS);
    const int64_t r0 = int64_t(tid) * cpt;
    int cnt = 0;
    for (int k = 0; k < cpt; ++k) {
        int64_t r = r0 + k;
        if (r < N) cnt += w.flag[base + r];
    }
    int K;
    int off = block_excl_scan(cnt, sh, K);
    for (int k = 0; k < cpt; ++k) {
        int64_t r = r0 + k;
        if (r < N && w.flag[base + r]) w.frow[base + off++] = int32_t(r);
    }
    __syncthreads();
    if (K == 0) {
        if (tid == 0) {
            out_count[b] = 0;
            if (SORT_ONLY) w.kcount[b] = 0;
        }
        return;
    }
    if constexpr (SORT_ONLY) {        // bitmask path: the sort runs over the whole GPU (nms_rank_kernel)
        for (int64_t r = tid; r < N; r += NMS_THREADS) w.flag[base + r] = 0;   // rank counters
        if (tid == 0) w.kcount[b] = K;
        return;
    }

    // b. sort (score desc, filtered index asc)
    int P = 1;
    while (P < K) P <<= 1;
    const bool lds_sort = P <= SORT_LDS_KEYS;
    uint64_t* keys = lds_sort ? skeys : (w.keys + b * KP);   // KP >= P
    for (int i = tid; i < P; i += NMS_THREADS) {
        uint64_t key = ~0ull;
        if (i < K) key = (uint64_t(desc_bits(w.score[base + w.frow[base + i]])) << 32) | uint32_t(i);
        keys[i] = key;
    }
    __syncthreads();
    // the LDS image is sorted through the __shared__ pointer itself (ds_ instructions); the generic
    // `keys` pointer would compile to flat loads/stores, ~10x slower for the 91 bitonic stages
    if (lds_sort) bitonic<true>(skeys, P);
    else bitonic<false>(w.keys + b * KP, P);

    // c. greedy loop; sorted position s -> filtered index f = keys[s] low bits
    float4 mybox[REG_ITEMS];
    LT mylab[REG_ITEMS];
    bool alive[REG_ITEMS];
    [[maybe_unused]] int slot[REG_ITEMS];     // MERGE: the kept slot that absorbed the candidate, -1: none
    const bool in_regs = K <= REG_ITEMS * NMS_THREADS;
    if (in_regs) {
#pragma unroll
        for (int it = 0; it < REG_ITEMS; ++it) {
            int s = tid + it * NMS_THREADS;
            alive[it] = s < K;
            if constexpr (MERGE) slot[it] = -1;
            if constexpr (CLS) {          // the CLS loop evaluates whole waves: no indeterminate operand
                mybox[it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                mylab[it] = LT(0);
            }
            if (s < K) {
                int f = int(uint32_t(keys[s]));
                mybox[it] = w.box[base + w.frow[base + f]];
                if constexpr (CLS) mylab[it] = labs[base + w.frow[base + f]];
            }
        }
    }
    // alive flags for the large-K path live in out_index scratch as bytes: reuse w.flag (now free)
    // (MERGE: 1 alive, -(k + 1) absorbed by kept slot k)
    int32_t* galive = w.flag + base;
    if (!in_regs) {
        for (int s = tid; s < K; s += NMS_THREADS) galive[s] = 1;
    }
    if (tid == 0) kept_pos_count = 0;
    __syncthreads();

    int head = 0;
    int nkept = 0;                    // = kept_pos_count, in a register of every thread (one kept box per turn)
    while (head < K && !(CLS && max_det > 0 && nkept >= max_det)) {
        // record + broadcast the head box: from the registers of the thread that holds sorted
        // position `head` (no dependent global loads on the serial path), or from HBM for K > 8192
        if (in_regs) {
            if (tid == (head & (NMS_THREADS - 1))) {
                const int hit = head / NMS_THREADS;
#pragma unroll
                for (int it = 0; it < REG_ITEMS; ++it)
                    if (it == hit) {
                        head_box = mybox[it];
                        if constexpr (CLS) head_lab = mylab[it];
                    }
            }
        } else if (tid == 0) {
            int f = int(uint32_t(keys[head]));
            head_box = w.box[base + w.frow[base + f]];
            if constexpr (CLS) head_lab = labs[base + w.frow[base + f]];
        }
        if (tid == 0) {
            out_index[base + kept_pos_count] = head;   // sorted position for now
            kept_pos_count++;
        }
        __syncthreads();
        const float4 hb = head_box;
        [[maybe_unused]] LT hl = LT(0);
        if constexpr (CLS) hl = head_lab;
        ++nkept;
        int next = INT32_MAX;
        if (in_regs) {
#pragma unroll
            for (int it = 0; it < REG_ITEMS; ++it) {
                int s = tid + it * NMS_THREADS;
                if constexpr (CLS) {
                    // the label compare comes first, and the branch is on the whole wave: a wave none of whose
                    // live boxes has the head's label computes no IoU, and no lane diverges around the division
                    const bool live = alive[it] && s > head;
                    const bool test = live && mylab[it] == hl;
                    bool sup = false;
                    if (__builtin_amdgcn_ballot_w64(test) != 0) {
                        sup = test && !(match_ref<METRIC>(hb, mybox[it]) <= iou_thr);
                        if constexpr (MERGE) slot[it] = sup ? nkept - 1 : slot[it];   // (only where a lane was tested)
                    }
                    alive[it] = live && !sup;
                    if (alive[it]) next = min(next, s);
                } else if (alive[it] && s > head) {
                    float v = match_ref<METRIC>(hb, mybox[it]);
                    if (!(v <= iou_thr)) {                      // reference keeps IoU <= thr (:396)
                        alive[it] = false;
                        if constexpr (MERGE) slot[it] = nkept - 1;
                    } else next = min(next, s);
                } else if (s <= head) {
                    alive[it] = false;
                }
            }
        } else {
            for (int s = tid; s < K; s += NMS_THREADS) {
                if (s > head && (MERGE ? galive[s] > 0 : galive[s] != 0)) {
                    int f = int(uint32_t(keys[s]));
                    const int32_t dead = MERGE ? -nkept : 0;
                    if constexpr (CLS) {
                        const int64_t row = base + w.frow[base + f];
                        // the label first: a candidate of another label loads no box and computes no IoU.  (Loading
                        // the box beside the label, unconditionally, saves one dependent load where the labels
                        // match and was 7 % faster with one class, but 1.3x slower with 5 classes and 2.1x with 80:
                        // DESIGN §18.)
                        if (labs[row] == hl && !(match_ref<METRIC>(hb, w.box[row]) <= iou_thr)) galive[s] = dead;
                        else next = min(next, s);
                    } else {
                        float v = match_ref<METRIC>(hb, w.box[base + w.frow[base + f]]);
                        if (!(v <= iou_thr)) galive[s] = dead;
                        else next = min(next, s);
                    }
                }
            }
        }
        head = block_min(next, sh);
    }
    __syncthreads();

    // d. outputs
    const int nk = kept_pos_count;
    for (int k = tid; k < nk; k += NMS_THREADS) {
        int s = int(out_index[base + k]);
        int f = int(uint32_t(keys[s]));
        int64_t row = base + w.frow[base + f];
        float4 bx = w.box[row];
        if (clamp_norm) {
            bx.x = fminf(fmaxf(bx.x / img_w, 0.0f), 1.0f);
            bx.y = fminf(fmaxf(bx.y / img_h, 0.0f), 1.0f);
            bx.z = fminf(fmaxf(bx.z / img_w, 0.0f), 1.0f);
            bx.w = fminf(fmaxf(bx.w / img_h, 0.0f), 1.0f);
        }
        int64_t o = base + k;
        if constexpr (MEAN) {                   // the head's own terms; the absorbed add theirs below
            const long long q = nmw_q(w.score[row]);
            long long* a = acc + 5 * o;
            a[0] = q, a[1] = q * nmw_c(bx.x), a[2] = q * nmw_c(bx.y), a[3] = q * nmw_c(bx.z), a[4] = q * nmw_c(bx.w);
        }
        if (!MEAN && MERGE && do_union)         // the union pass works on the order-preserving integer images
            reinterpret_cast<uint4*>(out_boxes)[o] = make_uint4(ord_bits(bx.x), ord_bits(bx.y), ord_bits(bx.z),
                                                                ord_bits(bx.w));
        else
            reinterpret_cast<float4*>(out_boxes)[o] = bx;
        out_scores[o] = w.score[row];
        out_labels[o] = w.label[row];
        out_index[o] = f;
        if constexpr (MERGE)
            if (out_merged) out_merged[o] = 0;
    }
    if (tid == 0) out_count[b] = nk;

    // e. MERGE: every absorbed candidate adds one to its head's count and folds its box into its head's row.  The rows
    // were written above by other threads of this workgroup: the barrier orders those stores (the vector cache writes
    // through) before the atomics, which run in L2, and the rows are read back by agent-scope atomic loads, never
    // through this CU's vector cache.  A coordinate that cannot move
    // its head's (min and max are monotone: the test may use a stale value safely) costs a load, not an atomic.
    if constexpr (MEAN) {
        __syncthreads();
        using ull = unsigned long long;
        // (two's complement: the unsigned add is the signed one)
        auto fold = [&](int k, float4 bx, float score) {      // 0 <= k < nk: the slot of a kept head
            if (out_merged) atomicAdd(&out_merged[base + k], 1);
            const long long q = nmw_q(score);
            ull* a = reinterpret_cast<ull*>(acc + 5 * (base + k));
            atomicAdd(a + 0, ull(q));
            atomicAdd(a + 1, ull(q * nmw_c(bx.x)));
            atomicAdd(a + 2, ull(q * nmw_c(bx.y)));
            atomicAdd(a + 3, ull(q * nmw_c(bx.z)));
            atomicAdd(a + 4, ull(q * nmw_c(bx.w)));
        };
        if (in_regs) {
#pragma unroll
            for (int it = 0; it < REG_ITEMS; ++it)
                if (slot[it] >= 0) {
                    const int f = int(uint32_t(keys[tid + it * NMS_THREADS]));
                    fold(slot[it], mybox[it], w.score[base + w.frow[base + f]]);
                }
        } else {
            for (int s = tid; s < K; s += NMS_THREADS) {
                const int32_t g = galive[s];
                if (g < 0) {
                    const int64_t row = base + w.frow[base + int(uint32_t(keys[s]))];
                    fold(-g - 1, w.box[row], w.score[row]);
                }
            }
        }
        __syncthreads();
        auto cur = [&](const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        for (int k = tid; k < nk; k += NMS_THREADS) {
            const int64_t o = base + k;
            const long long* a = acc + 5 * o;
            const long long sq = cur(a);
            if (sq == nmw_q(out_scores[o])) continue;           // absorbed nothing: the stored box stands
            const double den = double(sq) * double(1 << NMW_CS);
            reinterpret_cast<float4*>(out_boxes)[o] =
                make_float4(float(double(cur(a + 1)) / den), float(double(cur(a + 2)) / den),
                            float(double(cur(a + 3)) / den), float(double(cur(a + 4)) / den));
        }
    } else if constexpr (MERGE) {
        if (!do_union && !out_merged) return;
        __syncthreads();
        uint32_t* ub = reinterpret_cast<uint32_t*>(out_boxes) + base * 4;
        auto cur = [&](const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        auto fold = [&](int k, float4 bx) {      // 0 <= k < nk: the slot of a kept head
            if (out_merged) atomicAdd(&out_merged[base + k], 1);
            if (do_union) {
                uint32_t* u = ub + 4 * int64_t(k);
                const uint32_t x1 = ord_bits(bx.x), y1 = ord_bits(bx.y), x2 = ord_bits(bx.z), y2 = ord_bits(bx.w);
                if (x1 < cur(u + 0)) atomicMin(u + 0, x1);
                if (y1 < cur(u + 1)) atomicMin(u + 1, y1);
                if (x2 > cur(u + 2)) atomicMax(u + 2, x2);
                if (y2 > cur(u + 3)) atomicMax(u + 3, y2);
            }
        };
        if (in_regs) {
#pragma unroll
            for (int it = 0; it < REG_ITEMS; ++it)
                if (slot[it] >= 0) fold(slot[it], mybox[it]);
        } else {
            for (int s = tid; s < K; s += NMS_THREADS) {
                const int32_t g = galive[s];
                if (g < 0) fold(-g - 1, w.box[base + w.frow[base + int(uint32_t(keys[s]))]]);
            }
        }
        if (!do_union) return;
        __syncthreads();
        for (int k = tid; k < nk; k += NMS_THREADS) {
            const uint32_t* u = ub + 4 * int64_t(k);
            reinterpret_cast<float4*>(out_boxes)[base + k] =
                make_float4(ord_float(cur(u + 0)), ord_float(cur(u + 1)), ord_float(cur(u + 2)), ord_float(cur(u + 3)));
        }
    }
}

// Sort of the filtered candidates (bitmask path) by rank: the keys (score descending, filtered
// index ascending) are unique, so key i goes to position #{j : key_j < key_i}.  K^2 comparisons
// over a (key tile i, key tile j) grid; the per-tile counts are integer atomics into rank[] (w.flag,
// zeroed by the compaction kernel) — order-independent, so the result is exact.
__device__ __forceinline__ uint64_t cand_key(const Ws& w, int64_t base, int f) {
    return (uint64_t(desc_bits(w.score[base + w.frow[base + f]])) << 32) | uint32_t(f);
}

__global__ void __launch_bounds__(256) nms_rank_kernel(int64_t N, Ws w) {
    __shared__ uint64_t tile[256];
    const int64_t b = blockIdx.z;
    const int K = w.kcount[b];
    const int i0 = blockIdx.x * 256, j0 = blockIdx.y * 256;
    if (i0 >= K || j0 >= K) return;
    const int64_t base = b * N;
    const int i = i0 + threadIdx.x;
    tile[threadIdx.x] = j0 + int(threadIdx.x) < K ? cand_key(w, base, j0 + threadIdx.x) : ~0ull;
    __syncthreads();
    if (i >= K) return;
    const uint64_t ki = cand_key(w, base, i);
    const int jn = min(256, K - j0);
    int cnt = 0;
    for (int jj = 0; jj < jn; ++jj) cnt += tile[jj] < ki;
    if (cnt) atomicAdd(&w.flag[base + i], cnt);
}

template <bool CLS>
__global__ void nms_rank_scatter_kernel(int64_t N, int64_t KP, Ws w) {
    const int64_t b = blockIdx.y;
    const int K = w.kcount[b];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const int64_t base = b * N;
    const int r = w.flag[base + i];
    w.keys[b * KP + r] = cand_key(w, base, i);
    w.sbox[base + r] = w.box[base + w.frow[base + i]];
    if constexpr (CLS) w.slabel[base + r] = w.label[base + w.frow[base + i]];
}

// maskT[b][cb][i] bit j-64cb = (j > i) && !(IoU(i, j) <= thr) for sorted positions i, j < K; only
// cb >= i/64 is written (the scan reads the upper triangle).  Block = 64 rows of one row block.
// Grid: x = the upper triangle's Wn (Wn + 1) / 2 (row block, column block) pairs, t = cb (cb + 1) / 2 + rb
// (half the blocks of a square grid, whose lower half only returned), z = image.
// CLS: the bit also needs label_i == label_j (tested first: another label's pair costs no IoU), so the scan, which
// only ORs kept rows' words, is class-aware without seeing a label.
template <bool CLS>
__global__ void __launch_bounds__(64) nms_mask_kernel(int64_t N, int Wn, float iou_thr, Ws w) {
    __shared__ float4 cols[64];
    __shared__ int32_t clab[64];
    const int tri = blockIdx.x;
    int cb = int((sqrtf(8.0f * float(tri) + 1.0f) - 1.0f) * 0.5f);
    while (cb * (cb + 1) / 2 > tri) --cb;
    while ((cb + 1) * (cb + 2) / 2 <= tri) ++cb;
    const int rb = tri - cb * (cb + 1) / 2;
    const int64_t b = blockIdx.z;
    const int K = w.kcount[b];
    if (rb * 64 >= K || cb * 64 >= K) return;
    const int t = threadIdx.x;
    const int64_t base = b * N;
    const int j0 = cb * 64;
    if (j0 + t < K) {
        cols[t] = w.sbox[base + j0 + t];
        if constexpr (CLS) clab[t] = w.slabel[base + j0 + t];
    }
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= K) return;
    const float4 bi = w.sbox[base + i];
    int32_t li = 0;
    if constexpr (CLS) li = w.slabel[base + i];
    uint64_t word = 0;
    const int jn = min(64, K - j0);
    for (int jj = 0; jj < jn; ++jj) {
        const int j = j0 + jj;
        if constexpr (CLS) {
            if (j > i && clab[jj] == li && !(iou_ref(bi, cols[jj]) <= iou_thr)) word |= uint64_t(1) << jj;
        } else {
            if (j > i && !(iou_ref(bi, cols[jj]) <= iou_thr)) word |= uint64_t(1) << jj;
        }
    }
    w.mask[(b * Wn + cb) * N + i] = word;          // column-major: column cb, row i
}

// Greedy scan, ONE wave per image, visiting only what the kept rows need (round 1's workgroup scan read the
// whole upper triangle: every earlier row of every column, ~K^2/128 words per image).  A chunk c's
// removed bits come from two places:
//  * NEAR rows (the previous group of 4 chunks and the earlier chunks of this group): the words
//    D(c', c) = column c, rows 64c'..64c'+63 are loaded one group AHEAD (they do not depend on any
//    decision; coalesced 512-B wave loads) and read under the kept bits of chunk c';
//  * FAR rows (two or more groups back): each lane accumulates, for the column blocks it owns
//    (cb = lane + 64k), the words of every kept row; a group's kept rows are gathered at the start
//    of the next group and joined at the start of the one after (the loads fly during a group).
// The per-chunk work is then one wave OR, the fixpoint of the chunk's 64x64 diagonal block and the
// keep update: no workgroup barrier, and ~(kept x Wn + 26 x 64 x groups) words read instead of the
// triangle.  Same decisions as nms_scan_kernel (a box is kept iff no earlier kept box has
// IoU > thr with it): the removed bits of chunk c are the OR over ALL kept rows j < 64c of
// mask[j][c], split into near and far.
constexpr int SCAN_WL = (BM_MAX_WN + 63) / 64;      // column-block words per lane (far bits)

// OR over the 64 lanes by DPP (row prefix-ORs, then row broadcasts 15 / 31; the total lands in lane
// 63): a dozen VALU steps instead of a chain of 12 cross-lane permutes
__device__ __forceinline__ uint32_t wave_or32_dpp(uint32_t v) {
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xf, 0xf, false));   // row_shr:1
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xf, 0xf, false));   // row_shr:2
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xf, 0xf, false));   // row_shr:4
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xf, 0xf, false));   // row_shr:8
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xa, 0xf, false));   // row_bcast:15
    v |= uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xc, 0xf, false));   // row_bcast:31
    return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}
__device__ __forceinline__ uint64_t wave_or64_dpp(uint64_t v) {
    return (uint64_t(wave_or32_dpp(uint32_t(v >> 32))) << 32) | wave_or32_dpp(uint32_t(v));
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    return (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), l))) << 32) |
           uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), l));
}
constexpr int SCAN_RB = 8;                          // kept rows per group gathered asynchronously

// CAP: stop at max_det (> 0) kept boxes: the chunk whose alive bits would pass the cap keeps its lowest
// max_det - nkept of them (sorted order within a chunk is bit order) and the scan ends; later decisions cannot matter.
template <bool CAP>
__global__ void __launch_bounds__(64) nms_scan_wave_kernel(int64_t N, int64_t KP, int Wn, float img_w, float img_h,
                                                           Ws w,
                                                           int32_t* __restrict__ out_count,
                                                           float* __restrict__ out_boxes,
                                                           float* __restrict__ out_scores,
                                                           int64_t* __restrict__ out_labels,
                                                           int64_t* __restrict__ out_index, int max_det = 0) {
    __shared__ int rows_sh[256];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int K = w.kcount[b];
    const int64_t base = b * N;
    if (K == 0) {
        if (lane == 0) out_count[b] = 0;
        return;
    }
    const int nch = (K + 63) / 64;
    const int ngr = (nch + 3) / 4;
    const uint64_t* mcol = w.mask + int64_t(b) * Wn * N;     // column cb: mcol + cb * N, row-indexed
    // raw buffer loads over this image's mask: 32-bit byte offsets, and every guarded-off load reads 0
    // through an out-of-range offset instead of a branch (one wave runs alone per image: its
    // instruction count is the kernel's time)
    const __amdgpu_buffer_rsrc_t mres = make_rsrc(mcol, int64_t(Wn) * N * 8);
    auto ld8 = [&](uint32_t off) -> uint64_t {
        const uint2 v = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(mres, off, 0, 0));
        return (uint64_t(v.y) << 32) | v.x;
    };

    uint64_t far[SCAN_WL];
#pragma unroll
    for (int k = 0; k < SCAN_WL; ++k) far[k] = 0;
    // D(c', c) for the 4 chunks q of a group: slot s <-> c' = 4g - 4 + s (s <= 4 + q)
    uint64_t dcur[4][8], dnx[4][8];
    auto load_group = [&](int g, uint64_t (&d)[4][8]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 4 * g + q;
            const uint32_t col = c < nch ? uint32_t(c * int(N) + lane) * 8u : OOB;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (s > 4 + q) {
                    d[q][s] = 0;
                    continue;
                }
                const int cp = 4 * g - 4 + s;
                d[q][s] = ld8(col == OOB || cp < 0 ? OOB : col + uint32_t(cp) * 512u);
            }
        }
    };
    uint64_t kprev[4] = {0, 0, 0, 0};                 // kept bits of the previous group's chunks
    uint64_t pend[SCAN_RB][SCAN_WL];                   // far words of the gathered rows, in flight
#pragma unroll
    for (int r = 0; r < SCAN_RB; ++r)
#pragma unroll
        for (int k = 0; k < SCAN_WL; ++k) pend[r][k] = 0;
    int nkept = 0;
    bool full = false;                                // CAP: max_det boxes are kept
    load_group(0, dcur);
    for (int g = 0; g < ngr && !full; ++g) {
        // Everything loaded at the previous group's start (this group's D blocks, the far words of
        // group g-2's kept rows) has had a whole group of decisions to arrive: wait for it HERE, once,
        // explicitly.  (Left to the compiler, the loop-carried loads got conservative vmcnt waits
        // inside the chunk loop that also waited for the loads issued at THIS group's start.)
        __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0), expcnt / lgkmcnt untouched
#pragma unroll
        for (int r = 0; r < SCAN_RB; ++r)
#pragma unroll
            for (int k = 0; k < SCAN_WL; ++k) far[k] |= pend[r][k];
        if (g >= 1)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < 8; ++s) dcur[q][s] = dnx[q][s];
        // next group's D blocks, and the far words (columns cb >= 4(g+1), beyond group g's near window)
        // of group g-1's kept rows: in flight during this group, used from the next group on
        if (g + 1 < ngr) load_group(g + 1, dnx);
        int nr = 0;
        if (g >= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t kb = kprev[q];
                if ((kb >> lane) & 1)
                    rows_sh[nr + __popcll(kb & ((uint64_t(1) << lane) - 1))] = 64 * (4 * (g - 1) + q) + lane;
                nr += __popcll(kb);
            }
            __builtin_amdgcn_wave_barrier();
        }
        const int cb_lo = 4 * (g + 1);
        auto row_words = [&](int j, uint64_t* dst) {
#pragma unroll
            for (int k = 0; k < SCAN_WL; ++k) {
                const int cb = lane + 64 * k;
                dst[k] = ld8(j >= 0 && cb >= cb_lo && cb < Wn ? uint32_t(cb * int(N) + j) * 8u : OOB);
            }
        };
        const int npend = min(nr, SCAN_RB);
#pragma unroll
        for (int r = 0; r < SCAN_RB; ++r) row_words(r < npend ? rows_sh[r] : -1, pend[r]);
        for (int r = SCAN_RB; r < nr; ++r) {   // > SCAN_RB kept rows: synchronously
            uint64_t t[SCAN_WL];
            row_words(rows_sh[r], t);
#pragma unroll
            for (int k = 0; k < SCAN_WL; ++k) far[k] |= t[k];
        }
        uint64_t kcur[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 4 * g + q;
            if (c >= nch) break;
            // near rows: previous group (slots 0..3) and this group's earlier chunks (slots 4..4+q-1):
            // each lane ORs the words of its kept rows, then one DPP OR over the wave
            uint64_t nl = 0;
#pragma unroll
            for (int s = 0; s < 4 + q; ++s)
                if ((((s < 4 ? kprev[s] : kcur[s - 4]) >> lane) & 1)) nl |= dcur[q][s];
            const uint64_t near = wave_or64_dpp(nl);
            // far rows: column c's word lives in lane c & 63, slot c >> 6
            const int kw = c >> 6;
            uint64_t fw = far[0];
#pragma unroll
            for (int k = 1; k < SCAN_WL; ++k)
                if (kw == k) fw = far[k];
            const uint64_t rem = near | readlane64(fw, c & 63);
            const int rows = min(64, K - 64 * c);
            const uint64_t diag = dcur[q][4 + q];
            // the diagonal block greedily, one iteration per KEPT row (~1-2 per chunk): the lowest
            // undecided bit s survives, and its row (lane s's word, bits > s only) removes later bits
            uint64_t und = ~rem & (rows == 64 ? ~uint64_t(0) : ((uint64_t(1) << rows) - 1));
            uint64_t alive = 0;
            while (und) {
                const int sl = __builtin_ctzll(und);
                alive |= uint64_t(1) << sl;
                und &= ~readlane64(diag, sl) & ~(uint64_t(1) << sl);
            }
            if constexpr (CAP) {
                if (nkept + __popcll(alive) >= max_det) {
                    uint64_t rest = alive;
                    alive = 0;
                    for (int m = max_det - nkept; m > 0; --m) {     // the lowest max_det - nkept alive bits
                        alive |= rest & (~rest + 1);
                        rest &= rest - 1;
                    }
                    full = true;
                }
            }
            if ((alive >> lane) & 1) out_index[base + nkept + __popcll(alive & ((uint64_t(1) << lane) - 1))] = 64 * c + lane;
            nkept += __popcll(alive);
            kcur[q] = alive;
            if constexpr (CAP)
                if (full) break;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) kprev[q] = kcur[q];
    }
    // CAP: the early stop leaves this group's dnx / pend loads in flight; nothing reads them, drain them before
    // the registers are reused below
    if constexpr (CAP) __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();                                 // this wave's out_index stores are visible to its loads
    // outputs in kept order (sorted position -> filtered index -> row)
    for (int k = lane; k < nkept; k += 64) {
        const int spos = int(out_index[base + k]);
        const int f = int(uint32_t(w.keys[b * KP + spos]));
        const int64_t row = base + w.frow[base + f];
        float4 bx = w.box[row];
        bx.x = fminf(fmaxf(bx.x / img_w, 0.0f), 1.0f);
        bx.y = fminf(fmaxf(bx.y / img_h, 0.0f), 1.0f);
        bx.z = fminf(fmaxf(bx.z / img_w, 0.0f), 1.0f);
        bx.w = fminf(fmaxf(bx.w / img_h, 0.0f), 1.0f);
        reinterpret_cast<float4*>(out_boxes)[base + k] = bx;
        out_scores[base + k] = w.score[row];
        out_labels[base + k] = w.label[row];
        out_index[base + k] = f;
    }
    if (lane == 0) out_count[b] = nkept;
}

// cls: the class-aware instances with the max_det cap (0: none); lab64: the caller's 64-bit labels by row (ym_nms_cls),
// null: w.label.  The class-agnostic entry points launch the CLS = false / CAP = false instances.
int launch_nms(int64_t B, int64_t Nalloc, float iou_thr, float img_w, float img_h, int clamp_norm, Ws w,
               int32_t* out_count, float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_index,
               hipStream_t st, bool cls = false, int max_det = 0, const int64_t* lab64 = nullptr) {
    size_t lds = size_t(SORT_LDS_KEYS) * sizeof(uint64_t);
    if (w.mask && clamp_norm) {
        const int Wn = int((Nalloc + 63) / 64);
        const int64_t KP = pow2_at_least(Nalloc);
        // (the compaction never reads a label: one instance serves both)
        hipLaunchKernelGGL((nms_image_kernel<true, false, int32_t>), dim3(unsigned(B)), dim3(NMS_THREADS), lds, st,
                           Nalloc, KP, iou_thr, img_w, img_h, clamp_norm, w, out_count, out_boxes, out_scores,
                           out_labels, out_index,static_cast<const int32_t*>(nullptr), 0);
        const unsigned nt = unsigned((Nalloc + 255) / 256);
        hipLaunchKernelGGL(nms_rank_kernel, dim3(nt, nt, unsigned(B)), dim3(256), 0, st, Nalloc, w);
        const dim3 mgrid(unsigned(Wn * (Wn + 1) / 2), 1, unsigned(B));
        if (cls) {
            hipLaunchKernelGGL(nms_rank_scatter_kernel<true>, dim3(nt, unsigned(B)), dim3(256), 0, st, Nalloc, KP, w);
            hipLaunchKernelGGL(nms_mask_kernel<true>, mgrid, dim3(64), 0, st, Nalloc, Wn, iou_thr, w);
        } else {
            hipLaunchKernelGGL(nms_rank_scatter_kernel<false>, dim3(nt, unsigned(B)), dim3(256), 0, st, Nalloc, KP, w);
            hipLaunchKernelGGL(nms_mask_kernel<false>, mgrid, dim3(64), 0, st, Nalloc, Wn, iou_thr, w);
        }
        if (cls && max_det > 0)
            hipLaunchKernelGGL(nms_scan_wave_kernel<true>, dim3(unsigned(B)), dim3(64), 0, st, Nalloc, KP, Wn, img_w,
                               img_h, w, out_count, out_boxes, out_scores, out_labels, out_index, max_det);
        else
            hipLaunchKernelGGL(nms_scan_wave_kernel<false>, dim3(unsigned(B)), dim3(64), 0, st, Nalloc, KP, Wn,
                               img_w, img_h, w, out_count, out_boxes, out_scores, out_labels, out_index, 0);
        YM_LAUNCH_CHECK("nms bitmask path");
        return YM_OK;
    }
    const int64_t KP = pow2_at_least(Nalloc);
    if (cls && lab64)
        hipLaunchKernelGGL((nms_image_kernel<false, true, int64_t>), dim3(unsigned(B)), dim3(NMS_THREADS), lds, st,
                           Nalloc, KP, iou_thr, img_w, img_h, clamp_norm, w, out_count, out_boxes, out_scores,
                           out_labels, out_index,lab64, max_det);
    else if (cls)
        hipLaunchKernelGGL((nms_image_kernel<false, true, int32_t>), dim3(unsigned(B)), dim3(NMS_THREADS), lds, st,
                           Nalloc, KP, iou_thr, img_w, img_h, clamp_norm, w, out_count, out_boxes, out_scores,
                           out_labels, out_index,static_cast<const int32_t*>(w.label), max_det);
    else
        hipLaunchKernelGGL((nms_image_kernel<false, false, int32_t>), dim3(unsigned(B)), dim3(NMS_THREADS), lds, st,
                           Nalloc, KP, iou_thr, img_w, img_h, clamp_norm, w, out_count, out_boxes, out_scores,
                           out_labels, out_index,static_cast<const int32_t*>(nullptr), 0);
    YM_LAUNCH_CHECK("nms_image_kernel");
    return YM_OK;
}

}  // namespace
}  // namespace ym

using namespace ym;

extern "C" size_t ym_nms_workspace_size(int64_t B, int64_t N) { return 2 * ws_bytes(B, N); }

__global__ void ym_iou_row_kernel(const float4* __restrict__ b1, const float4* __restrict__ b2, int64_t m,
                                  float* __restrict__ out) {
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < m) out[i] = iou_ref(*b1, b2[i]);
}

extern "C" int ym_iou_row(const float* box1, const float* boxes2, int64_t m, float* out, void* stream) {
    YM_CHECK_ARG(m >= 0, "ym_iou_row: m < 0");
    if (m == 0) return YM_OK;
    hipLaunchKernelGGL(ym_iou_row_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4*>(box1), reinterpret_cast<const float4*>(boxes2), m, out);
    YM_LAUNCH_CHECK("ym_iou_row");
    return YM_OK;
}

// cls: ym_decode_nms_cls (its workspace layout, the class-aware kernels, the max_det cap).  Kept boxes are written as
// x / img_w, y / img_h; the single-size entry points pass img_w = img_h = img_size.
static int decode_nms_impl(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t img_stride,
                           int64_t col_stride, float conf, float iou_thr, float img_w, float img_h, bool cls,
                           int max_det, void* workspace, size_t workspace_bytes, int32_t* out_count, float* out_boxes,
                           float* out_scores, int64_t* out_labels, int64_t* out_index, void* stream) {
    YM_CHECK_ARG(max_det >= 0, "ym_decode_nms_cls: max_det %d < 0", max_det);
    YM_CHECK_ARG(B >= 0 && N >= 0 && C >= 1, "ym_decode_nms: bad shape B=%lld N=%lld C=%lld", (long long)B,
                 (long long)N, (long long)C);
    YM_CHECK_ARG(col_stride >= 1 && (col_stride > 1 || row_stride >= 4 + C), "ym_decode_nms: row_stride < 4+C");
    YM_CHECK_ARG(N < (int64_t(1) << 30), "ym_decode_nms: N too large");
    if (B == 0) return YM_OK;
    hipStream_t st = as_stream(stream);
    if (N == 0) return hipMemsetAsync(out_count, 0, B * sizeof(int32_t), st) == hipSuccess ? YM_OK : YM_ERR_HIP;
    const size_t need = cls ? ws_bytes_cls(B, N) : ws_bytes(B, N);
    YM_CHECK_ARG(workspace_bytes >= need, "ym_decode_nms: workspace too small (%zu < %zu)", workspace_bytes, need);
    Ws w = carve(workspace, B, N, cls);
    if (C <= 64)
        hipLaunchKernelGGL(rowmax_thread_kernel, dim3(unsigned((B * N + 255) / 256)), dim3(256), 0, st, pred, B, N,
                           C, row_stride, img_stride, col_stride, conf, w);
    else
        hipLaunchKernelGGL(rowmax_wave_kernel, dim3(unsigned((B * N + 3) / 4)), dim3(256), 0, st, pred, B, N, C,
                           row_stride, img_stride, col_stride, conf, w);
    YM_LAUNCH_CHECK("rowmax");
    return launch_nms(B, N, iou_thr, img_w, img_h, 1, w, out_count, out_boxes, out_scores, out_labels, out_index, st,
                      cls, max_det);
}

extern "C" int ym_decode_nms_strided(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride,
                                     int64_t img_stride, int64_t col_stride, float conf, float iou_thr, float img_size,
                                     void* workspace, size_t workspace_bytes, int32_t* out_count, float* out_boxes,
                                     float* out_scores, int64_t* out_labels, int64_t* out_index, void* stream) {
    return decode_nms_impl(pred, B, N, C, row_stride, img_stride, col_stride, conf, iou_thr, img_size, img_size, false,
                           0, workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                           stream);
}

// A frame of img_h rows and img_w columns: x / img_w, y / img_h.  Everything else is ym_decode_nms_strided.
extern "C" int ym_decode_nms_strided_wh(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride,
                                        int64_t img_stride, int64_t col_stride, float conf, float iou_thr, float img_w,
                                        float img_h, void* workspace, size_t workspace_bytes, int32_t* out_count,
                                        float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_index,
                                        void* stream) {
    YM_CHECK_ARG(img_w > 0.0f && img_h > 0.0f, "ym_decode_nms_strided_wh: img_w %g, img_h %g must be > 0",
                 double(img_w), double(img_h));
    return decode_nms_impl(pred, B, N, C, row_stride, img_stride, col_stride, conf, iou_thr, img_w, img_h, false, 0,
                           workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index, stream);
}

extern "C" size_t ym_nms_cls_workspace_size(int64_t B, int64_t N) { return 2 * ws_bytes_cls(B, N); }

extern "C" int ym_decode_nms_cls(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride,
                                 int64_t img_stride, int64_t col_stride, float conf, float iou_thr, float img_size,
                                 int max_det, void* workspace, size_t workspace_bytes, int32_t* out_count,
                                 float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_index,
                                 void* stream) {
    return decode_nms_impl(pred, B, N, C, row_stride, img_stride, col_stride, conf, iou_thr, img_size, img_size, true,
                           max_det, workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                           stream);
}

extern "C" int ym_decode_nms_cls_wh(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride,
                                    int64_t img_stride, int64_t col_stride, float conf, float iou_thr, float img_w,
                                    float img_h, int max_det, void* workspace, size_t workspace_bytes,
                                    int32_t* out_count, float* out_boxes, float* out_scores, int64_t* out_labels,
                                    int64_t* out_index, void* stream) {
    YM_CHECK_ARG(img_w > 0.0f && img_h > 0.0f, "ym_decode_nms_cls_wh: img_w %g, img_h %g must be > 0", double(img_w),
                 double(img_h));
    return decode_nms_impl(pred, B, N, C, row_stride, img_stride, col_stride, conf, iou_thr, img_w, img_h, true,
                           max_det, workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                           stream);
}

extern "C" int ym_decode_nms(const float* pred, int64_t B, int64_t N, int64_t C, int64_t row_stride,
                             int64_t img_stride, float conf, float iou_thr, float img_size, void* workspace,
                             size_t workspace_bytes, int32_t* out_count, float* out_boxes, float* out_scores,
                             int64_t* out_labels, int64_t* out_index, void* stream) {
    return ym_decode_nms_strided(pred, B, N, C, row_stride, img_stride, 1, conf, iou_thr, img_size, workspace,
                                 workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index, stream);
}

// cls: ym_nms_cls (labels, null: one class; max_det).  Both use ym_nms's workspace layout.
static int nms_impl(const float* boxes, const float* scores, const int64_t* labels, int64_t n, float iou_thr, bool cls,
                    int max_det, void* workspace, size_t workspace_bytes, int64_t* keep, int32_t* count,
                    void* stream) {
    YM_CHECK_ARG(n >= 0, "ym_nms: n < 0");
    YM_CHECK_ARG(max_det >= 0, "ym_nms_cls: max_det %d < 0", max_det);
    hipStream_t st = as_stream(stream);
    if (n == 0) return hipMemsetAsync(count, 0, sizeof(int32_t), st) == hipSuccess ? YM_OK : YM_ERR_HIP;
    YM_CHECK_ARG(workspace_bytes >= ws_bytes(1, n) + ws_bytes(1, n), "ym_nms: workspace too small");
    Ws w = carve(workspace, 1, n);
    // scratch outputs (boxes/scores/labels) after the candidate arrays
    char* extra = static_cast<char*>(workspace) + ws_bytes(1, n);
    float* ob = reinterpret_cast<float*>(extra);
    float* os = reinterpret_cast<float*>(extra + align256(n * 16));
    int64_t* ol = reinterpret_cast<int64_t*>(extra + align256(n * 16) + align256(n * 4));
    hipLaunchKernelGGL(direct_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(boxes), scores, labels, n, w);
    YM_LAUNCH_CHECK("nms direct");
    return launch_nms(1, n, iou_thr, 1.0f, 1.0f, 0, w, count, ob, os, ol, keep, st, cls, max_det, labels);
}

extern "C" int ym_nms(const float* boxes, const float* scores, int64_t n, float iou_thr, void* workspace,
                      size_t workspace_bytes, int64_t* keep, int32_t* count, void* stream) {
    return nms_impl(boxes, scores, nullptr, n, iou_thr, false, 0, workspace, workspace_bytes, keep, count, stream);
}

extern "C" int ym_nms_cls(const float* boxes, const float* scores, const int64_t* labels, int64_t n, float iou_thr,
                          int max_det, void* workspace, size_t workspace_bytes, int64_t* keep, int32_t* count,
                          void* stream) {
    return nms_impl(boxes, scores, labels, n, iou_thr, true, max_det, workspace, workspace_bytes, keep, count, stream);
}

// ---------------------------------------------------------------- tiles (ym_decode_nms_tiles)
// The candidate stage of sliced inference: the rowmax stage over every tile's rows, with the map to source pixels and
// the tile-border filter fused into it (the box and the score are in registers there; a second launch would read and
// write the 20-byte box / flag record of every row again and add a launch).  The rows of image g land in the image's
// slice [g * R, (g + 1) * R) of the candidate arrays in (tile, row) order, so everything from nms_image_kernel
// downward runs unchanged on (G, R) with clamp_norm = 0.  blockIdx.y walks the images of a launch, whose tile ranges
// travel by value in the kernel arguments (TILE_SPAN images per launch): the host's tile_begin needs no copy of its
// own, and the image's range is block-uniform.
namespace ym {
namespace {

constexpr int TILE_SPAN = 32;
struct TileSpan {
    int32_t begin[TILE_SPAN + 1];
};

// the candidate arrays of launch_nms's image-kernel path alone (no bitmask path at clamp_norm = 0)
inline size_t tiles_ws_bytes(int64_t G, int64_t R) {
    const size_t n = size_t(G) * size_t(R);
    return align256(n * 16) + 4 * align256(n * 4) + align256(size_t(G) * pow2_at_least(R) * 8) + 256;
}

inline Ws carve_tiles(void* base, int64_t G, int64_t R) {
    char* p = static_cast<char*>(base);
    const size_t n = size_t(G) * size_t(R);
    Ws w;
    w.box = reinterpret_cast<float4*>(p);    p += align256(n * sizeof(float4));
    w.score = reinterpret_cast<float*>(p);   p += align256(n * sizeof(float));
    w.label = reinterpret_cast<int32_t*>(p); p += align256(n * sizeof(int32_t));
    w.flag = reinterpret_cast<int32_t*>(p);  p += align256(n * sizeof(int32_t));
    w.frow = reinterpret_cast<int32_t*>(p);  p += align256(n * sizeof(int32_t));
    w.keys = reinterpret_cast<uint64_t*>(p);
    w.sbox = nullptr; w.mask = nullptr; w.kcount = nullptr; w.slabel = nullptr;
    return w;
}

// row (x, y, bw, bh) of tile `e` with max score mx / label lab -> the candidate record at o: xywh -> xyxy in frame
// pixels, then to source pixels in rounded fp32 steps; the flag also needs the box not to be cut by an interior side
__device__ __forceinline__ void tile_candidate(const ym_tile_entry& e, float x, float y, float bw, float bh, float mx,
                                               int lab, float conf, float edge, int64_t o, const Ws& w) {
    const float hw = bw / 2.0f, hh = bh / 2.0f;
    const float left = float(e.left), top = float(e.top), tw = float(e.tw), th = float(e.th);
    float u1 = fminf(fmaxf(__fmul_rn(__fsub_rn(x - hw, left), e.sx), 0.f), tw);
    float v1 = fminf(fmaxf(__fmul_rn(__fsub_rn(y - hh, top), e.sy), 0.f), th);
    float u2 = fminf(fmaxf(__fmul_rn(__fsub_rn(x + hw, left), e.sx), 0.f), tw);
    float v2 = fminf(fmaxf(__fmul_rn(__fsub_rn(y + hh, top), e.sy), 0.f), th);
    // mirrored views: back through the mirror in window pixels, before the edge test, whose bits name
    // window sides in source orientation
    if (e.edges & YM_TILE_MIRROR_X) {
        const float a = __fsub_rn(tw, u2), b = __fsub_rn(tw, u1);
        u1 = a, u2 = b;
    }
    if (e.edges & YM_TILE_MIRROR_Y) {
        const float a = __fsub_rn(th, v2), b = __fsub_rn(th, v1);
        v1 = a, v2 = b;
    }
    bool cut = false;
    if (edge > 0.0f)
        cut = ((e.edges & 1) && u1 < edge) || ((e.edges & 2) && u2 > __fsub_rn(tw, edge)) ||
              ((e.edges & 4) && v1 < edge) || ((e.edges & 8) && v2 > __fsub_rn(th, edge));
    const float x0 = float(e.x0), y0 = float(e.y0);
    w.box[o] = make_float4(__fadd_rn(u1, x0), __fadd_rn(v1, y0), __fadd_rn(u2, x0), __fadd_rn(v2, y0));
    w.score[o] = mx;
    w.label[o] = lab;
    w.flag[o] = (mx > conf && !cut) ? 1 : 0;
}

// thread per row (C <= 64): rowmax_thread_kernel's scan; grid (ceil(R / 256), images of the launch)
__global__ void rowmax_tiles_thread_kernel(const float* __restrict__ pred, int64_t N, int64_t C, int64_t rs,
                                           int64_t ts, int64_t cs, const ym_tile_entry* __restrict__ table,
                                           TileSpan span, int64_t g0, int64_t R, float conf, float edge, Ws w) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= R) return;
    const int64_t o = (g0 + blockIdx.y) * R + j;
    const int64_t slot = j / N, n = j - slot * N;
    const int64_t t = span.begin[blockIdx.y] + slot;
    if (t >= span.begin[blockIdx.y + 1]) { w.flag[o] = 0; return; }     // padding row of an image with fewer tiles
    const ym_tile_entry e = table[t];
    if (e.src < 0) { w.flag[o] = 0; return; }
    const float* r = pred + t * ts + n * rs;
    float mx = r[4 * cs];
    int lab = 0;
    for (int64_t c = 1; c < C; ++c) {
        float v = r[(4 + c) * cs];
        if (v > mx) { mx = v; lab = int(c); }
    }
    tile_candidate(e, r[0], r[cs], r[2 * cs], r[3 * cs], mx, lab, conf, edge, o, w);
}

// wave per row (C > 64): rowmax_wave_kernel's scan; grid (ceil(R / 4), images of the launch)
__global__ void rowmax_tiles_wave_kernel(const float* __restrict__ pred, int64_t N, int64_t C, int64_t rs, int64_t ts,
                                         int64_t cs, const ym_tile_entry* __restrict__ table, TileSpan span,
                                         int64_t g0, int64_t R, float conf, float edge, Ws w) {
    const int64_t j = int64_t(blockIdx.x) * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (j >= R) return;
    const int64_t o = (g0 + blockIdx.y) * R + j;
    const int64_t slot = j / N, n = j - slot * N;
    const int64_t t = span.begin[blockIdx.y] + slot;
    if (t >= span.begin[blockIdx.y + 1]) {
        if (lane == 0) w.flag[o] = 0;
        return;
    }
    const ym_tile_entry e = table[t];
    if (e.src < 0) {
        if (lane == 0) w.flag[o] = 0;
        return;
    }
    const float* r = pred + t * ts + n * rs;
    float mx = -INFINITY;
    int64_t lab = INT64_MAX;
    for (int64_t c = lane; c < C; c += 64) {
        float v = r[(4 + c) * cs];
        if (v > mx || (v == mx && c < lab)) { mx = v; lab = c; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        float om = __shfl_xor(mx, s, 64);
        int64_t ol = __shfl_xor(lab, s, 64);
        if (om > mx || (om == mx && ol < lab)) { mx = om; lab = ol; }
    }
    if (lane == 0) tile_candidate(e, r[0], r[cs], r[2 * cs], r[3 * cs], mx, int(lab), conf, edge, o, w);
}

// kept filtered index -> row of the image's concatenation (frow survives the NMS kernel); grid (blocks, G)
__global__ void tile_rows_kernel(int64_t R, Ws w, const int32_t* __restrict__ count,
                                 const int64_t* __restrict__ index, int64_t* __restrict__ out_row) {
    const int64_t base = int64_t(blockIdx.y) * R;
    const int64_t n = min(int64_t(count[blockIdx.y]), R);
    for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += int64_t(gridDim.x) * blockDim.x)
        out_row[base + k] = w.frow[base + index[base + k]];
}

// the greedy-merging instances of the image kernel; track: out_merged or the union is wanted
template <bool CLS, int METRIC>
void launch_nmm_instance(bool track, int64_t G, int64_t R, float match_thr, Ws w, int32_t* out_count, float* out_boxes,
                         float* out_scores, int64_t* out_labels, int64_t* out_index, int max_det, int32_t* out_merged,
                         int do_union, hipStream_t st) {
    const size_t lds = size_t(SORT_LDS_KEYS) * sizeof(uint64_t);
    const int64_t KP = pow2_at_least(R);
    const int32_t* labs = CLS ? static_cast<const int32_t*>(w.label) : nullptr;
    // (IoU without tracking is nms_image_kernel, which the caller launches: no instance of its own)
    if (track || METRIC == YM_MATCH_IOU)
        hipLaunchKernelGGL((nms_image_kernel<false, CLS, int32_t, METRIC, true>), dim3(unsigned(G)), dim3(NMS_THREADS),
                           lds, st, R, KP, match_thr, 1.0f, 1.0f, 0, w, out_count, out_boxes, out_scores, out_labels,
                           out_index, labs, max_det, out_merged, do_union);
    else if constexpr (METRIC != YM_MATCH_IOU)
        hipLaunchKernelGGL((nms_image_kernel<false, CLS, int32_t, METRIC, false>), dim3(unsigned(G)),
                           dim3(NMS_THREADS), lds, st, R, KP, match_thr, 1.0f, 1.0f, 0, w, out_count, out_boxes,
                           out_scores, out_labels, out_index, labs, max_det, static_cast<int32_t*>(nullptr), 0);
}

// the weighted-mean instances (ym_decode_nmw_tiles); acc: G * R * 5 sums in the workspace
template <bool CLS, int METRIC>
void launch_nmw_instance(int64_t G, int64_t R, float match_thr, Ws w, int32_t* out_count, float* out_boxes,
                         float* out_scores, int64_t* out_labels, int64_t* out_index, int max_det, int32_t* out_merged,
                         long long* acc, hipStream_t st) {
    const size_t lds = size_t(SORT_LDS_KEYS) * sizeof(uint64_t);
    const int32_t* labs = CLS ? static_cast<const int32_t*>(w.label) : nullptr;
    hipLaunchKernelGGL((nms_image_kernel<false, CLS, int32_t, METRIC, true, true>), dim3(unsigned(G)),
                       dim3(NMS_THREADS), lds, st, R, pow2_at_least(R), match_thr, 1.0f, 1.0f, 0, w, out_count,
                       out_boxes, out_scores, out_labels, out_index, labs, max_det, out_merged, 0, acc);
}

inline size_t nmw_ws_bytes(int64_t G, int64_t R) {
    return tiles_ws_bytes(G, R) + align256(size_t(G) * size_t(R) * 5 * sizeof(long long));
}

// nmm: ym_decode_nmm_tiles / ym_decode_nmw_tiles (fn names the entry point in messages); otherwise metric = IoU,
// merge = 0, out_merged null.  mean: ym_decode_nmw_tiles (merge unused)
int decode_tiles_impl(const char* fn, bool nmm, bool mean, const float* pred, int64_t T, int64_t N, int64_t C, int64_t row_stride,
                      int64_t tile_stride, int64_t col_stride, const ym_tile_entry* table_dev,
                      const int64_t* tile_begin, int64_t G, float conf, float thr, int metric, int merge, float edge,
                      int class_aware, int max_det, void* workspace, size_t workspace_bytes, int32_t* out_count,
                      float* out_boxes, float* out_scores, int64_t* out_labels, int64_t* out_index, int64_t* out_row,
                      int32_t* out_merged, void* stream) {
    YM_CHECK_ARG(G >= 0 && G <= 65535 * int64_t(TILE_SPAN), "%s: G=%lld", fn, (long long)G);
    YM_CHECK_ARG(max_det >= 0, "%s: max_det %d < 0", fn, max_det);
    YM_CHECK_ARG(max_det == 0 || class_aware, "%s: max_det needs class_aware", fn);
    YM_CHECK_ARG(edge == edge, "%s: edge is NaN", fn);
    YM_CHECK_ARG(metric == YM_MATCH_IOU || metric == YM_MATCH_IOS, "%s: metric %d is neither YM_MATCH_IOU nor YM_MATCH_IOS",
                 fn, metric);
    YM_CHECK_ARG(!nmm || thr == thr, "%s: match_thr is NaN", fn);
    YM_CHECK_ARG(T >= 0 && T <= INT32_MAX && N >= 0 && N < (int64_t(1) << 30) && C >= 1,
                 "%s: bad shape T=%lld N=%lld C=%lld", fn, (long long)T, (long long)N, (long long)C);
    YM_CHECK_ARG(col_stride >= 1 && (col_stride > 1 || row_stride >= 4 + C), "%s: row_stride < 4+C", fn);
    YM_CHECK_ARG(tile_begin && tile_begin[0] >= 0, "%s: tile_begin", fn);
    int64_t most = 0;
    for (int64_t g = 0; g < G; ++g) {
        YM_CHECK_ARG(tile_begin[g + 1] >= tile_begin[g], "%s: tile_begin is not monotone at %lld", fn, (long long)g);
        most = std::max(most, tile_begin[g + 1] - tile_begin[g]);
    }
    YM_CHECK_ARG(tile_begin[G] <= T, "%s: tile_begin[G]=%lld > T=%lld", fn, (long long)tile_begin[G], (long long)T);
    const int64_t R = N * most;                              // < 2^61: both factors were bounded above
    YM_CHECK_ARG(R < (int64_t(1) << 30), "%s: R=%lld too large", fn, (long long)R);
    YM_CHECK_ARG(!mean || R < NMW_MAX_R, "%s: R=%lld too large for the int64 sums (< 2^26)", fn, (long long)R);
    if (G == 0) return YM_OK;
    YM_CHECK_ARG(out_count, "%s: out_count is NULL", fn);
    hipStream_t st = as_stream(stream);
    if (R == 0) return hipMemsetAsync(out_count, 0, G * sizeof(int32_t), st) == hipSuccess ? YM_OK : YM_ERR_HIP;
    YM_CHECK_ARG(pred && table_dev && workspace && out_boxes && out_scores && out_labels && out_index,
                 "%s: NULL argument", fn);
    const size_t need = mean ? nmw_ws_bytes(G, R) : tiles_ws_bytes(G, R);
    YM_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    Ws w = carve_tiles(workspace, G, R);
    for (int64_t g0 = 0; g0 < G; g0 += TILE_SPAN) {
        const int ng = int(std::min<int64_t>(TILE_SPAN, G - g0));
        TileSpan span = {};
        for (int k = 0; k <= ng; ++k) span.begin[k] = int32_t(tile_begin[g0 + k]);
        if (C <= 64)
            hipLaunchKernelGGL(rowmax_tiles_thread_kernel, dim3(unsigned((R + 255) / 256), unsigned(ng)), dim3(256), 0,
                               st, pred, N, C, row_stride, tile_stride, col_stride, table_dev, span, g0, R, conf, edge,
                               w);
        else
            hipLaunchKernelGGL(rowmax_tiles_wave_kernel, dim3(unsigned((R + 3) / 4), unsigned(ng)), dim3(256), 0, st,
                               pred, N, C, row_stride, tile_stride, col_stride, table_dev, span, g0, R, conf, edge, w);
    }
    YM_LAUNCH_CHECK("rowmax tiles");
    const bool track = merge != 0 || out_merged != nullptr;
    if (mean) {
        long long* acc = reinterpret_cast<long long*>(static_cast<char*>(workspace) + tiles_ws_bytes(G, R));
        if (class_aware && metric == YM_MATCH_IOS)
            launch_nmw_instance<true, YM_MATCH_IOS>(G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                    out_index, max_det, out_merged, acc, st);
        else if (class_aware)
            launch_nmw_instance<true, YM_MATCH_IOU>(G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                    out_index, max_det, out_merged, acc, st);
        else if (metric == YM_MATCH_IOS)
            launch_nmw_instance<false, YM_MATCH_IOS>(G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                     out_index, 0, out_merged, acc, st);
        else
            launch_nmw_instance<false, YM_MATCH_IOU>(G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                     out_index, 0, out_merged, acc, st);
        YM_LAUNCH_CHECK("nms_image_kernel (weighted mean)");
    } else if (metric == YM_MATCH_IOU && !track) {                  // the suppression kernels themselves
        const int rc = launch_nms(G, R, thr, 1.0f, 1.0f, 0, w, out_count, out_boxes, out_scores, out_labels, out_index,
                                  st, class_aware != 0, max_det);
        if (rc != YM_OK) return rc;
    } else {
        const int du = merge != 0;
        if (class_aware && metric == YM_MATCH_IOS)
            launch_nmm_instance<true, YM_MATCH_IOS>(track, G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                    out_index, max_det, out_merged, du, st);
        else if (class_aware)
            launch_nmm_instance<true, YM_MATCH_IOU>(track, G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                    out_index, max_det, out_merged, du, st);
        else if (metric == YM_MATCH_IOS)
            launch_nmm_instance<false, YM_MATCH_IOS>(track, G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                     out_index, 0, out_merged, du, st);
        else
            launch_nmm_instance<false, YM_MATCH_IOU>(track, G, R, thr, w, out_count, out_boxes, out_scores, out_labels,
                                                     out_index, 0, out_merged, du, st);
        YM_LAUNCH_CHECK("nms_image_kernel (merging)");
    }
    if (!out_row) return YM_OK;
    hipLaunchKernelGGL(tile_rows_kernel, dim3(unsigned(std::min<int64_t>((R + 255) / 256, 64)), unsigned(G)),
                       dim3(256), 0, st, R, w, out_count, out_index, out_row);
    YM_LAUNCH_CHECK("tile_rows_kernel");
    return YM_OK;
}

}  // namespace
}  // namespace ym

// (class_aware: the sorted labels belong to the bitmask path, which unnormalised boxes never take: the same size)
extern "C" size_t ym_decode_nms_tiles_workspace_size(int64_t G, int64_t R, int class_aware) {
    (void)class_aware;
    return tiles_ws_bytes(std::max<int64_t>(G, 0), std::max<int64_t>(R, 1));
}

extern "C" int ym_decode_nms_tiles(const float* pred, int64_t T, int64_t N, int64_t C, int64_t row_stride,
                                   int64_t tile_stride, int64_t col_stride, const ym_tile_entry* table_dev,
                                   const int64_t* tile_begin, int64_t G, float conf, float iou_thr, float edge,
                                   int class_aware, int max_det, void* workspace, size_t workspace_bytes,
                                   int32_t* out_count, float* out_boxes, float* out_scores, int64_t* out_labels,
                                   int64_t* out_index, int64_t* out_row, void* stream) {
    return decode_tiles_impl("ym_decode_nms_tiles", false, false, pred, T, N, C, row_stride, tile_stride, col_stride,
                             table_dev, tile_begin, G, conf, iou_thr, YM_MATCH_IOU, 0, edge, class_aware, max_det,
                             workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                             out_row, nullptr, stream);
}

// (the absorbing slots live in registers and in the flag words: ym_decode_nms_tiles's workspace)
extern "C" size_t ym_decode_nmm_tiles_workspace_size(int64_t G, int64_t R, int class_aware) {
    return ym_decode_nms_tiles_workspace_size(G, R, class_aware);
}

extern "C" int ym_decode_nmm_tiles(const float* pred, int64_t T, int64_t N, int64_t C, int64_t row_stride,
                                   int64_t tile_stride, int64_t col_stride, const ym_tile_entry* table_dev,
                                   const int64_t* tile_begin, int64_t G, float conf, float match_thr, int metric,
                                   int merge, float edge, int class_aware, int max_det, void* workspace,
                                   size_t workspace_bytes, int32_t* out_count, float* out_boxes, float* out_scores,
                                   int64_t* out_labels, int64_t* out_index, int64_t* out_row, int32_t* out_merged,
                                   void* stream) {
    return decode_tiles_impl("ym_decode_nmm_tiles", true, false, pred, T, N, C, row_stride, tile_stride, col_stride,
                             table_dev, tile_begin, G, conf, match_thr, metric, merge, edge, class_aware, max_det,
                             workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                             out_row, out_merged, stream);
}

// (ym_decode_nms_tiles's workspace, then the 5 int64 sums of every output slot)
extern "C" size_t ym_decode_nmw_tiles_workspace_size(int64_t G, int64_t R, int class_aware) {
    (void)class_aware;
    return nmw_ws_bytes(std::max<int64_t>(G, 0), std::max<int64_t>(R, 1));
}

extern "C" int ym_decode_nmw_tiles(const float* pred, int64_t T, int64_t N, int64_t C, int64_t row_stride,
                                   int64_t tile_stride, int64_t col_stride, const ym_tile_entry* table_dev,
                                   const int64_t* tile_begin, int64_t G, float conf, float match_thr, int metric,
                                   float edge, int class_aware, int max_det, void* workspace, size_t workspace_bytes,
                                   int32_t* out_count, float* out_boxes, float* out_scores, int64_t* out_labels,
                                   int64_t* out_index, int64_t* out_row, int32_t* out_merged, void* stream) {
    return decode_tiles_impl("ym_decode_nmw_tiles", true, true, pred, T, N, C, row_stride, tile_stride, col_stride,
                             table_dev, tile_begin, G, conf, match_thr, metric, 0, edge, class_aware, max_det,
                             workspace, workspace_bytes, out_count, out_boxes, out_scores, out_labels, out_index,
                             out_row, out_merged, stream);
}
