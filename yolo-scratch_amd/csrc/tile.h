// MFMA fragment types and raw-buffer helpers shared by the conv / wgrad kernels (gfx950).
#pragma once
#include "common.h"

namespace ym {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t OOB = 0x80000000u;          // buffer offset past num_records: loads return 0
constexpr int RSRC_FLAGS = 0x00020000;         // raw buffer, 32-bit data format (gfx9 dword3)

// buffer resource over [base, base + bytes); bytes clamped below 2^31 so OOB is always out of range
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0,
                                             int(bytes < 0x7fffffff ? (bytes > 0 ? bytes : 0) : 0x7fffffff),
                                             RSRC_FLAGS);
}

__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

// ---- LDS-DMA staging primitives of the conv kernels (conv.hip, conv_halo.hip, conv_pipe.hip, conv_hpipe.hip)
//
// LDS images are lane-linear (LDS-DMA writes lane l of a wave-instruction at base + 16*l); a row's 16-B chunk c is
// stored in slot c ^ f(r).  The swizzle lives on the global (source) side: a DMA lane that fills slot s of row r loads
// chunk s ^ f(r), so each lane group still reads one whole row.
// 128-B rows (64-deep K stages, 8 slots): f(r) = (r >> 1) & 7.  A ds_read_b128 lane group (rows {0-3,12-15} at chunk
// c, rows {4-11} at chunk c^1) then covers 16 distinct (row parity, slot) bank quads — for fragments that start at
// multiples of 16 rows (conv_hpipe.hip's halo rows start anywhere and use r & 7 instead).
__device__ __forceinline__ int fsw128(int r) { return (r >> 1) & 7; }
// 64-B rows (32-deep K stages, 4 slots): F(r) = 2 * ((r >> 2) & 1).  A ds_read_b128 lane group reads 16 rows s + fr at
// chunks c (fr in {0-3, 12-15}) and c ^ 1 (fr in {4-11}) (or the reverse); rows s+k, s+k+4, s+k+8, s+k+12 share bank
// quads and land on chunks {c, c^3, c^1, c^2} for EVERY start s — conv_halo.hip's fragments start at arbitrary rows
// (tap shifts, tile rows), where the earlier F = {0,3,2,1}[(r>>2)&3] conflicted 1.8-2.4x (bank-conflict model over
// the kernel's fragment rows: 7.3-9.4 LDS cycles per read -> 4.0-6.4; in conv.hip's 128x64 tiles it cost 45-50 %
// extra LDS cycles, this one measures SQ_LDS_BANK_CONFLICT 0, tools/pmc_conv.sh).
__device__ __forceinline__ int fsw64(int r) { return ((r >> 2) & 1) << 1; }

// one 1-KiB LDS-DMA piece: lane l's 16 bytes from rsrc + voff + soff land at lds + 16 l.  (A function, not the builtin
// written inline in the kernel's lambdas: there hipcc's host pass silently dropped the kernels' launch stubs.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}

// counted wait: at most N of this wave's vector-memory operations (LDS-DMA pieces, stores) stay in flight
template <int N>
__device__ __forceinline__ void vm_wait() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
    asm volatile("" ::: "memory");
}

// workgroup barrier without the vmcnt(0) drain __syncthreads() implies; LDS-DMA ordering is the caller's (a counted
// vm_wait before it), the asm clobbers keep LDS accesses on their side
__device__ __forceinline__ void raw_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// every ds_read issued so far has returned, then the workgroup barrier (no vmcnt drain); the
// sched_barriers keep the compiler from moving MFMAs / LDS reads across it
__device__ __forceinline__ void step_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    // the builtin, not inline asm: the compiler's wait-count pass sees this wait, so the MFMAs after the
    // barrier do not wait again for the fragments read before it (with an asm wait they stalled on the
    // next stage's freshly issued reads: lgkmcnt(3..0) ahead of the first four MFMAs of every step)
    __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// 8 fp16 -> 8 bf16 (v_cvt_f32_f16 + v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint4 h8_to_bf8(uint4 h) {
    uint32_t w[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = pk2bf(h2f(uint16_t(w[e] & 0xffff)), h2f(uint16_t(w[e] >> 16)));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// q = x / d, r = x % d for x < 2^24 (exact as a float), d >= 1, inv_d = 1.0f / d: the float estimate is within one of
// the quotient, one compare-and-correct each way (~8 VALU against ~25 for a 32-bit integer division)
__device__ __forceinline__ void fdivmod(uint32_t x, uint32_t d, float inv_d, uint32_t& q, uint32_t& r) {
    uint32_t e = uint32_t(float(x) * inv_d);
    int rem = int(x) - int(e * d);
    e = rem < 0 ? e - 1 : (rem >= int(d) ? e + 1 : e);
    q = e;
    r = x - e * d;
}

}  // namespace ym
