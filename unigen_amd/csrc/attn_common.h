// Device helpers shared by the attention kernels (attention.hip: the forward kernel and the backward kernels; tools/probe/csrc/attn_fwd_variants.hip,
// attn_bwd_variants.hip: the forward and backward forms that lost their A/B): LDS-DMA issue in pointer and buffer form, the XOR-swizzled K/V tile image, transposed LDS reads and the
// NaN-free max helpers. Sources that include this are built with -fno-honor-nans -mno-amdgpu-ieee (unigen_amd/build.py, EXTRA).
#pragma once
#include "ug_common.h"

#ifdef UG_PROBE_BUILD
// every forward form but the shipped one (attn_fwd_variants.hip, probe library only); the UG_ATTN_* environment switches select among them
int ug_attn_fwd_variants(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                         const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                         int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale, float* lse_out, int64_t lse_ld,
                         ug_stream_t stream);
#endif

// what ug_flash_attn_bwd has validated and derived, for the launch helpers of its three stages
struct ug_attn_bwd_args {
    const bf16_t* q; int64_t q_rs, q_bs; const bf16_t* k; int64_t k_rs, k_bs; const bf16_t* v; int64_t v_rs, v_bs; const bf16_t* dout; int64_t do_rs, do_bs;
    bf16_t* dq; int64_t dq_rs, dq_bs; bf16_t* dk; int64_t dk_rs, dk_bs; bf16_t* dv; int64_t dv_rs, dv_bs;
    float* lse2; const float* delta; int64_t stat_ld;      // statistics rows [batches][heads][stat_ld]
    int64_t batches; int heads, Lq, Lkv; float c /* scale * log2(e) */, scale; hipStream_t s;
};
enum { UG_BWD_STAGE_LSE = 0, UG_BWD_STAGE_DQ = 1, UG_BWD_STAGE_DKV = 2 };
#ifdef UG_PROBE_BUILD
// the backward forms that are not in the product (attn_bwd_variants.hip, probe library only): launches `stage` and returns true if the
// UG_ATTN_BWD_DMA / UG_ATTN_BWD_FUSE_DKV switches send it to one of them, else returns false and the caller launches the shipped kernel
bool ug_attn_bwd_variants(int stage, int dh, const ug_attn_bwd_args& a);
#endif

namespace {

constexpr int KVB = 64;      // keys per tile

typedef __attribute__((address_space(3))) bf16x4* lds_b64_ptr;
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
// LDS-DMA as inline asm: hipcc's waitcnt pass then does not know DMAs are in flight (with the builtin it put `s_waitcnt vmcnt(0)` ahead of
// the first ds_read behind every barrier, i.e. one segment after the issue instead of two); the kernel states the one wait itself.
// M0 = LDS byte address of the wave's 1 KiB run (lane l lands at + 16 l); one wait state between the SALU write of M0 and the DMA.
// (M0 is a reserved register for hipcc - it never keeps a value there across statements and rejects it on a clobber list - so writing it here is safe.)
__device__ __forceinline__ unsigned lds_addr(const unsigned char* l) { return (unsigned)(size_t)(lptr_t)l; }
__device__ __forceinline__ const void* uniform_ptr(const void* p) {      // pin a wave-uniform pointer into an SGPR pair
    const unsigned long long a = (unsigned long long)p;
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    asm volatile("s_nop 4" : "+s"(lo), "+s"(hi));      // VALU-written SGPR -> VMEM base: 5 wait states, not padded inside an asm statement
    return (const void*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void glds16_off(const void* base /* uniform_ptr() */, unsigned off_bytes, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off_bytes), "s"(base), "s"(lds) : "memory");
}
// buffer form of the same DMA: SGPR resource (base of the (batch, head)'s K or V) + per-lane byte offset + SGPR byte offset (the tile / run part)
__device__ __forceinline__ void bufds16(u32x4 rsrc, unsigned voff, unsigned soff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(rsrc), "s"(soff), "s"(lds) : "memory");
}
__device__ __forceinline__ void glds16_ptr(const void* g, unsigned lds) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory");
}
__device__ __forceinline__ void glds4_ptr(const void* g, unsigned lds) {          // 4 bytes per lane: lane l lands at lds + 4 l
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g), "s"(lds) : "memory");
}

// Row swizzle of the K/V tile images. f(row) is XORed into the 16-byte chunk index.
//   DH = 128 (256-byte rows): f = ((row & 3) << 2) | ((row >> 2) & 3)          (cdna guide T10, image (b))
//   DH =  64 (128-byte rows, two rows per 256-byte bank row): f = swap_bits_0_2((row >> 1) & 7): the 8 same-parity rows of a
//            ds_read_b128 lane group get 8 distinct chunks, and rows r, r+2 of a transposed-read block land in different
//            64-byte quarters -> both read kinds are conflict-free.
template <int DH>
__device__ __forceinline__ int row_swz(int row) {
    if constexpr (DH == 128) {
        return ((row & 3) << 2) | ((row >> 2) & 3);
    } else {
        const int v = (row >> 1) & 7;
        return ((v & 1) << 2) | (v & 2) | ((v >> 2) & 1);
    }
}
// byte offset of 16-byte chunk ch of row `row` in a [rows][DH x bf16] tile image
template <int DH>
__device__ __forceinline__ int img_off(int row, int ch) {
    return 2 * DH * row + 16 * (ch ^ row_swz<DH>(row));
}

__device__ __forceinline__ bf16x8 tr_read_pair(const unsigned char* lo, const unsigned char* hi) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64_ptr)lo);
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64_ptr)hi);
    return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// max of three; without IEEE mode hipcc does not add a NaN-quieting self-max per operand (the scores are finite or -inf here)
__device__ __forceinline__ float ug_max3(float a, float b, float c) {
    return __builtin_fmaxf(__builtin_fmaxf(a, b), c);     // v_max3_f32 (attention.hip is built with -fno-honor-nans -mno-amdgpu-ieee)
}
// max over the two 32-lane halves (lane l and l ^ 32), in every lane: one v_permlane32_swap (VALU) instead of the ds_bpermute +
// lgkmcnt(0) that __shfl_xor compiles to (which also waits for every LDS read in flight)
__device__ __forceinline__ float ug_max_halves(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return ug_max3(__uint_as_float(r[0]), __uint_as_float(r[1]), x);
}

}  // namespace
