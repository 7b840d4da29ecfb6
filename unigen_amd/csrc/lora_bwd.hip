// The skinny products of the LoRA adapters' backward (unigen_amd/autograd.py, the LoRA-carrying linears): with y = x W^T + b + (x A_cat^T) B_bd^T,
// T = x A_cat^T and R = the padded rank (64 ... 256),
//     dA_cat = dT^T X   [R, K]   contraction over the M rows
//     dB_bd^T = T^T dY  [R, N]   contraction over the M rows
// Both read one large activation ([M, K] or [M, N]) once and do R FLOP per byte of it: HBM-bound. The route through ug_gemm_bf16 needs zero-padded
// transposed copies of BOTH operands (the activation is then written once more and read twice); here both operands stay row-major.
//   ug_lora_wgrad_bf16   C[R, J] = alpha * sum_m P[m, :R]^T Q[m, :J]: P [M, R], Q [M, J] row-major bf16. Both arrive contraction-major, so both MFMA
//                        fragments are transposed reads (ds_read_b64_tr_b16) out of 64-row tiles in the 256-byte-row swizzled image that the
//                        attention kernel uses for V^T. The output has R / 64 tile rows only, so the M rows are split across workgroups as
//                        well as J; a split writes an fp32 slab into the caller's workspace and a second launch adds the slabs in the order of
//                        the splits (no float atomics: bit-identical run to run). The last, partial 64-row block of M is zero-filled in LDS.
//                        dB_bd is produced as its transpose [R, N] (P = T, Q = dY); the caller views it.
//   ug_lora_wgrad_f32    the fp32 verification twin: plain FMA chains over the same splits, the same slab reduction.
#include "ug_common.h"

namespace {

typedef __attribute__((address_space(3))) bf16x4* lds_b64_ptr;

__device__ __forceinline__ int lw_row_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }       // as attention.hip, 256-byte rows
__device__ __forceinline__ int lw_img_off(int row, int ch) { return 256 * row + 16 * (ch ^ lw_row_swz(row)); }
__device__ __forceinline__ bf16x8 lw_tr_pair(const unsigned char* lo, const unsigned char* hi) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64_ptr)lo);
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64_ptr)hi);
    return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

constexpr int LW_TILE = 64 * 256;      // one operand tile image: 64 rows x 256 bytes (P uses the chunks 0 .. 7 of a row, Q all 16)
constexpr int LW_BR = 64, LW_BJ = 128; // output tile of a workgroup
constexpr int LW_TARGET_WGS = 512;     // two workgroups per CU on 256 CUs
constexpr int LW_MIN_BLOCKS = 4;       // at least 256 rows per split: a slab (32 KiB per tile) stays well under the operand bytes of its split

// 64 x 128 output tile over the rows [blk_lo, blk_hi) * 64 of one split: 4 waves as 2 (R) x 2 (J), each 32 x 64 = two 32x32x16 accumulators; two tile
// pairs in LDS (64 KiB, 2 workgroups / CU), register staging one tile ahead. grid = (J tiles, splits, R / 64).
__global__ __launch_bounds__(256, 2) void lora_wgrad_kernel(const bf16_t* __restrict__ P, int64_t ldp, const bf16_t* __restrict__ Q, int64_t ldq,
                                                            bf16_t* __restrict__ C, int64_t ldc, float* __restrict__ slab, int M, int R, int J,
                                                            int blocks_per_split, float alpha) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [2][P tile | Q tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int j0 = blockIdx.x * LW_BJ, r0 = blockIdx.z * LW_BR;
    const int nblk = (M + 63) / 64;
    const int blk_lo = blockIdx.y * blocks_per_split;
    const int blk_hi = blk_lo + blocks_per_split < nblk ? blk_lo + blocks_per_split : nblk;
    // staging: thread -> 2 chunks (16 bytes) of the P tile, 4 of the Q tile
    u32x4 rp[2], rq[4];
    auto stage_load = [&](int m0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int cid = tid + 256 * u, m = m0 + (cid >> 3), ch = cid & 7;
            rp[u] = (u32x4){0u, 0u, 0u, 0u};
            if (m < M) rp[u] = *(const u32x4*)(P + (int64_t)m * ldp + r0 + ch * 8);          // R is a multiple of 64: the tile's columns exist
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cid = tid + 256 * u, m = m0 + (cid >> 4), cj = j0 + (cid & 15) * 8;
            rq[u] = (u32x4){0u, 0u, 0u, 0u};
            if (m < M && cj < J) rq[u] = *(const u32x4*)(Q + (int64_t)m * ldq + cj);         // J is a multiple of 64: a chunk is in or out as a whole
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int cid = tid + 256 * u;
            *(u32x4*)(smem + buf * 2 * LW_TILE + lw_img_off(cid >> 3, cid & 7)) = rp[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cid = tid + 256 * u;
            *(u32x4*)(smem + buf * 2 * LW_TILE + LW_TILE + lw_img_off(cid >> 4, cid & 15)) = rq[u];
        }
    };
    // transposed-read offsets (attention.hip's V^T pattern): lane -> column 32 blk + (lane & 31), rows 16 ks + {4h + (i16 >> 2), + 8}
    const int h = lane >> 5, i16 = lane & 15, g16 = lane >> 4;
    const int t_row = 4 * h + (i16 >> 2), t_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1), t_b8 = 8 * (i16 & 1);
    int off_lo[4], off_hi[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const int ch = 4 * blk + t_lowch;
        off_lo[blk] = 256 * t_row + 16 * (ch ^ lw_row_swz(t_row)) + t_b8;
        off_hi[blk] = 256 * (t_row + 8) + 16 * (ch ^ lw_row_swz(t_row + 8)) + t_b8;
    }
    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    if (blk_lo < blk_hi) {                                       // (workgroup-uniform: every lane takes part in the transposed reads)
        stage_load(blk_lo * 64);
        stage_write(0);
        __syncthreads();
        for (int t = blk_lo; t < blk_hi; ++t) {
            const int cur = (t - blk_lo) & 1;
            if (t + 1 < blk_hi) stage_load((t + 1) * 64);
            const unsigned char* Pb = smem + cur * 2 * LW_TILE;
            const unsigned char* Qb = Pb + LW_TILE;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 pf = lw_tr_pair(Pb + ks * 16 * 256 + off_lo[wi], Pb + ks * 16 * 256 + off_hi[wi]);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const bf16x8 qf = lw_tr_pair(Qb + ks * 16 * 256 + off_lo[wj * 2 + b], Qb + ks * 16 * 256 + off_hi[wj * 2 + b]);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, qf, acc[b], 0, 0, 0);
                }
            }
            if (t + 1 < blk_hi) stage_write(cur ^ 1);
            __syncthreads();
        }
    }
    // accumulator element i of lane (n = lane & 31, h): row (i & 3) + 8 (i >> 2) + 4 h of the 32 x 32 block
    const int n = lane & 31;
    float* sl = slab ? slab + (int64_t)blockIdx.y * R * J : nullptr;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = j0 + wj * 64 + b * 32 + n;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = r0 + wi * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;         // < R: R is a multiple of 64
            if (col < J) {
                if (sl) sl[(int64_t)row * J + col] = acc[b][i];
                else C[(int64_t)row * ldc + col] = f2bf(alpha * acc[b][i]);
            }
        }
    }
}

// fp32 twin: one thread per output column, 4 rank rows per thread, a plain FMA chain over the rows of its split. grid = (J / 256, splits, R / 4).
__global__ __launch_bounds__(256) void lora_wgrad_f32_kernel(const float* __restrict__ P, int64_t ldp, const float* __restrict__ Q, int64_t ldq,
                                                             float* __restrict__ slab, int M, int R, int J, int blocks_per_split) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.z * 4;
    const int m_lo = blockIdx.y * blocks_per_split * 64;
    const int m_end = m_lo + blocks_per_split * 64, m_hi = m_end < M ? m_end : M;
    if (j >= J) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int m = m_lo; m < m_hi; ++m) {
        const float q = Q[(int64_t)m * ldq + j];
        const f32x4 p = *(const f32x4*)(P + (int64_t)m * ldp + r);
        a0 = fmaf(p[0], q, a0); a1 = fmaf(p[1], q, a1); a2 = fmaf(p[2], q, a2); a3 = fmaf(p[3], q, a3);
    }
    float* sl = slab + (int64_t)blockIdx.y * R * J + (int64_t)r * J + j;
    sl[0] = a0; sl[J] = a1; sl[2 * (int64_t)J] = a2; sl[3 * (int64_t)J] = a3;
}

// C[r][j] = alpha * (slab 0 + slab 1 + ...)[r][j], in the order of the splits; 4 columns per thread.
template <typename T>
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ slab, T* __restrict__ C, int64_t ldc, int R, int J, int splits,
                                                                float alpha) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int jq = J >> 2;
    if (id >= (int64_t)R * jq) return;
    const int r = (int)(id / jq), j = (int)(id - (int64_t)r * jq) * 4;
    f32x4 s = *(const f32x4*)(slab + (int64_t)r * J + j);
    for (int k = 1; k < splits; ++k) {
        const f32x4 v = *(const f32x4*)(slab + ((int64_t)k * R + r) * J + j);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    T* o = C + (int64_t)r * ldc + j;
#pragma unroll
    for (int e = 0; e < 4; ++e) ElemT<T>::st(o + e, alpha * s[e]);
}

// 64-row blocks of M per split: enough splits to fill the chip with J tiles x splits x R tiles workgroups, never under LW_MIN_BLOCKS blocks each.
// A function of the shape only, so a shape always reduces in the same order.
void lw_splits(int64_t M, int64_t R, int64_t J, int64_t* blocks_per_split, int64_t* splits) {
    const int64_t nblk = (M + 63) / 64, tiles = ((J + LW_BJ - 1) / LW_BJ) * (R / LW_BR);
    int64_t want = (LW_TARGET_WGS + tiles - 1) / tiles;
    const int64_t most = (nblk + LW_MIN_BLOCKS - 1) / LW_MIN_BLOCKS;
    if (want > most) want = most;
    if (want < 1) want = 1;
    *blocks_per_split = (nblk + want - 1) / want;
    *splits = (nblk + *blocks_per_split - 1) / *blocks_per_split;
}

template <typename T>
int lora_wgrad_impl(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int64_t M, int64_t R, int64_t J, float alpha,
                    void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    constexpr bool F32 = ElemT<T>::kF32;
    const char* name = F32 ? "ug_lora_wgrad_f32" : "ug_lora_wgrad_bf16";
    UG_REQUIRE(P && Q && C && M > 0 && R > 0 && J > 0 && ldp >= R && ldq >= J && ldc >= J, UG_ERR_BAD_SHAPE, "%s: bad arguments", name);
    UG_REQUIRE(R % 64 == 0 && R <= 256 && J % 64 == 0, UG_ERR_UNSUPPORTED, "%s: R must be 64, 128, 192 or 256 and J a multiple of 64 (R = %lld, J = %lld)",
               name, (long long)R, (long long)J);
    UG_REQUIRE(ldp % 8 == 0 && ldq % 8 == 0 && ug_aligned(P, 16) && ug_aligned(Q, 16), UG_ERR_BAD_ALIGN,
               "%s: leading dimensions of P and Q must be multiples of 8, bases 16-byte aligned", name);
    UG_REQUIRE(M < (1ll << 31) - 64 && J < (1ll << 31) - 256, UG_ERR_UNSUPPORTED, "%s: sizes must fit 31 bits", name);
    int64_t bps, splits;
    lw_splits(M, R, J, &bps, &splits);
    UG_REQUIRE(splits <= 65535, UG_ERR_UNSUPPORTED, "%s: too many row splits", name);
    const bool direct = !F32 && splits == 1;                    // one split: the tile's owner rounds and stores, no slab
    if (!direct) {
        UG_REQUIRE(workspace && ug_aligned(workspace, 16) && workspace_bytes >= splits * R * J * (int64_t)sizeof(float), UG_ERR_BAD_SHAPE,
                   "%s: workspace of ug_lora_wgrad_workspace_bytes() needed", name);
    }
    float* slab = direct ? nullptr : (float*)workspace;
    if constexpr (F32) {
        hipLaunchKernelGGL(lora_wgrad_f32_kernel, dim3((unsigned)((J + 255) / 256), (unsigned)splits, (unsigned)(R / 4)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)P, ldp, (const float*)Q, ldq, slab, (int)M, (int)R, (int)J, (int)bps);
    } else {
        (void)hipFuncSetAttribute((const void*)lora_wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * LW_TILE);   // per call: any device, any thread
        hipLaunchKernelGGL(lora_wgrad_kernel, dim3((unsigned)((J + LW_BJ - 1) / LW_BJ), (unsigned)splits, (unsigned)(R / LW_BR)), dim3(256), 4 * LW_TILE,
                           (hipStream_t)stream, (const bf16_t*)P, ldp, (const bf16_t*)Q, ldq, (bf16_t*)C, ldc, slab, (int)M, (int)R, (int)J, (int)bps, alpha);
    }
    if (!direct)
        hipLaunchKernelGGL(lora_wgrad_reduce_kernel<T>, dim3((unsigned)((R * (J / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)slab,
                           (T*)C, ldc, (int)R, (int)J, (int)splits, alpha);
    UG_CHECK_LAUNCH(name);
    return UG_OK;
}

}  // namespace

extern "C" int64_t ug_lora_wgrad_workspace_bytes(int64_t M, int64_t R, int64_t J) {
    if (M <= 0 || R <= 0 || J <= 0 || R % 64 != 0) return 0;
    int64_t bps, splits;
    lw_splits(M, R, J, &bps, &splits);
    return splits * R * J * (int64_t)sizeof(float);
}
extern "C" int ug_lora_wgrad_bf16(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int64_t M, int64_t R, int64_t J, float alpha,
                                  void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    return lora_wgrad_impl<bf16_t>(P, ldp, Q, ldq, C, ldc, M, R, J, alpha, workspace, workspace_bytes, stream);
}
extern "C" int ug_lora_wgrad_f32(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int64_t M, int64_t R, int64_t J, float alpha,
                                 void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    return lora_wgrad_impl<float>(P, ldp, Q, ldq, C, ldc, M, R, J, alpha, workspace, workspace_bytes, stream);
}
