// The skinny "down" product of the LoRA adapters: T[M, R] = X[M, K] . A[R, K]^T for R <= 256 - the training forward's T = x A_cat^T and the backward's
// dT = dY B_bd (A = B_bd^T [R, N], the contraction then runs over N). HBM-bound: X is read once and does R FLOP per byte; ug_gemm_bf16 with a 64-wide
// output runs the same product as one tile column of its 128^2 kernel.
//   ug_lora_down_bf16   a workgroup of 4 waves owns 32 rows of X and the FULL K; wave w takes the 64-wide K chunks w, w + 4, ... Both operands are
//                       K-major, so a lane's MFMA fragment is 8 consecutive k of one row: it is loaded straight from global memory (X: once, no
//                       reuse, so LDS would add nothing; A: R x K x 2 bytes, L2-resident). The order of k inside a chunk is free as long as both
//                       operands agree: lane (row, h) takes the 32 consecutive k at 32 h, so it reads 64 contiguous bytes per chunk.
//                       The four waves' fp32 partial tiles meet in LDS and are added in wave order (fixed: bit-identical run to run); bf16 output
//                       with a leading dimension. Rows >= M of the last block are loaded from row M - 1 and not stored.
// Measured (tools/lora_down_ab.py, profiles/r07_lora_down_ab.log): 1.7x faster than ops.gemm at N = 64 for M = 8192, 0.6x at M = 18432 (1.4 TB/s: the
// 16-byte fragment loads at a 64-byte lane stride do not stream) - not a win across the shapes, so probe library only; the product path keeps ops.gemm.
#include "ug_common.h"
#include "../unigen_hip_probe.h"   // probe library only: not part of the product C ABI

namespace {

template <int NB>      // R / 32 column blocks of the output tile
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ X, int64_t ldx, const bf16_t* __restrict__ A, int64_t lda,
                                                        bf16_t* __restrict__ T, int64_t ldt, int M, int K) {
    extern __shared__ __attribute__((aligned(16))) float red[];      // [3 waves][NB][16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 32;
    const int row = m0 + r < M ? m0 + r : M - 1;
    const bf16_t* xp = X + (int64_t)row * ldx + 32 * h;
    const bf16_t* ap = A + (int64_t)r * lda + 32 * h;
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
    for (int k0 = wave * 64; k0 < K; k0 += 256) {
        bf16x8 xf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) xf[s] = *(const bf16x8*)(xp + k0 + 8 * s);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            bf16x8 af[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) af[s] = *(const bf16x8*)(ap + (int64_t)nb * 32 * lda + k0 + 8 * s);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[s], af[s], acc[nb], 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) red[(((wave - 1) * NB + nb) * 16 + i) * 64 + lane] = acc[nb][i];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float v = acc[nb][i];
#pragma unroll
            for (int w = 0; w < 3; ++w) v += red[((w * NB + nb) * 16 + i) * 64 + lane];
            // accumulator element i of lane (n = lane & 31, h): row (i & 3) + 8 (i >> 2) + 4 h of the 32 x 32 block, column n
            const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (m < M) T[(int64_t)m * ldt + nb * 32 + r] = f2bf(v);
        }
}

template <int NB>
void launch_down(const bf16_t* X, int64_t ldx, const bf16_t* A, int64_t lda, bf16_t* T, int64_t ldt, int M, int K, hipStream_t stream) {
    const size_t lds = 3 * NB * 16 * 64 * sizeof(float);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)lora_down_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(lora_down_kernel<NB>, dim3((unsigned)((M + 31) / 32)), dim3(256), lds, stream, X, ldx, A, lda, T, ldt, M, K);
}

int lora_down_impl(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int64_t M, int64_t R, int64_t K, ug_stream_t stream) {
    const char* name = "ug_lora_down_bf16";
    UG_REQUIRE(X && A && T && M > 0 && R > 0 && K > 0 && ldx >= K && lda >= K && ldt >= R, UG_ERR_BAD_SHAPE, "%s: bad arguments", name);
    UG_REQUIRE(R % 64 == 0 && R <= 256 && K % 64 == 0, UG_ERR_UNSUPPORTED, "%s: R must be 64, 128, 192 or 256 and K a multiple of 64 (R = %lld, K = %lld)", name,
               (long long)R, (long long)K);
    UG_REQUIRE(ldx % 8 == 0 && lda % 8 == 0 && ug_aligned(X, 16) && ug_aligned(A, 16), UG_ERR_BAD_ALIGN,
               "%s: leading dimensions of X and A must be multiples of 8, bases 16-byte aligned", name);
    UG_REQUIRE(M < (1ll << 31) - 64 && K < (1ll << 31) - 256, UG_ERR_UNSUPPORTED, "%s: sizes must fit 31 bits", name);
    hipStream_t st = (hipStream_t)stream;
    const bf16_t* x = (const bf16_t*)X; const bf16_t* a = (const bf16_t*)A; bf16_t* t = (bf16_t*)T;
    switch (R / 32) {
        case 2: launch_down<2>(x, ldx, a, lda, t, ldt, (int)M, (int)K, st); break;
        case 4: launch_down<4>(x, ldx, a, lda, t, ldt, (int)M, (int)K, st); break;
        case 6: launch_down<6>(x, ldx, a, lda, t, ldt, (int)M, (int)K, st); break;
        default: launch_down<8>(x, ldx, a, lda, t, ldt, (int)M, (int)K, st); break;
    }
    UG_CHECK_LAUNCH(name);
    return UG_OK;
}

}  // namespace

extern "C" int ug_lora_down_bf16(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int64_t M, int64_t R, int64_t K,
                                 ug_stream_t stream) {
    return lora_down_impl(X, ldx, A, lda, T, ldt, M, R, K, stream);
}
