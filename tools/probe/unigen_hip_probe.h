/* Entry points that exist only in the PROBE library (python -m unigen_amd.build --probe -> tools/probe/libunigen_hip_probe.so): kernels that were
 * built, measured and dropped from the product path, kept for A/B measurements. Not part of the product C ABI (include/unigen_hip.h). */
#pragma once
#include "../../include/unigen_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* C[I][J] = sum_r A[r][I] * B[r][J], bf16 in / out, fp32 accumulation: dW = dY^T X of a Linear layer (A = dY [rows][out_features],
 * B = X [rows][in_features]) straight from the row-major operands - both MFMA fragments come from transposing LDS reads, no transposed copies.
 * I, J, lda, ldb multiples of 8. Measured 6 % slower per training step than two ug_transpose + the 256^2 ug_gemm_bf16 (round 2). */
int ug_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t R, int64_t I, int64_t J, ug_stream_t stream);
/* T[m][r] = sum_k X[m][k] * A[r][k]: X [M, K] and A [R, K] row-major (leading dimensions multiples of 8, bases 16-byte aligned), fp32 accumulation,
 * T [M, R] with leading dimension ldt (a column block of a wider buffer is fine). R = 64, 128, 192 or 256; K a multiple of 64; any M > 0. The training
 * forward's T = x A_cat^T and the backward's dT = dY B_bd (A = B_bd^T, K = N). The K range is split across the waves of a workgroup and added in a
 * fixed order: bit-identical run to run. Measured against ug_gemm_bf16 at N = 64: 1.7x faster at M = 8192, 0.6x at M = 18432 (profiles/r07_lora_down_ab.log). */
int ug_lora_down_bf16(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int64_t M, int64_t R, int64_t K, ug_stream_t stream);
#ifdef __cplusplus
}
#endif
