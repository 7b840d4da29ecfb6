/*
 * unigen_hip.h — C ABI of libunigen_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for ONE hot path of gavin-gqzhang/UniGen: the
 * condition-weaving + expert-modulation diffusion forward pass
 * (reference: src/UniGenTransformer.py:712-1450 UniGenFlux / MultiCondtionUniGenFlux,
 *  src/UniGenUtils.py:17-228,340-622, denoise loop src/UniGenPipeline.py:721-789).
 *
 * The reference has no FFI of its own (it is pure PyTorch eager); every entry point
 * below names the reference torch call site it replaces. Conventions:
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - asynchronous, stream-ordered on `stream` (a hipStream_t passed as void*);
 *     no allocation, no ownership transfer, no host synchronisation.
 *   - bf16 storage (uint16 bit patterns), fp32 accumulate / statistics / gate / RoPE tables.
 *   - every compute entry point has an fp32 VERIFICATION twin `<name>_f32` (section at the end): identical argument
 *     meaning, fp32 storage for every tensor that is bf16 here, no intermediate rounding. Slow, correctness-first
 *     kernels; the Python host runs the SAME orchestration through them when the model's parameters are fp32, which
 *     is how forward-level parity with the reference is shown to <= 1e-3 (a bf16 forward cannot be: eps = 7.8e-3).
 *   - return 0 on success, a negative UG_ERR_* otherwise; ug_last_error() gives the
 *     thread-local message of the most recent failure.
 *   - "row map": a logical row m of an operand lives at physical row
 *         (m / rows_per_batch) * batch_stride + (m % rows_per_batch)
 *     of its buffer (rows_per_batch == 0 means identity). It lets a GEMM read or write
 *     a token slice of a concatenated (text|image|condition) buffer without a copy.
 */
#ifndef UNIGEN_HIP_H
#define UNIGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ug_stream_t; /* hipStream_t */

enum {
    UG_OK = 0,
    UG_ERR_BAD_SHAPE = -1,
    UG_ERR_BAD_ALIGN = -2,
    UG_ERR_UNSUPPORTED = -3,
    UG_ERR_HIP = -4
};

/* GEMM epilogues (ug_gemm_desc.epilogue). v = bf16(acc + bias) is rounded first, as the
 * reference's separate nn.Linear does, then: */
enum {
    UG_EPI_BIAS = 0,       /* C = v                                            nn.Linear */
    UG_EPI_BIAS_GELU = 1,  /* C = gelu_tanh(v)                                 FeedForward net.0 (diffusers GELU approximate="tanh") */
    UG_EPI_RES_GATE = 2,   /* C = R + gate[sample(m)][n] * v                   x + gate.unsqueeze(1) * attn/ff  (FluxTransformerBlock) */
    UG_EPI_RES_SCALE = 3,  /* C = R + alpha * v                                x + cn_block(z) * conditioning_scale (UniGenTransformer.py:1104,1141) */
    UG_EPI_F32 = 4,        /* C(fp32) = acc + bias (no rounding; verification / gate logits) */
    UG_EPI_QKV_ROPE = 5    /* fused [to_q; to_k; to_v (; proj_mlp)] projection: columns [0, qk_until_n) are q | k heads of 128 and get
                              Attention.norm_q / norm_k (RMSNorm) + apply_rotary_emb in the epilogue (src/UniGenUtils.py:561-599, the work of
                              ug_qk_rmsnorm_rope); the other columns behave as UG_EPI_BIAS, or GELU from gelu_from_n > 0 on */
};

typedef struct ug_gemm_desc {
    /* C[m][n] = epilogue( sum_k A[m][k] * W[n][k] + bias[n] ), all bf16, W in nn.Linear layout [N][K].
     * Row maps (x_rpb, x_bstride): logical row m sits at physical row (m / rpb) * bstride + m % rpb (rpb 0: m itself). The A map may be
     * anything (bstride < rpb broadcasts a batch); a NON-MONOTONIC A map (bstride < rpb) is served by the 128^2 kernel only - the 256^2
     * kernel's DMA offsets are unsigned distances from a tile's first row - and is refused (UG_ERR_BAD_SHAPE) with UG_EPI_QKV_ROPE. */
    const void* A; int64_t lda; int64_t a_rpb; int64_t a_bstride;
    const void* W; int64_t ldw;
    const void* bias;                 /* [N] bf16 or NULL */
    void* C; int64_t ldc; int64_t c_rpb; int64_t c_bstride;
    const void* R; int64_t ldr; int64_t r_rpb; int64_t r_bstride; /* residual; MAY ALIAS C (same base, ld and row map): every kernel path reads a residual element before the store that overwrites it (tests/test_kernels_gpu.py::test_gemm_residual_aliased_to_output_every_dispatch_path) */
    const void* gate; int64_t gate_ld; int64_t rows_per_sample;   /* gate[(m / rows_per_sample) * gate_ld + n] bf16 */
    float alpha;
    int32_t epilogue;
    int64_t M, N, K;
    /* grouped / batched over `groups` experts (blockIdx.z); strides in ELEMENTS */
    int32_t groups; int32_t _pad0;
    int64_t a_gstride, w_gstride, bias_gstride, c_gstride;
    /* optional LoRA epilogue (peft 0.15 Linear; src/lora_switching_module.py:11-38):
     *   acc += lora_scale-premultiplied T[m][0..r) . B[n][0..r)   with T = scale * (x A^T) computed by a prior ug_gemm_bf16 */
    const void* lora_T; int64_t ldt;
    const void* lora_B; int64_t ldb;
    int32_t lora_r; int32_t _pad1;
    /* group strides (ELEMENTS) of the residual and gate operands for grouped residual epilogues (per-expert transformer blocks) */
    int64_t r_gstride, gate_gstride;
    /* optional caller-owned scratch (>= ug_gemm_workspace_bytes(), 16-byte aligned) for the split-K treatment of the last, partially
     * filled round of tiles; NULL = plain tiles only. Its first 4096 bytes (arrival tickets) must be ZERO before the first call;
     * every call leaves them zero again. The rest needs no initialisation. One workspace per stream. A launch writes only the slabs of its
     * own K-slices (bytes [4096, 4096 + padded tail tiles x K-slices x 256 KiB)); a workspace too small for them is not an error: that launch
     * runs unsplit, with the result of workspace = NULL, and does not touch it (tests/test_workspace_gpu.py). */
    void* workspace; int64_t workspace_bytes;
    /* Column split, for one launch over the concatenated weights of two Linear layers that read the same input (the single block's
     * [to_q; to_k; to_v; proj_mlp], diffusers FluxSingleTransformerBlock, called at src/UniGenTransformer.py:1151):
     *   UG_EPI_BIAS_GELU applies GELU only to columns n >= gelu_from_n (0: all columns);
     *   output column n is stored at column n + c_shift when n >= c_shift_from_n > 0 (a gap in the destination row).
     * Both boundaries must be multiples of 256 (a tile never straddles them); c_shift a multiple of 8. */
    int64_t gelu_from_n, c_shift_from_n, c_shift;
    /* UG_EPI_QKV_ROPE only. Heads are qk_dh wide (128; 0 means 128; or 64: SD3.5); q heads fill columns [0, qk_until_n / 2), k heads
     * [qk_until_n / 2, qk_until_n).
     *   qk_wq, qk_wk : [qk_dh] bf16 RMSNorm weights;  rope_cs : fp32 [positions][qk_dh / 2][2] = (cos, sin) of each rotation pair (may be NULL
     *   at qk_dh = 64: RMSNorm only, JointAttnProcessor2_0 has no RoPE);
     *   row m sits at position rope_pos0 + (m % rope_rpb) (rope_rpb 0: m itself).
     * Needs M, N, qk_until_n multiples of 256, groups 1, no LoRA segment, 16-byte aligned C rows. */
    const void* qk_wq; const void* qk_wk; const float* rope_cs;
    int64_t rope_rpb, rope_pos0, qk_until_n;
    float qk_eps; int32_t qk_dh;
} ug_gemm_desc;

/* bytes of ug_gemm_desc.workspace that are always sufficient (any shape) */
int64_t ug_gemm_workspace_bytes(void);

/* replaces every nn.Linear on the path (torch F.linear -> BLAS) incl. fused epilogues. */
int ug_gemm_bf16(const ug_gemm_desc* d, ug_stream_t stream);

/* Which kernel ug_gemm_bf16 launches for a descriptor, and how - the dispatcher's own answer (gemm_check, then gemm_plan of csrc/gemm.hip),
 * computed on the host: no device, no HIP call, no pointer dereferenced (pointer VALUES count: alignment, workspace NULL or not).
 * ug_gemm_plan(d, ncu, force_tile, out): the plan of *d on a chip of ncu > 0 compute units under UG_GEMM_FORCE_TILE = force_tile (0: none).
 * Returns what ug_gemm_bf16 returns for a refused descriptor (same code, same message), else UG_OK with *out filled; M == 0 (nothing to launch)
 * gives UG_OK and an all-zero *out. ug_gemm_bf16(d) launches ug_gemm_plan(d, CUs of the device, UG_GEMM_FORCE_TILE).
 *
 * The dispatch rules, in the order they apply (T256 / T128 = tiles of 256^2 / 128^2 over all groups, KT = K / 64 K-tiles):
 *   1. Fill: the 256^2 kernel (one persistent workgroup per CU) when M, N >= 192 and T256 / roundup(T256, 256) >= 0.6 T128 / roundup(T128, 512).
 *   2. Small M: a launch that lost rule 1 with M, N >= 192 and T256 < ncu still takes the 256^2 kernel when rule 7 would split it and the
 *      priced split (1.53 KT / slices + 22 + 2.5 slices us) is below 0.9 x the 128^2 kernel's rounds (0.97 or 1.27 us per K-tile). Not UG_EPI_F32.
 *   3. force_tile 128 / 256 overrides rules 1-2.
 *   4. The 256^2 kernel addresses a tile's A and W rows by unsigned 32-bit byte offsets from the tile's first row: a non-monotonic A row map
 *      (a_bstride < a_rpb), or 255 rows (plus the A map's batch jumps inside them) + K elements reaching 2^31 bytes, go to the 128^2 kernel.
 *   5. A LoRA segment (lora_r > 0) takes the 256^2 kernel's LoRA variant only with K >= 128 and not under UG_EPI_F32, skips rule 4, never splits.
 *   6. UG_EPI_QKV_ROPE exists in the 256^2 kernel only (variant by head width): what rule 4 sends away is refused there; rules 1-3 do not apply.
 *   7. Split-K tail: the T256 % ncu tiles of the last round, padded to a multiple of 8 (rem8), are each cut into
 *      nslices = min(ncu / rem8, 8, KT / 4) K-slices when there are any, they fill at most half the CUs, KT >= 96, nslices >= 2 and the
 *      workspace is there, 16-byte aligned and holds 4096 + rem8 nslices 256 KiB; with T256 < ncu the grid is rem8 x nslices workgroups.
 *   8. wide16 bit 0: 16-byte epilogue accesses (N, ldc, c_gstride multiples of 8, C 16-byte aligned; the same of R under a residual epilogue);
 *      bit 1: one row map per tile (c_rpb, and r_rpb under a residual epilogue, multiples of 256).
 *   9. ug_conv2d_nhwc takes the 256^2 kernel's convolution variant (A gathered per filter tap) when B Ho Wo and Cout are multiples of 256,
 *      Cin / 64 is a power of two >= 2, K >= 3 K-tiles, there are at least UG_CONV256_MIN_TILES (192) tiles, B < 256, H, W < 2048, Ho, Wo < 4096,
 *      out and R are 16-byte aligned and the zero page holds 2 (Cin + 64) bytes; UG_CONV256=0 switches it off. No split-K tail. */
enum { UG_GEMM_PLAIN = 0, UG_GEMM_LORA = 1, UG_GEMM_QK128 = 2, UG_GEMM_QK64 = 3, UG_GEMM_CONV = 4 };
typedef struct ug_gemm_dispatch {
    int32_t tile;                                   /* 128 or 256 */
    int32_t variant;                                /* UG_GEMM_*: the 256^2 kernel's instantiation besides the epilogue (128^2: UG_GEMM_PLAIN) */
    int32_t grid, grid_z;                           /* workgroups: 256^2 min(tiles, ncu) or rule 7's, z = 1; 128^2 tiles of one group, z = groups */
    int32_t tiles, tiles_per_group;                 /* 256^2 tiles in all and per group (128^2: 0) */
    int32_t rounds, full_tiles, nslices, rem8;      /* rounds of the persistent walk; tiles before the split tail; rule 7 (1, 0: no split) */
    int32_t wide16, group_m, walk;                  /* rule 8; M-tiles per group of the tile walk and the walk's form (0 on the 128^2 kernel) */
    int32_t lds_bytes;                              /* dynamic LDS of the launch */
} ug_gemm_dispatch;
int ug_gemm_plan(const ug_gemm_desc* d, int32_t ncu, int32_t force_tile, ug_gemm_dispatch* out);

/* out[m][n] = R[m][n] + bf16( sum_k act(x[m][k]) * W[n][k] + b[n] ),  M <= 16 rows (per-sample vectors).
 * act: 0 none, 1 SiLU. Replaces AdaLayerNormZero.linear(silu(emb)), TimestepEmbedding, PixArtAlphaTextProjection
 * (diffusers 0.32.2 normalization.py / embeddings.py; called from UniGenTransformer.py:1222,1048-1049). */
int ug_small_linear_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                         const void* R, int64_t ldr, void* out, int64_t ldo,
                         int64_t M, int64_t N, int64_t K, int32_t act_in, ug_stream_t stream);

/* out = LayerNorm(x; eps, no affine) * (1 + scale[sample]) + shift[sample]   (AdaLayerNormZero / norm2+modulate /
 * AdaLayerNormContinuous; diffusers normalization.py; src/UniGenUtils.py:354-373). shift/scale are bf16 rows of the
 * adaLN linear output with leading dimension mod_ld. */
int ug_adaln_modulate(const void* x, int64_t ldx, int64_t x_rpb, int64_t x_bstride,
                      const void* shift, const void* scale, int64_t mod_ld, int64_t rows_per_sample,
                      void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream);

/* In-place RMSNorm(q), RMSNorm(k) (per head, weight) then RoPE on a fused [.. q | k | v ..] projection buffer.
 * Row r in [0, rows_per_batch) of batch b is at buf + (b*batch_stride_rows + r)*ld and has sequence position
 * pos = pos_offset + r. Positions < split use (wq_a, wk_a) (text: norm_added_q/k), positions >= split use (wq_b, wk_b)
 * (image: norm_q/k). cos/sin: fp32 [>= pos_offset + rows_per_batch][dh] indexed by pos, or NULL (no RoPE);
 * weights may be NULL (no qk-norm). q_off < 0 skips q (k/v-only context streams).
 * Replaces Attention.norm_q/norm_k + apply_rotary_emb (FluxAttnProcessor2_0; src/UniGenUtils.py:561-599). */
int ug_qk_rmsnorm_rope(void* buf, int64_t ld, int64_t batches, int64_t rows_per_batch, int64_t batch_stride_rows,
                       int64_t pos_offset, int64_t q_off, int64_t k_off, int32_t heads, int32_t dh,
                       const void* wq_a, const void* wk_a, const void* wq_b, const void* wk_b, int64_t split,
                       const float* cos_tab, const float* sin_tab, float eps, ug_stream_t stream);

/* O = softmax(Q K^T / sqrt(dh)) V, non-causal, no mask; Q rows [Lq], K/V rows [Lkv]; head h occupies
 * columns [h*dh, (h+1)*dh) of each row. Strides in elements. Replaces F.scaled_dot_product_attention
 * (src/UniGenUtils.py:601 and diffusers FluxAttnProcessor2_0). dh in {64, 128}.
 *
 * Strided attention views. Every attention entry point takes each operand as a view (pointer, row stride, batch stride), strides in elements, so
 * that the column blocks of a packed buffer are read and written in place. One checker (csrc/ug_common.h: ug_check_views) applies, per view,
 * a multiple both strides must have, an alignment of the base in bytes (either missed: UG_ERR_BAD_ALIGN) and, for some, 0 < row stride < 2^24
 * (UG_ERR_UNSUPPORTED; looked at only when every view of the call is aligned). Batch strides are 64-bit everywhere.
 *   entry                                          stride multiple / base alignment                    row stride in (0, 2^24)
 *   ug_flash_attn_fwd, _fwd_lse                    q, k, v: 8 / 16;  o: 4 / 8                          q, k, v, o
 *   ug_flash_attn_fwd_wide                         q, k, v: 8 / 16;  o: 4 / 8                          k, v
 *   ug_flash_attn_fwd_bias (table or mask given)   q, k, v: 8 / 16;  o: 4 / 8                          none
 *   ug_flash_attn_fwd_f32, _bias_f32, _wide_f32    all: 4 / 16                                         none
 *   ug_flash_attn_bwd                              all eight: 8;  q, k, v, o, dout: 16;  dq, dk, dv: 8 all eight
 *   ug_linear_attn, _bwd (fp32 twins)              all: 8 (4) / 16;  workspace and state: 16           none
 *   ug_flash_attn_fwd_softcap (fp32 twin)          q, k, v: 8 (4) / 16;  o: 4 / 8 (4 / 16)              none
 * The bound is there because the bf16 kernels stream K / V (the backward: Q / dO too) with LDS-DMAs whose per-lane byte offsets over a 64-row tile
 * are 32-bit, 2 (63 rs + 120) < 2^32; the narrow entry points apply it to every row stride (the widest row of the package is 21 504). The fp32
 * twins and ug_flash_attn_fwd_bias with a table or a mask index in 64 bits. Before the views an entry point returns UG_OK when there is nothing to
 * do (batches or Lq / N zero: no pointer is looked at), then refuses null operands and non-positive counts (UG_ERR_BAD_SHAPE), then its head width
 * and a sequence of 2^30 or more (UG_ERR_UNSUPPORTED); after them come the grid limits and, in the backward, the workspace (UG_ERR_BAD_SHAPE). */
int ug_flash_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                      const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                      const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                      void* o, int64_t o_row_stride, int64_t o_batch_stride,
                      int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                      float softmax_scale, ug_stream_t stream);

/* ug_flash_attn_fwd at head width 512: the single-head mid-block attention of AutoencoderKL (diffusers Attention(heads = 1, dim_head = 512);
 * unigen_amd/vae.py), without the [Lq, Lkv] score matrix in memory. Same arguments; views as in "Strided attention views" above; any Lq, Lkv >= 1. dh must be 512
 * (UG_ERR_UNSUPPORTED otherwise; 64 and 128 stay with ug_flash_attn_fwd), softmax_scale > 0.
 * bf16 in / out, fp32 accumulation, online softmax, P rounded to bf16 as the P.V operand. No workspace, no atomics, no state between launches:
 * two launches give the same bits, and the launch can be captured in a graph (128 KiB of dynamic LDS; one workgroup = 128 query rows). */
int ug_flash_attn_fwd_wide(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                           const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                           const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                           void* o, int64_t o_row_stride, int64_t o_batch_stride,
                           int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                           float softmax_scale, ug_stream_t stream);

/* Sinusoidal Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0): out[b] = [cos(t f) | sin(t f)] as bf16.
 * (diffusers embeddings.get_timestep_embedding; called inside time_text_embed, UniGenTransformer.py:1222). */
int ug_timestep_embed(const float* t, void* out, int64_t ldo, int64_t B, int32_t dim, ug_stream_t stream);

/* x = bf16( float(x) + bf16( bf16(dt) * v ) )  FlowMatchEulerDiscreteScheduler.step (called at src/UniGenPipeline.py:768 / :411) as torch evaluates
 * `sample.float() + (sigma_next - sigma) * model_output`: the step is a 0-dim fp32 tensor, so the product is a bf16 op (both operands cast, result rounded)
 * before the fp32 add. dt = the fp32 difference of the scheduler's fp32 sigmas. (dt = -0.25, FLUX-schnell's four steps: exact.) _f32 twin: no rounding. */
int ug_euler_step(void* x, const void* v, float dt, int64_t n, ug_stream_t stream);

/* out = uncond + gs * (text - uncond), each step rounded to bf16 as the reference's tensor ops do: classifier-free guidance of
 * UniGenSD3Pipeline (src/UniGenPipeline.py:404-407). n elements, contiguous. */
int ug_cfg_combine(const void* uncond, const void* text, float guidance_scale, void* out, int64_t n, ug_stream_t stream);

/* One step of DPMSolverMultistepScheduler as Sana configures it (dpmsolver++, midpoint, solver_order <= 2, flow prediction, flow sigmas) over n
 * contiguous elements, in one launch: classifier-free guidance, the flow-to-x0 conversion, the first- or second-order update, the history and the
 * next forward's input. pred_uncond, pred_text (NULL: no guidance) and model_in (NULL allowed with copies = 0) are bf16, fp32 in the _f32 twin;
 * sample and x0_prev are fp32 in both. Per element, every line ONE IEEE fp32 operation (no FMA), as torch's tensor ops on fp32 latents round:
 *     p  = pred_text ? u + gs * (t - u) : u            u, t widened to fp32
 *     x0 = x - sigma * p
 *     o  = a * x - b * x0                              order 1 ends here
 *     o  = o - (0.5f * b) * (rinv * (x0 - m1))         order 2; m1 = x0_prev[i] as the previous step left it
 *     x0_prev[i] = x0;  sample[i] = o;  model_in[k * n + i] = o rounded to the predictions' type, for k < copies
 * sigma = sigma_s0; a = sigma_t / sigma_s0, b = alpha_t * (exp(-h) - 1), rinv = 1 / ((lambda_s0 - lambda_s1) / h), formed by the host in fp32
 * (unigen_amd/sana_pipeline.py). The last step has a = 0, b = -1: the result is x0. model_in stands for `torch.cat([latents] * copies).to(dtype)`.
 * A thread reads its 8 elements of every operand before it writes any: sample and x0_prev are updated in place, and model_in may be the very buffer
 * that holds the predictions (model_in + k n = pred_uncond / pred_text) once the transformer has finished reading it; any other overlap of model_in with
 * the predictions, or of sample / x0_prev with anything else, is undefined. n % 8 == 0 and 16-byte aligned pointers, or UG_ERR_BAD_ALIGN; order outside
 * {1, 2}: UG_ERR_UNSUPPORTED; a NULL pred_uncond, sample or x0_prev, copies < 0, or copies > 0 without model_in: UG_ERR_BAD_SHAPE. n == 0: UG_OK. */
int ug_dpm_step(const void* pred_uncond, const void* pred_text, float guidance_scale, float* sample, float* x0_prev, void* model_in, int32_t copies,
                int32_t order, float sigma, float a, float b, float rinv, int64_t n, ug_stream_t stream);

/* out = bf16(a + b) elementwise (bf16), rows x D with leading dims. */
int ug_add_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo,
                int64_t rows, int64_t D, ug_stream_t stream);

/* x[r][:] = bf16( float(x[r][:]) + table[r % rows_per_batch][:] ), table fp32: PatchEmbed's `(latent + pos_embed).to(latent.dtype)`
 * with the centre-cropped sincos table (diffusers embeddings.PatchEmbed.forward; UniGenSD3, src/UniGenTransformer.py:663,510). */
int ug_add_rowbcast_f32(void* x, int64_t ldx, const float* table, int64_t ldt, int64_t rows, int64_t rows_per_batch, int64_t D,
                        ug_stream_t stream);

/* out[i][:W] = src[idx[i]][:W] (zeros when idx[i] < 0): per-slot rows of per-sample tables (per-token AdaLN embeddings of the
 * SD3 transformer-block experts: the reference broadcasts temb per token and dispatches it, src/UniGenUtils.py:107-109). */
int ug_gather_rows(const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W,
                   ug_stream_t stream);

/* ---- CoMoE (src/UniGenUtils.py:74-191 MOELayer + deepspeed 0.16.5 top1gating; UniGenTransformer.py:925-1026) ---- */

/* Gate: xc = bf16(x + c); logits = xc.float() @ wg.float()^T (fp32); gates = softmax; idx = argmax.
 * Writes gates fp32 [S][E], idx int32 [S]. */
int ug_moe_gate_top1(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E,
                     float* gates, int32_t* idx, ug_stream_t stream);

/* Capacity selection with Random Token Selection (use_rts=True, drop_tokens=True): per expert keep the `capacity`
 * tokens with the largest uniform[s][idx[s]]; slot = rank of the token among kept tokens of its expert (token order).
 * Writes slot int32 [S] (-1 = dropped), token_of_slot int32 [E][capacity] (-1 = empty), exp_counts int64 [E]
 * (pre-drop counts, as deepspeed returns), l_aux fp32 scalar = E * sum_e mean_s(gates[s][e]) * mean_s(idx[s]==e). */
int ug_moe_capacity_rts(const float* gates, const int32_t* idx, const float* uniform, int64_t S, int32_t E,
                        int64_t capacity, int32_t* slot, int32_t* token_of_slot, int64_t* exp_counts, float* l_aux,
                        ug_stream_t stream);

/* ---- top-2 gating (control_params.top_num = 2 -> MoE(..., k = 2), src/UniGenTransformer.py:162,197 / :808,857 / :1565,1650; TopKGate then calls
 * deepspeed 0.16.5 sharded_moe.top2gating(logits, capacity_factor = 1, min_capacity = 4, drop_tokens = True, top2_2nd_expert_sampling = True),
 * a dependency that is not in /root/reference: restated from its published source, parity unpinned). Arrays over the two choices are
 * choice-major [2][S]. ---- */

/* Gate: gates = softmax(logits) fp32 [S][E] as ug_moe_gate_top1; idx[0][s] = argmax; idx[1][s] = argmax over the OTHER experts of
 * logits[s][e] + noise[s][e] (noise: the Gumbel(0, 1) sample deepspeed adds to the logits for its second choice, fp32 [S][E]; NULL = no
 * sampling, the second-largest logit). 2 <= E <= 16. */
int ug_moe_gate_top2(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E, const float* noise,
                     float* gates, int32_t* idx, ug_stream_t stream);

/* Capacity rule of top2gating (no random token selection): per expert the first choices take slots in token order, the second choices
 * follow behind ALL its first choices; a choice at or beyond `capacity` (= max(ceil(S / E * 2), 4) for the reference's settings) is dropped.
 * Writes slot int32 [2][S] (-1 = dropped), token_of_slot int32 [E][capacity] (-1 = empty; the layout ug_moe_dispatch_modulate reads),
 * weights fp32 [2][S] = the kept choices' gate probabilities over their sum clamped at FLT_EPSILON (0 for a dropped choice), exp_counts
 * int64 [E] = first + second choices before the drop, l_aux fp32 scalar = E * sum_e mean_s(gates[s][e]) * mean_s(idx[0][s] == e). */
int ug_moe_capacity_top2(const float* gates, const int32_t* idx, int64_t S, int32_t E, int64_t capacity, int32_t* slot,
                         int32_t* token_of_slot, float* weights, int64_t* exp_counts, float* l_aux, ug_stream_t stream);

/* deepspeed topkgating (TopKGate with k > 2: control_params.top_num > 2, src/UniGenTransformer.py:808 -> src/UniGenUtils.py:33-36): the gate.
 * gates fp32 [S][E] = softmax of the fp32 logits of bf16(x + c), logits fp32 [S][E] (the capacity rule ranks LOGITS), idx int32 [K][S] = the
 * token's K choices by descending logit (the lower expert index first among equal logits). 1 <= K <= E <= 16. No random draw. */
int ug_moe_gate_topk(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E, int32_t K, float* gates,
                     float* logits, int32_t* idx, ug_stream_t stream);

/* Capacity rule of topkgating (drop_policy "probs"): expert e keeps the `capacity` (= max(ceil(S / E * K), 4) for the reference's settings) largest
 * entries of its column of [logit if e is one of the token's K choices, else 0] over ALL S tokens - a chosen logit below zero loses to every
 * non-chooser's zero - ties in token order, -0.0 and +0.0 being equal (a chosen -0.0 ties with the zeros); a choice survives if its entry is kept. Writes slot int32 [K][S] (-1 = dropped; slots in token order
 * among the kept), token_of_slot int32 [E][capacity] (-1 = empty), weights fp32 [K][S] = the kept choices' gate probabilities over their sum
 * clamped at FLT_EPSILON, exp_counts int64 [E] = choosers before the drop, l_aux fp32 scalar = (E / K) * sum_e mean_s(gates[s][e]) * exp_counts[e] / S. */
int ug_moe_capacity_topk(const float* gates, const float* logits, const int32_t* idx, int64_t S, int32_t E, int32_t K, int64_t capacity,
                         int32_t* slot, int32_t* token_of_slot, float* weights, int64_t* exp_counts, float* l_aux, ug_stream_t stream);

/* Combine over a token's K <= 16 (expert, slot) pairs - einsum("sec,ecm->sm") src/UniGenUtils.py:183 with top2gating's / topkgating's combine weights:
 *   eh = bf16( sum_k bf16(weights[k][s]) * yh[idx[k][s]][slot[k][s]] )   (fp32 sum, one rounding; dropped choices contribute nothing),
 * ec likewise; residual sums, row map and `accumulate` exactly as ug_moe_combine. weights / idx / slot: [K][kstride], kstride >= S
 * (a slice of a longer token axis keeps its parent's stride). K = 1 with weights = the gate probability reproduces ug_moe_combine. */
int ug_moe_combine_topk(const void* yh, const void* yc, const float* weights, const int32_t* idx, const int32_t* slot, int32_t K,
                        int64_t kstride, int32_t E, int64_t capacity, const void* xs, const void* cs, int64_t ld_s, int64_t s_rpb,
                        int64_t s_bstride, void* out, int64_t ldo, int64_t S, int64_t D, int32_t accumulate, ug_stream_t stream);

/* Dispatch + expert modulation prologue (replaces einsum("sec,sm->ecm") src/UniGenUtils.py:140 and the s-scaling of
 * modulated_flatten src/UniGenUtils.py:204-228):
 *   out[e][slot][:] = bf16( mod[e][sample(tok)][:] * bf16( x[tok][:] + (add ? add[e][slot][:] : 0) ) ), zeros for empty slots.
 * mod: bf16, row of (expert e, sample b) at mod + e * mod_estride + b * mod_bstride (elements) = Linear(768->D)(pooled) of that
 * expert (all experts' linears run as ONE launch over their stacked weights, so the natural layout is [B][E][D]); NULL for a plain
 * dispatch (transformer-block experts). tokens_per_sample = N. */
int ug_moe_dispatch_modulate(const void* x, int64_t ldx, const void* add, const void* mod, int64_t mod_estride, int64_t mod_bstride,
                             const int32_t* token_of_slot, int32_t E, int64_t capacity, int64_t tokens_per_sample,
                             int64_t D, void* out, ug_stream_t stream);

/* Combine (replaces einsum("sec,ecm->sm") src/UniGenUtils.py:183) fused with the CoMoE residual sums
 * (UniGenTransformer.py:1024,1089):
 *   eh = bf16(bf16(p) * yh[e][slot]) (0 if dropped), ec likewise from yc;
 *   out = bf16( bf16(xs + eh) + bf16(cs + ec) )    when xs/cs given (shared experts),
 *   out = bf16( eh + ec )                          otherwise.
 * If `accumulate` != 0, out = bf16(out_prev + that)  (MultiCondtionUniGenFlux sum over conditions, :1316).
 * Token s of xs / cs sits at physical row rowmap(s; s_rpb, s_bstride) (file header: "row map"; 0, 0 = identity): the shared experts'
 * image and condition streams are the two halves of one [B][2N][D] buffer, so all B samples combine in one launch. */
int ug_moe_combine(const void* yh, const void* yc, const float* gates, const int32_t* idx, const int32_t* slot,
                   int32_t E, int64_t capacity, const void* xs, const void* cs, int64_t ld_s, int64_t s_rpb, int64_t s_bstride,
                   void* out, int64_t ldo, int64_t S, int64_t D, int32_t accumulate, ug_stream_t stream);

/* FluxPipeline._pack_latents / _unpack_latents (diffusers; called at src/UniGenPipeline.py:641 and :796):
 *   packed[b][(i, j)][c*4 + dy*2 + dx] = latents[b][c][2i + dy][2j + dx],   latents [B][C][H][W], packed [B][(H/2)(W/2)][4C], contiguous. */
int ug_pack_latents(const void* latents, void* packed, int64_t B, int64_t C, int64_t H, int64_t W, ug_stream_t stream);
int ug_unpack_latents(const void* packed, void* latents, int64_t B, int64_t C, int64_t H, int64_t W, ug_stream_t stream);

/* ---- AutoencoderKL (the VAE either side of the hot path; reference src/UniGenPipeline.py:635-636 vae.encode of the
 * condition image, :797-798 vae.decode of the latents; diffusers 0.32.2 Encoder / Decoder / ResnetBlock2D / Upsample2D / Downsample2D /
 * Attention). Activations are NHWC [B][H][W][C]; 1x1 convolutions and the attention projections are ug_gemm_bf16 on [B H W][C]. ---- */

typedef struct ug_conv_desc {
    /* out[b][oy][ox][n] = R[..] + bf16( bias[n] + sum_{ky,kx,c} x[b][(oy*stride + ky - pad_t) >> up][(ox*stride + kx - pad_l) >> up][c] * w[n][ky][kx][c] ),
     * taps whose (virtual) coordinate falls outside [0, H << up) x [0, W << up) contribute zero. up = 1 folds Upsample2D's nearest-2x
     * interpolation into the gather; Downsample2D(padding=0)'s F.pad(x, (0, 1, 0, 1)) + stride-2 conv is pad_t = pad_l = 0, stride = 2. */
    const void* x; int64_t B, H, W, Cin;        /* NHWC input; Cin a multiple of 64 (zero-pad the channels) */
    const void* w;                              /* [Cout][KH][KW][Cin] (torch's [Cout][Cin][KH][KW] permuted once at load time) */
    const void* bias;                           /* [Cout] or NULL */
    const void* R;                              /* residual, NHWC [B][Ho][Wo][Cout] or NULL (may alias out) */
    void* out; int64_t Ho, Wo, Cout;            /* Cout a multiple of 4 */
    int32_t KH, KW, stride, pad_t, pad_l, up;
    const void* zero_page;                      /* >= 128 bytes of zeros, 16-byte aligned (device): what padding taps read */
    int64_t zero_page_bytes;                    /* size of zero_page (0 is read as 128). With >= 2 * (Cin + 64) bytes, Cin / 64 a power of two >= 2 and Cout,
                                                 * B Ho Wo multiples of 256, the convolution runs on the 256^2 GEMM kernel (its A operand gathered per tap) */
} ug_conv_desc;

/* torch F.conv2d (called by diffusers Conv2d layers of the VAE) as an implicit GEMM on MFMA. */
int ug_conv2d_nhwc(const ug_conv_desc* d, ug_stream_t stream);

/* out = [SiLU](GroupNorm(x; G groups, eps, gamma, beta)), x / out NHWC [B][HW][C] (F.group_norm + F.silu in ResnetBlock2D / Attention.group_norm /
 * conv_norm_out). Deterministic two-pass statistics in fp64 (per-thread sums over 64 rows: fp32 in the bf16 kernels, where they are exact for
 * bf16 inputs of one magnitude; fp64 in the fp32 twin, which holds rel-L2 1e-5 up to a group mean of 64 standard deviations and returns beta
 * exactly on a constant sample); workspace >= ug_groupnorm_workspace_bytes(B, HW, G), 8-byte aligned, no init needed.
 * UG_ERR_UNSUPPORTED unless C % 8 == 0 and C / G divides 256; UG_ERR_BAD_SHAPE unless G divides C. */
int64_t ug_groupnorm_workspace_bytes(int64_t B, int64_t HW, int32_t G);
int ug_groupnorm_nhwc(const void* x, const void* gamma, const void* beta, void* out, void* workspace, int64_t workspace_bytes,
                      int64_t B, int64_t HW, int64_t C, int32_t G, float eps, int32_t silu, ug_stream_t stream);

/* P[r][c] = softmax_c(scale * S[r][c]), S fp32 (ug_gemm_bf16 with UG_EPI_F32), P bf16: the VAE mid-block attention has one head of dim C
 * (F.scaled_dot_product_attention in AttnProcessor2_0), run as scores GEMM -> this -> P.V GEMM. Rows may be views (ld_s, ld_p >= cols); any
 * sign of scale. The fp32 twin takes scale s - max in fp64, so a common offset of the scores does not reach the probabilities. */
int ug_softmax_rows(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int64_t cols, float scale, ug_stream_t stream);

/* Layout changes at the VAE boundary: NCHW [B][C][HW] <-> NHWC [B][HW][Cp], Cp >= C (extra channels zero / ignored). div != 0 applies the
 * decode side's latent un-scaling on the way in: v -> bf16(bf16(v / div) + add)  (latents / scaling_factor + shift_factor, :797). */
int ug_nchw_to_nhwc(const void* in, void* out, int64_t B, int64_t C, int64_t HW, int64_t Cp, float div, float add, ug_stream_t stream);
int ug_nhwc_to_nchw(const void* in, void* out, int64_t B, int64_t C, int64_t HW, int64_t Cp, ug_stream_t stream);

/* z = ((mean + exp(0.5 clamp(logvar, -30, 20)) * noise) - shift) * scale: DiagonalGaussianDistribution.sample() and the latent scaling of
 * :635-636. moments NHWC [B][HW][Cp] (mean = channels [0, L), logvar = [L, 2L)); noise, z NCHW [B][L][HW]. */
int ug_vae_sample(const void* moments, int64_t Cp, const void* noise, void* z, int64_t B, int64_t L, int64_t HW, float shift, float scale,
                  ug_stream_t stream);

/* One tile of AutoencoderKL.tiled_decode / tiled_encode as the blend kernel sees it: logical element (b, c, y, x) of a [B][C][H][W] tile
 * lives at p + b * sb + c * sc + y * sy + x * sx (strides in ELEMENTS, any layout: NHWC rows [B*H*W][Cp] are sb = H W Cp, sc = 1, sy = W Cp,
 * sx = Cp; NCHW is sb = C H W, sc = H W, sy = W, sx = 1). p == NULL: there is no such neighbour (first row / first column of tiles). */
typedef struct ug_vae_tile {
    const void* p;
    int64_t H, W;
    int64_t sb, sc, sy, sx;
} ug_vae_tile;

typedef struct ug_vae_blend_desc {
    ug_vae_tile T, U, Lf, UL;            /* the tile, its upper, left and upper-left neighbours, all RAW (as the decoder / encoder wrote them) */
    void* out;                           /* canvas element that receives T(0, 0): out + b * ob + c * oc + y * oy + x * ox */
    int64_t ob, oc, oy, ox;
    int64_t B, C;
    int64_t h, w;                        /* the region written: rows [0, h) x columns [0, w) of the tile (diffusers' [:row_limit, :row_limit] crop) */
    int64_t E;                           /* blend extent in rows / columns (>= 0; 0 = plain copy of the crop) */
} ug_vae_blend_desc;

/* diffusers AutoencoderKL.tiled_decode / tiled_encode after the per-tile decoder / encoder: blend_v with the upper tile, blend_h with the left
 * tile, crop, and the two torch.cat calls, as ONE pass per tile that writes every element of the tile's canvas region exactly once.
 * The reference blends in place in row-major tile order, so a tile's neighbours are already blended when it reads them; because a blend only
 * touches a tile's first E rows / columns, that order collapses to a closed form over the four RAW tiles (needs U.H >= e_v + E and
 * Lf.W >= e_h + E, i.e. a full tile of at least 2 E: tile_overlap_factor <= 0.5; UG_ERR_UNSUPPORTED otherwise). With
 * e_v = U ? min(U.H, T.H, E) : 0, e_h = Lf ? min(Lf.W, T.W, E) : 0 and lerp(a, b, k, e) = rnd(rnd(a * f32(1 - k / e)) + rnd(b * f32(k / e)))
 * (k / e and 1 - k / e in double, rnd = round to the tensor dtype: torch's three roundings of `a * (1 - k / e) + b * (k / e)`):
 *     U'(r, x)  = x < e_h ? lerp(UL(r, UL.W - e_h + x), U(r, x), x, e_h) : U(r, x)
 *     Lf'(y, c) = y < e_v ? lerp(UL(UL.H - e_v + y, c), Lf(y, c), y, e_v) : Lf(y, c)
 *     t1        = y < e_v ? lerp(U'(U.H - e_v + y, x), T(y, x), y, e_v) : T(y, x)
 *     out(y, x) = x < e_h ? lerp(Lf'(y, Lf.W - e_h + x), t1, x, e_h) : t1            for y < h <= T.H, x < w <= T.W, every b < B, c < C.
 * Shapes: U.W == T.W, Lf.H == T.H, UL.H == U.H, UL.W == Lf.W; UL is required when both U and Lf are given (UG_ERR_BAD_SHAPE).
 * Aliasing: the region written must not overlap any of the four tiles; the tiles are only read and may overlap each other. No workspace, no
 * atomics, nothing kept between launches. Fast paths (16-byte loads and stores) when every tile given is channel-contiguous with pixels
 * of whole 8-channel groups (sc == 1, p 16-byte aligned, sb / sy / sx multiples of 8, sx >= C rounded up to 8: the channels up to that bound are
 * READ at every pixel of a tile, so they must exist, as they do in NHWC rows [B*H*W][Cp]) and the canvas is channel-contiguous in the same way (the encoder's NHWC moments) or x-contiguous (ox == 1:
 * the decoder's NCHW image, written straight from the NHWC conv_out rows); rows that are not 16-byte aligned, ragged row ends and
 * C % 8 channels go through scalar accesses. Any other stride combination runs element by element. */
int ug_vae_tile_blend(const ug_vae_blend_desc* d, ug_stream_t stream);

/* ---- fp32 verification twins (see the conventions at the top). Same arguments as the functions they mirror; every `void*` tensor
 * that is bf16 there is fp32 here (weights included); fp32 / integer arguments are unchanged. ug_gemm_f32: K, N unconstrained,
 * the column-split boundaries multiples of 64, no workspace. ug_small_linear_f32: M <= 64. ---- */
int ug_gemm_f32(const ug_gemm_desc* d, ug_stream_t stream);
int ug_small_linear_f32(const void* x, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                        const void* R, int64_t ldr, void* out, int64_t ldo,
                        int64_t M, int64_t N, int64_t K, int32_t act_in, ug_stream_t stream);
int ug_adaln_modulate_f32(const void* x, int64_t ldx, int64_t x_rpb, int64_t x_bstride,
                          const void* shift, const void* scale, int64_t mod_ld, int64_t rows_per_sample,
                          void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream);
int ug_qk_rmsnorm_rope_f32(void* buf, int64_t ld, int64_t batches, int64_t rows_per_batch, int64_t batch_stride_rows,
                           int64_t pos_offset, int64_t q_off, int64_t k_off, int32_t heads, int32_t dh,
                           const void* wq_a, const void* wk_a, const void* wq_b, const void* wk_b, int64_t split,
                           const float* cos_tab, const float* sin_tab, float eps, ug_stream_t stream);
int ug_flash_attn_fwd_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                          const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                          const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                          void* o, int64_t o_row_stride, int64_t o_batch_stride,
                          int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                          float softmax_scale, ug_stream_t stream);
/* fp32 twin of ug_flash_attn_fwd_wide (dh = 512 only): plain FMA loops, exact online softmax ("Strided attention views") */
int ug_flash_attn_fwd_wide_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                               const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                               const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                               void* o, int64_t o_row_stride, int64_t o_batch_stride,
                               int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                               float softmax_scale, ug_stream_t stream);
int ug_timestep_embed_f32(const float* t, void* out, int64_t ldo, int64_t B, int32_t dim, ug_stream_t stream);
int ug_euler_step_f32(void* x, const void* v, float dt, int64_t n, ug_stream_t stream);
int ug_cfg_combine_f32(const void* uncond, const void* text, float guidance_scale, void* out, int64_t n, ug_stream_t stream);
int ug_dpm_step_f32(const void* pred_uncond, const void* pred_text, float guidance_scale, float* sample, float* x0_prev, void* model_in, int32_t copies,
                    int32_t order, float sigma, float a, float b, float rinv, int64_t n, ug_stream_t stream);
int ug_add_f32(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo,
               int64_t rows, int64_t D, ug_stream_t stream);
int ug_add_rowbcast_f32_f32(void* x, int64_t ldx, const float* table, int64_t ldt, int64_t rows, int64_t rows_per_batch, int64_t D,
                            ug_stream_t stream);
int ug_gather_rows_f32(const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W,
                       ug_stream_t stream);
int ug_moe_gate_top1_f32(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E,
                         float* gates, int32_t* idx, ug_stream_t stream);
int ug_moe_gate_top2_f32(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E, const float* noise,
                         float* gates, int32_t* idx, ug_stream_t stream);
int ug_moe_gate_topk_f32(const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E, int32_t K, float* gates,
                         float* logits, int32_t* idx, ug_stream_t stream);
int ug_moe_combine_topk_f32(const void* yh, const void* yc, const float* weights, const int32_t* idx, const int32_t* slot, int32_t K,
                            int64_t kstride, int32_t E, int64_t capacity, const void* xs, const void* cs, int64_t ld_s, int64_t s_rpb,
                            int64_t s_bstride, void* out, int64_t ldo, int64_t S, int64_t D, int32_t accumulate, ug_stream_t stream);
int ug_moe_dispatch_modulate_f32(const void* x, int64_t ldx, const void* add, const void* mod, int64_t mod_estride, int64_t mod_bstride,
                                 const int32_t* token_of_slot, int32_t E, int64_t capacity, int64_t tokens_per_sample,
                                 int64_t D, void* out, ug_stream_t stream);
int ug_moe_combine_f32(const void* yh, const void* yc, const float* gates, const int32_t* idx, const int32_t* slot,
                       int32_t E, int64_t capacity, const void* xs, const void* cs, int64_t ld_s, int64_t s_rpb, int64_t s_bstride,
                       void* out, int64_t ldo, int64_t S, int64_t D, int32_t accumulate, ug_stream_t stream);
int ug_conv2d_nhwc_f32(const ug_conv_desc* d, ug_stream_t stream);      /* any Cin / Cout, no zero_page */
int ug_groupnorm_nhwc_f32(const void* x, const void* gamma, const void* beta, void* out, void* workspace, int64_t workspace_bytes,
                          int64_t B, int64_t HW, int64_t C, int32_t G, float eps, int32_t silu, ug_stream_t stream);
int ug_softmax_rows_f32(const float* S, int64_t ld_s, void* P, int64_t ld_p, int64_t rows, int64_t cols, float scale, ug_stream_t stream);
int ug_nchw_to_nhwc_f32(const void* in, void* out, int64_t B, int64_t C, int64_t HW, int64_t Cp, float div, float add, ug_stream_t stream);
int ug_nhwc_to_nchw_f32(const void* in, void* out, int64_t B, int64_t C, int64_t HW, int64_t Cp, ug_stream_t stream);
int ug_vae_sample_f32(const void* moments, int64_t Cp, const void* noise, void* z, int64_t B, int64_t L, int64_t HW, float shift, float scale,
                      ug_stream_t stream);
int ug_vae_tile_blend_f32(const ug_vae_blend_desc* d, ug_stream_t stream);
int ug_pack_latents_f32(const void* latents, void* packed, int64_t B, int64_t C, int64_t H, int64_t W, ug_stream_t stream);
int ug_unpack_latents_f32(const void* packed, void* latents, int64_t B, int64_t C, int64_t H, int64_t W, ug_stream_t stream);

/* Diagnostic, not on the hot path: one launch of a bare bf16 MFMA loop (operands in registers, one wave per SIMD, pseudo-random
 * operand values) on `blocks` workgroups of 256 threads; shape 0 = v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_16x16x32_bf16. The caller
 * times it (HIP events) to get the measured MFMA peak that bench.py reports as `roofline.peak_measured`.
 * scratch: blocks * 256 floats (device). *flops_out_host (HOST pointer, may be NULL) receives the FLOPs of the launch. */
int ug_probe_mfma_bf16(int32_t shape, int64_t blocks, int64_t iters, void* scratch, double* flops_out_host, ug_stream_t stream);

/* ---- Backward pass of the control-module training step (reference train.py:622-662 `accelerator.backward(loss)` over the same
 * forward). The matrix work of the backward is ug_gemm_bf16 again (dX = dY W through a transposed copy of W, dW = dY^T X through transposed copies
 * of dY and X, the attention backward as grouped GEMMs per sample); these entry points are what sits between those GEMMs. Each replaces the
 * autograd formula of the torch op named; each has an `_f32` twin like the forward entry points. ---- */
/* dst[b][c][r] = src[b][r][c] for r < rows, c < cols; dst[b][c][rows .. rows_pad) = 0. (Tensor.t().contiguous() of an operand) */
int ug_transpose(const void* src, int64_t ld_src, int64_t src_bstride, void* dst, int64_t ld_dst, int64_t dst_bstride, int64_t batch, int64_t rows,
                 int64_t cols, int64_t rows_pad, ug_stream_t stream);
/* out[g][c] = alpha * sum over the rows r of group g (rows_per_group consecutive rows) of a[r][c] * (b ? b[r][c] : 1), fp32 accumulation.
 * (grad of a bias / a per-sample gate, shift, scale: `.sum(dim)` in the backward of a broadcast) */
int ug_colsum(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int64_t cols, int64_t rows_per_group,
              float alpha, void* workspace, int64_t workspace_bytes, ug_stream_t stream);
/* bytes of the caller-owned fp32 scratch of ug_colsum (per-chunk partial sums, added in a fixed order: run-to-run reproducible) */
int64_t ug_colsum_workspace_bytes(int64_t rows, int64_t cols, int64_t rows_per_group);
/* y[r] = (x ? x[r] : 0) + gate[r / rows_per_sample] * a[r], the product rounded first: `x + gate.unsqueeze(1) * a` of every transformer block
 * (FluxTransformerBlock / FluxSingleTransformerBlock, called at src/UniGenTransformer.py:1129,1151) as one op of the training forward; with x = NULL
 * its backward d a = gate * d y (d x = d y; d gate = ug_colsum(d y, a) per sample). */
int ug_gate_residual(const void* x, int64_t ldx, const void* a, int64_t lda, const void* gate, int64_t gate_ld, int64_t rows_per_sample, void* y,
                     int64_t ldy, int64_t rows, int64_t D, ug_stream_t stream);
int ug_gate_residual_f32(const void* x, int64_t ldx, const void* a, int64_t lda, const void* gate, int64_t gate_ld, int64_t rows_per_sample, void* y,
                         int64_t ldy, int64_t rows, int64_t D, ug_stream_t stream);
/* backward of ug_moe_gate_top1 (deepspeed TopKGate / top1gating gate softmax, src/UniGenUtils.py:99; reference: torch autograd through
 * F.linear(x.float(), wg.float()) + softmax, train.py:654): d gates [S, E] fp32 -> dx [S, D] = d(x + c) (the gradient of BOTH x and c) and
 * dwg_partials fp32 [ug_moe_gate_bwd_slices(S)][E][D], whose sum over the first axis (fixed order: reproducible) is d wg. E <= 16. */
int ug_moe_gate_bwd(const float* gates, const float* dgates, const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E,
                    void* dx, int64_t lddx, float* dwg_partials, ug_stream_t stream);
int ug_moe_gate_bwd_f32(const float* gates, const float* dgates, const void* x, const void* c, int64_t ld, const void* wg, int64_t S, int64_t D, int32_t E,
                        void* dx, int64_t lddx, float* dwg_partials, ug_stream_t stream);
int64_t ug_moe_gate_bwd_slices(int64_t S);
/* y = gelu_tanh(x); dx = dy * gelu_tanh'(x)   (F.gelu(approximate="tanh") of FeedForward net.0 / proj_mlp and its backward) */
int ug_gelu_tanh(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_gelu_tanh_bwd(const void* x, const void* dy, void* dx, int64_t n, ug_stream_t stream);
/* backward of ug_adaln_modulate (LayerNorm(x) * (1 + scale) + shift): dx, and partials: fp32 [samples][P][2][D], P =
 * ug_adaln_modulate_bwd_partials(rows, rows_per_sample): partial column sums over disjoint row sets of each sample of dy ([..][0][D], whose sum
 * over P is d shift) and of dy * xhat ([..][1][D]: d scale); the caller adds them. scale: [samples][mod_ld] as in the forward. D <= 4096, D % 8 == 0. */
int64_t ug_adaln_modulate_bwd_partials(int64_t rows, int64_t rows_per_sample);
int ug_adaln_modulate_bwd(const void* x, int64_t ldx, const void* dy, int64_t lddy, const void* scale, int64_t mod_ld, int64_t rows_per_sample,
                          void* dx, int64_t lddx, void* partials, int64_t rows, int64_t D, float eps, ug_stream_t stream);
/* backward of ug_qk_rmsnorm_rope for ONE of q / k: x = the projection's output (pre-norm) [rows][heads * dh] at ldx, dy = gradient of the
 * normalised + rotated heads; dx likewise; dw_partial: fp32 [ug_qk_rmsnorm_rope_bwd_partials(rows, heads)][dh], partial sums of d(un) * xhat
 * over disjoint sets of (row, head) vectors - their sum over the first index, taken by the caller, is d weight (deterministic: the assignment of
 * vectors to partial rows depends only on rows and heads). w NULL: no RMSNorm, dw_partial unused; cos NULL: no RoPE. dh <= 256.
 * Row r sits at position pos_offset + r % rows_per_batch; cos / sin tables [positions][dh] fp32 as in the forward. */
int64_t ug_qk_rmsnorm_rope_bwd_partials(int64_t rows, int32_t heads);
int ug_qk_rmsnorm_rope_bwd(const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw_partial, const void* w,
                           const float* cos_tab, const float* sin_tab, int64_t rows, int64_t rows_per_batch, int64_t pos_offset, int32_t heads,
                           int32_t dh, float eps, ug_stream_t stream);
/* attention backward between its GEMMs (F.scaled_dot_product_attention, src/UniGenUtils.py:601): lse[r] = logsumexp(scale * S[r][:]);
 * P = exp(scale * S - lse) for the first valid_cols columns, 0 for the rest (zero-padded keys: sequence lengths are padded to the GEMM's
 * contraction granularity); delta[g][r] = sum_c dO[r][g*cols + c] * O[r][g*cols + c]; dS = scale * P * (dP - delta). S, dP fp32. */
int ug_row_lse(const float* S, int64_t ld, float* lse, int64_t rows, int64_t cols, float scale, ug_stream_t stream);
int ug_attn_prob(const float* S, int64_t ld_s, const float* lse, void* P, int64_t ld_p, int64_t rows, int64_t cols, int64_t valid_cols, float scale,
                 ug_stream_t stream);
int ug_attn_dscore(const void* P, int64_t ld_p, const float* dP, int64_t ld_dp, const float* delta, void* dS, int64_t ld_ds, int64_t rows, int64_t cols,
                   float scale, ug_stream_t stream);
int ug_rowdot(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int64_t groups, int64_t cols, ug_stream_t stream);
/* F.scaled_dot_product_attention backward on the forward kernel's tiling (bf16): dq, dk, dv from q, k, v, o, dout in the forward's [batch][row][head*dh]
 * strided layout. Four launches of one kernel (row statistics lse, then dQ, dK, dV, each recomputing its score tiles; csrc/attention.hip) plus
 * delta = rowsum(dout * o). workspace: ug_flash_attn_bwd_workspace_bytes() bytes, 16-byte aligned (lse and delta, fp32 per (batch, head, query)).
 * The fp32 verification path keeps the GEMM-based formulation of unigen_amd/autograd.py. */
int64_t ug_flash_attn_bwd_workspace_bytes(int64_t batches, int32_t heads, int64_t Lq);
/* ug_flash_attn_fwd that also writes lse2[b][h][q] = log2 sum_k 2^(scale log2(e) s_qk) (fp32, row length lse_ld >= Lq, typically Lq rounded up to 64
 * with the padding zeroed by the caller): the forward of a training step; hand the buffer to ug_flash_attn_bwd as lse_in. The padding must be
 * there (the backward loads whole 64-row tiles of statistics), but no kernel multiplies by it - a query row >= Lq is selected to 0 - so its values
 * reach no result (tests/test_workspace_gpu.py fills it with NaN). */
int ug_flash_attn_fwd_lse(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                          const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                          int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale, float* lse2, int64_t lse_ld,
                          ug_stream_t stream);
int ug_flash_attn_bwd(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                      const void* v, int64_t v_row_stride, int64_t v_batch_stride, const void* o, int64_t o_row_stride, int64_t o_batch_stride,
                      const void* dout, int64_t do_row_stride, int64_t do_batch_stride, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride,
                      void* dk, int64_t dk_row_stride, int64_t dk_batch_stride, void* dv, int64_t dv_row_stride, int64_t dv_batch_stride,
                      int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                      const float* lse_in /* [batches][heads][Lq rounded up to 64], or NULL: recomputed */, void* workspace, int64_t workspace_bytes,
                      ug_stream_t stream);
/* ---- Backward of the LoRA adapters (csrc/lora_bwd.hip; reference: torch autograd through the PEFT LoraLayer of train.py's
 * `transformer_lora_parameters`). With y = x W^T + b + (x A_cat^T) B_bd^T and T = x A_cat^T, the adapter gradients are products with one skinny
 * side R (the padded rank) that contract over the M rows: dA_cat = dT^T X, dB_bd^T = T^T dY.
 * C[r][j] = alpha * sum_m P[m][r] * Q[m][j]: P [M, R] and Q [M, J] row-major (leading dimensions ldp, ldq: multiples of 8, bases 16-byte aligned),
 * fp32 accumulation, alpha applied in fp32 before the one rounding; C [R, J] with leading dimension ldc. R = 64, 128, 192 or 256; J a multiple of 64;
 * any M > 0 (the last partial block of rows is zero-filled on chip). The rows are split across workgroups; the splits' fp32 partial results go
 * through the caller-owned workspace and are added in a fixed order (no atomics: results are bit-identical run to run).
 * dB_bd itself is the transpose of the result for P = T, Q = dY: callers view it. ---- */
int ug_lora_wgrad_bf16(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int64_t M, int64_t R, int64_t J, float alpha,
                       void* workspace, int64_t workspace_bytes, ug_stream_t stream);
int ug_lora_wgrad_f32(const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc, int64_t M, int64_t R, int64_t J, float alpha,
                      void* workspace, int64_t workspace_bytes, ug_stream_t stream);
/* bytes of the fp32 scratch of ug_lora_wgrad_* for this shape (splits x R x J floats; 16-byte aligned). An upper bound for both twins: the bf16
 * entry point stores straight from the tile when the shape makes one split and then ignores the workspace. */
int64_t ug_lora_wgrad_workspace_bytes(int64_t M, int64_t R, int64_t J);
int ug_transpose_f32(const void* src, int64_t ld_src, int64_t src_bstride, void* dst, int64_t ld_dst, int64_t dst_bstride, int64_t batch, int64_t rows,
                     int64_t cols, int64_t rows_pad, ug_stream_t stream);
int ug_colsum_f32(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int64_t cols, int64_t rows_per_group,
                  float alpha, void* workspace, int64_t workspace_bytes, ug_stream_t stream);
int ug_gelu_tanh_f32(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_gelu_tanh_bwd_f32(const void* x, const void* dy, void* dx, int64_t n, ug_stream_t stream);
int ug_adaln_modulate_bwd_f32(const void* x, int64_t ldx, const void* dy, int64_t lddy, const void* scale, int64_t mod_ld, int64_t rows_per_sample,
                              void* dx, int64_t lddx, void* partials, int64_t rows, int64_t D, float eps, ug_stream_t stream);
int ug_qk_rmsnorm_rope_bwd_f32(const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw_partial, const void* w,
                               const float* cos_tab, const float* sin_tab, int64_t rows, int64_t rows_per_batch, int64_t pos_offset, int32_t heads,
                               int32_t dh, float eps, ug_stream_t stream);
int ug_attn_prob_f32(const float* S, int64_t ld_s, const float* lse, void* P, int64_t ld_p, int64_t rows, int64_t cols, int64_t valid_cols, float scale,
                     ug_stream_t stream);
int ug_attn_dscore_f32(const void* P, int64_t ld_p, const float* dP, int64_t ld_dp, const float* delta, void* dS, int64_t ld_ds, int64_t rows,
                       int64_t cols, float scale, ug_stream_t stream);
int ug_rowdot_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int64_t groups, int64_t cols, ug_stream_t stream);

/* ---- optimizer step of the training loop (csrc/optim.hip): accelerator.clip_grad_norm_(transformer.parameters(), max_grad_norm)
 * (train.py:658) and torch.optim.AdamW.step() (train.py:660) over every trainable tensor in one launch each. The work list is a DEVICE table
 * of ug_optim_tensor descriptors and a DEVICE list of int32 (tensor index, chunk index) pairs, chunk c of tensor t covering elements
 * [c * UG_OPTIM_CHUNK, min((c + 1) * UG_OPTIM_CHUNK, numel)); every element of every tensor in exactly one pair. Any element alignment is
 * accepted (16-byte vector accesses on the aligned body of a chunk, scalar head and tail). No atomics: results are bitwise reproducible. ---- */
enum { UG_DT_BF16 = 0, UG_DT_F32 = 1 };
#define UG_OPTIM_CHUNK 65536
#define UG_ADAMW_MAX_GROUPS 32

typedef struct ug_optim_tensor {
    void* param;           /* bf16 or fp32 (param_dtype); unused by ug_grad_sumsq / ug_grad_scale */
    void* grad;            /* bf16 or fp32 (grad_dtype); written only by ug_grad_scale */
    float* master;         /* fp32 master weights of a bf16 param; NULL for an fp32 param (updated in place) */
    float* exp_avg;        /* fp32 first / second moments */
    float* exp_avg_sq;
    int64_t numel;
    int32_t param_dtype;   /* UG_DT_* */
    int32_t grad_dtype;
    int32_t group;         /* index into the ug_adamw_group array of ug_adamw_step */
    int32_t _pad;
} ug_optim_tensor;

/* hyperparameters of one param group at this step, each computed by the caller in fp64 (as torch's Python does) and rounded to fp32 once */
typedef struct ug_adamw_group {
    float decay;             /* 1 - lr * weight_decay */
    float lerp_w;            /* 1 - beta1 */
    float beta2;
    float one_minus_beta2;   /* 1 - beta2 */
    float eps;
    float step_size;         /* lr / (1 - beta1^step) */
    float inv_bc2_sqrt;      /* 1 / fp32(sqrt(1 - beta2^step)) in fp32: torch divides a tensor by a Python scalar as a product with its reciprocal */
    float _pad;
} ug_adamw_group;

/* host-side check of a HOST copy of the table before it is uploaded: numel >= 0, known dtypes, non-null grads; with n_groups > 0 (an AdamW table)
 * also group < n_groups, non-null param / moments, a master exactly for bf16 params. n_groups == 0: a gradient-only table. */
int ug_optim_check_table(const ug_optim_tensor* table_host, int32_t n_tensors, int32_t n_groups);
/* bytes of the fp64 per-chunk partials of ug_grad_sumsq */
int64_t ug_grad_sumsq_workspace_bytes(int64_t n_chunks);
/* total_norm = ||all grads||_2 (fp32 per lane and wave, fp64 across the chunk and in the fixed-order sum of the chunks, a second one-block launch);
 * norm_coef[0] = total_norm, norm_coef[1] = min(1, max_norm / (total_norm + 1e-6)) with torch's arithmetic (torch/nn/utils/clip_grad.py:
 * inf -> 0, NaN propagates). Both fp32 in device memory. */
int ug_grad_sumsq(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, float max_norm, float* norm_coef,
                  void* workspace, int64_t workspace_bytes, ug_stream_t stream);
/* grad = grad * (*coef) in place, rounded once to the grad's dtype (torch._foreach_mul_ of clip_grad_norm_ with the 0-dim fp32 clip_coef) */
int ug_grad_scale(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, const float* coef, ug_stream_t stream);
/* torch.optim.AdamW (decoupled weight decay; torch.optim.adam._single_tensor_adam's order of operations) on every chunk, fp32 arithmetic:
 *   g = grad * (coef ? *coef : 1); p = p * decay; m = lerp(m, g, lerp_w); v = v * beta2 + one_minus_beta2 * g * g;
 *   p = p - step_size * (m / (sqrt(v) * inv_bc2_sqrt + eps))      (IEEE sqrt and division)
 * p is the master (bf16 param: the param is then written as RNE(p)) or the fp32 param itself. Grads are only read. groups_host: n_groups <=
 * UG_ADAMW_MAX_GROUPS entries, passed by value with the launch. */
int ug_adamw_step(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, const ug_adamw_group* groups_host,
                  int32_t n_groups, const float* coef, ug_stream_t stream);

/* ---- AdamW without fp32 masters and / or with bf16 moments: what is kept in bf16 is written with STOCHASTIC rounding, so that an update far
 * below a bf16 ulp still moves the value in expectation. The arithmetic before the rounding is ug_adamw_step's, operation for operation.
 *
 * Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", Random123), counter-based and stateless.
 *   key     = { seed & 0xffffffff, seed >> 32 }
 *   counter = { j & 0xffffffff, j >> 32, param_index, step }   with j = element_index >> 1
 * element_index is the element's index inside its TENSOR (not inside a chunk), param_index the parameter's ordinal in the optimizer (the id of
 * torch's Optimizer.state_dict), step the parameter's step count after this step's increment (first step: 1). The four output words serve the
 * two elements 2j and 2j + 1: element i takes the 16 bits at shift 16 * (i & 1) of word 0 for the parameter, of word 1 for exp_avg, of word 2
 * for exp_avg_sq; word 3 is unused. A draw depends on (seed, param_index, step, element_index, word) and on nothing else: not on chunking,
 * alignment, the vector or scalar path, or what else is in the launch.
 *
 * Rounding of an fp32 value with bits u and a draw r in [0, 65536): finite values give bf16 bits (u + r) >> 16 - symmetric about zero
 * (sign-magnitude), a value on the bf16 grid never moves, a value goes to the neighbour away from zero with probability (u & 0xffff) / 65536
 * exactly, the top half-ulp below the largest finite value can reach Inf (as round-to-nearest does); Inf stays Inf; NaN becomes the quiet NaN
 * (u >> 16) | 0x0040. ---- */
typedef struct ug_optim_tensor_lp {
    void* param;           /* bf16 or fp32 (param_dtype) */
    void* grad;            /* bf16 or fp32 (grad_dtype); only read */
    float* master;         /* fp32 master of a bf16 param, or NULL: the bf16 param itself is then read, updated and rounded stochastically */
    void* exp_avg;         /* first / second moments, bf16 or fp32 (state_dtype) */
    void* exp_avg_sq;
    int64_t numel;
    int32_t param_dtype;   /* UG_DT_* */
    int32_t grad_dtype;
    int32_t state_dtype;
    int32_t group;         /* index into the ug_adamw_group_lp array */
    uint32_t param_index;  /* counter word 2 of this tensor's draws */
    int32_t _pad;
} ug_optim_tensor_lp;

/* ug_adamw_group's hyperparameters, plus what the draws of the group's tensors need */
typedef struct ug_adamw_group_lp {
    float decay;
    float lerp_w;
    float beta2;
    float one_minus_beta2;
    float eps;
    float step_size;
    float inv_bc2_sqrt;
    uint32_t step;           /* the step count after this step's increment, >= 1: counter word 3 */
    uint64_t seed;           /* the Philox key */
} ug_adamw_group_lp;

/* host-side check of a HOST copy of the table: as ug_optim_check_table for an AdamW table (n_groups >= 1), with the arrangements of this entry point.
 * bf16 param: (master NULL, bf16 state) p, m, v read as bf16, each written with its own draw; (master NULL, fp32 state) only p is drawn for;
 * (master, bf16 state) the master stays fp32 and p is its RNE, m and v are drawn for; (master, fp32 state) and every fp32 param (no master, fp32
 * state): ug_adamw_step's path, no draws. */
int ug_optim_check_table_lowp(const ug_optim_tensor_lp* table_host, int32_t n_tensors, int32_t n_groups);
/* ug_adamw_step on a table of ug_optim_tensor_lp: same chunk list, same fused clip coefficient, no atomics, no workspace. */
int ug_adamw_step_lowp(const ug_optim_tensor_lp* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks,
                       const ug_adamw_group_lp* groups_host, int32_t n_groups, const float* coef, ug_stream_t stream);
/* out[i] (bf16) = the stochastic rounding of x[i] with the draw of element_index first_index + i, word in {0, 1, 2}. Any element alignment:
 * 16-byte accesses on the body where x and out are 16-byte aligned at a common element, scalar head and tail. */
int ug_sr_round_bf16(const float* x, void* out, int64_t n, int64_t first_index, uint64_t seed, uint32_t param_index, uint32_t step, int32_t word,
                     ug_stream_t stream);

/* ---- flow-matching training objective (csrc/objective.hip; reference train.py:589-613 noisy model input, :644-652 loss). Contiguous tensors;
 * `void*` tensors are bf16 (fp32 in the `_f32` twins), `float*` ones fp32 in both. 16-byte accesses where the base pointers are 16-byte aligned,
 * scalar accesses otherwise and on a sample's unaligned head and tail. No atomics: results are bitwise reproducible. ---- */
enum { UG_FLOW_NONE = 0, UG_FLOW_SIGMA_SQRT = 1, UG_FLOW_COSMAP = 2, UG_FLOW_LOGIT_NORMAL = 3, UG_FLOW_MODE = 4 };   /* args.weighting_scheme */

/* x, noise [B][C][H][W]; u [B] uniform draws in [0, 1); sigma_table [T] (the scheduler's training sigmas, device memory). Per sample
 *   idx = min((int)(u * T), T - 1)  (clamped: the reference indexes out of range when u * T rounds up to T), s32 = sigma_table[idx],
 *   timestep = (s32 * T) / 1000  (two fp32 operations: scheduler.timesteps, then :630), sigma = bf16(s32) (s32 in the twin),
 *   weight (fp32, from that sigma) = 1 | sigma^-2 (UG_FLOW_SIGMA_SQRT) | 2 / (pi (1 - 2 sigma + 2 sigma^2)) (UG_FLOW_COSMAP);
 * per element
 *   noisy = bf16(bf16(bf16(1 - sigma) * x) + bf16(sigma * noise))   (no intermediate rounding in the twin),   target = bf16(noise - x).
 * pack = 1 writes noisy and target in FluxPipeline._pack_latents layout [B][(H/2)(W/2)][4C] (H, W even), pack = 0 in [B][C][H][W]. */
int ug_flow_noise(const void* x, const void* noise, const float* u, const float* sigma_table, int64_t T, int32_t scheme, int32_t pack, int64_t B,
                  int64_t C, int64_t H, int64_t W, void* noisy, void* target, float* sigma, float* timestep, float* weight, ug_stream_t stream);
int ug_flow_noise_f32(const void* x, const void* noise, const float* u, const float* sigma_table, int64_t T, int32_t scheme, int32_t pack, int64_t B,
                      int64_t C, int64_t H, int64_t W, void* noisy, void* target, float* sigma, float* timestep, float* weight, ug_stream_t stream);
/* pred, target [B][n], weight [B] -> loss_per_sample[b] = mean_i(weight[b] * (pred - target)^2), loss[0] = mean_b of those; fp32 accumulation in
 * both forms. Two launches: per-block partial sums into the caller-owned fp32 workspace, then one block that adds them in a fixed order. */
int64_t ug_flow_loss_workspace_bytes(int64_t B, int64_t n);
int ug_flow_loss(const void* pred, const void* target, const float* weight, int64_t B, int64_t n, float* loss_per_sample, float* loss,
                 void* workspace, int64_t workspace_bytes, ug_stream_t stream);
int ug_flow_loss_f32(const void* pred, const void* target, const float* weight, int64_t B, int64_t n, float* loss_per_sample, float* loss,
                     void* workspace, int64_t workspace_bytes, ug_stream_t stream);
/* grad[b][i] = gout[0] * 2 weight[b] (pred - target) / (n B) in pred's dtype, one rounding; gout: autograd's upstream gradient of loss[0], a DEVICE
 * fp32 scalar. fp32 order of operations: (((gout * 1/B) * 1/n) * weight[b]) * (2 (pred - target)), which is torch autograd's through the eager lines. */
int ug_flow_loss_bwd(const void* pred, const void* target, const float* weight, const float* gout, int64_t B, int64_t n, void* grad, ug_stream_t stream);
int ug_flow_loss_bwd_f32(const void* pred, const void* target, const float* weight, const float* gout, int64_t B, int64_t n, void* grad,
                         ug_stream_t stream);

/* ---- text encoders (csrc/text.hip; unigen_amd/text.py: T5EncoderModel, CLIPTextModel - the reference runs transformers' modules at train.py:381-395,
 * :523-569 and at the top of every pipeline call through src/text_encoder.py). Their matrix work is ug_gemm_bf16, the embedding ug_gather_rows. ---- */
/* ug_flash_attn_fwd with, before the softmax, an additive bias of the relative position and / or a causal mask:
 *   s_qk = softmax_scale * q.k + (rel_table ? rel_table[h][(k - q) + rel_len - 1] : 0);   causal != 0: keys k > q get probability 0.
 * rel_table: fp32 [heads][2 * rel_len - 1] (ug_t5_rel_table), rel_len >= max(Lq, Lkv) and <= 4096: a head's slice is loaded into LDS once per
 * workgroup; no [heads][Lq][Lkv] tensor exists anywhere. T5 passes softmax_scale = 1 (T5Attention does not scale), CLIP dh^-0.5 with causal = 1 and no
 * table. dh = 64 with a table or a mask; with neither the call IS ug_flash_attn_fwd (same kernel, same bits). */
int ug_flash_attn_fwd_bias(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                           const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                           const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                           void* o, int64_t o_row_stride, int64_t o_batch_stride,
                           int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                           float softmax_scale, const float* rel_table, int64_t rel_len, int32_t causal, ug_stream_t stream);
int ug_flash_attn_fwd_bias_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                               const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                               const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                               void* o, int64_t o_row_stride, int64_t o_batch_stride,
                               int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                               float softmax_scale, const float* rel_table, int64_t rel_len, int32_t causal, ug_stream_t stream);
/* table[h][j] = weight[bucket(j - (L - 1))][h] for j in [0, 2L - 1): T5Attention.compute_bias as a function of k - q alone. weight: block 0's
 * relative_attention_bias.weight [num_buckets][heads] (bf16; fp32 in the twin), table fp32 in both. bucket(): T5's bidirectional rule - the upper half of
 * the buckets for k > q; within a half, distances n < max_exact = num_buckets / 4 have their own bucket, larger ones
 * min(max_exact + (int)(log(n / max_exact) / log(max_distance / max_exact) * (num_buckets / 2 - max_exact)), num_buckets / 2 - 1), in fp32. */
int ug_t5_rel_table(const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table, ug_stream_t stream);
int ug_t5_rel_table_f32(const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table, ug_stream_t stream);
/* T5LayerNorm: out = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))), statistics in fp32, no mean subtraction, the module's two rounding points (none in the
 * twin). Rows of any width D that is a multiple of 8, 16-byte aligned; one pass over the row up to D = 4608. */
int ug_rmsnorm_rows(const void* x, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream);
int ug_rmsnorm_rows_f32(const void* x, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream);
/* nn.LayerNorm with weight and bias: out = bf16((x - mean) * rsqrt(var + eps) * w + b), var = mean((x - mean)^2), fp32 arithmetic, one rounding. */
int ug_layernorm_rows(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
                      ug_stream_t stream);
int ug_layernorm_rows_f32(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
                          ug_stream_t stream);
/* out[m][n] = bf16( bf16(gelu_new(ab[m][n])) * ab[m][F + n] ), n < F: T5DenseGatedActDense between wi_0 | wi_1 (one GEMM over the stacked weight writes
 * ab [M][2F]) and wo. gelu_new(x) = 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))). F a multiple of 8. */
int ug_gated_gelu(const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream);
int ug_gated_gelu_f32(const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream);
/* y = x * sigmoid(1.702 x): CLIP-L's hidden_act "quick_gelu". n contiguous elements, a multiple of 8; y may alias x. */
int ug_quick_gelu(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_quick_gelu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);
/* y = 0.5 x (1 + erf(x / sqrt 2)): the exact GELU, hidden_act "gelu" (OpenCLIP bigG, SD3's second CLIP). Evaluated in fp32, the bf16 entry rounds once
 * at the store. Same contract as ug_quick_gelu: n contiguous elements, a multiple of 8; y may alias x. */
int ug_gelu_erf(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_gelu_erf_f32(const void* x, void* y, int64_t n, ug_stream_t stream);

/* ---- image front end (csrc/image.hip; unigen_amd/image.py: VaeImageProcessor, canny; unigen_amd/condition.py - the reference builds its canny
 * condition with cv2.Canny(img, 100, 200) in src/condition.py:63-67 and sends every image through diffusers' VaeImageProcessor). Integer or exactly
 * specified fp32 arithmetic: one right answer per element. Images are uint8 NHWC [B, H, W, C]; `bstride` / `rstride` are the BYTE distances between
 * samples and between rows, the pixels of a row are contiguous. B, H < 65536. No alignment is required; aligned bases and strides take the wide paths.
 * No fp32 twins: nothing here rounds. ---- */
/* Stage 1 of Canny: 3x3 Sobel in x and y with replicated borders and the L1 magnitude |dx| + |dy|, contiguous [B, H, W] each. C is 1 or 3; with 3
 * channels the channel with the largest magnitude supplies all three values, the first one on a tie. */
int ug_canny_grad(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int16_t* dx, int16_t* dy,
                  int32_t* mag, ug_stream_t stream);
/* Stage 2: non-maximum suppression and the double threshold of cv::Canny with L2gradient = false (fixed-point tangent test, TG22 = 13573; magnitudes
 * outside the image are 0). map [B, H, W]: 2 = strong (mag > high), 0 = candidate (kept, mag > low), 1 = not an edge. low > high swaps the two. */
int ug_canny_nms(const int16_t* dx, const int16_t* dy, const int32_t* mag, int64_t B, int64_t H, int64_t W, int32_t low, int32_t high, uint8_t* map,
                 ug_stream_t stream);
/* Stage 3: every candidate that is 8-connected to a strong pixel through candidates becomes strong (in place, in `map`); out = 255 there, else 0.
 * Runs as sweeps of one launch each - a workgroup takes its tile to a local fixed point, no workgroup waits on another - and reads the 4-byte device
 * word `flag` after each sweep (a stream synchronisation per sweep: this stage sits outside the denoise loop and cannot be graph-captured). *sweeps_host
 * (may be NULL) receives their number, at most the value returned by the bound function below, H * W + 1. */
int ug_canny_hysteresis(uint8_t* map, int64_t B, int64_t H, int64_t W, uint8_t* out, int64_t out_bstride, int64_t out_rstride, int32_t* flag,
                        int32_t* sweeps_host, ug_stream_t stream);
int64_t ug_canny_max_sweeps(int64_t H, int64_t W);
/* The three stages in one call on a caller-owned, 16-byte aligned workspace of the size the query returns. */
int64_t ug_canny_workspace_bytes(int64_t B, int64_t H, int64_t W);
int ug_canny_u8(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t low, int32_t high, uint8_t* out,
                int64_t out_bstride, int64_t out_rstride, void* workspace, int64_t workspace_bytes, int32_t* sweeps_host, ug_stream_t stream);
/* PIL's Image.resize for 8-bit images (ImagingResample, 8bpc): horizontal pass, then vertical pass, a uint8 image between them; a pass whose size does
 * not change is skipped and needs no tables. Per output coordinate o of a pass: bounds[2 o] = first input coordinate, bounds[2 o + 1] = taps n <= k,
 * coef[o * k + i] = 22-bit fixed-point weights (device tables, built on the host: unigen_amd/image.py resample_tables). A value is
 * clip((2^21 + sum_i in[first + i] * coef[i]) >> 22, 0, 255). tmp: [B, Hin, Wout, C] bytes, needed when both sizes change. C is 1 or 3. */
int ug_img_resize_u8(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t Hin, int64_t Win, int32_t C, uint8_t* dst,
                     int64_t dst_bstride, int64_t dst_rstride, int64_t Hout, int64_t Wout, const int32_t* xbounds, const int32_t* xcoef, int32_t xk,
                     const int32_t* ybounds, const int32_t* ycoef, int32_t yk, uint8_t* tmp, ug_stream_t stream);
/* PIL's convert("L") of an RGB image: (19595 R + 38470 G + 7471 B + 0x8000) >> 16, [B, H, W, 3] -> [B, H, W, 1]. */
int ug_img_rgb_to_l(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, uint8_t* dst, int64_t dst_bstride,
                    int64_t dst_rstride, ug_stream_t stream);
/* uint8 NHWC -> contiguous NCHW [B, Cout, H, W] of dst_dtype (UG_DT_F32 or UG_DT_BF16): v / 255.0f (IEEE division), then 2.0f * . - 1.0f when
 * `normalize`, every operation rounded in fp32; bf16 is that value rounded to nearest-even. C is 1 or 3; Cout = C, or 3 with C = 1 (gray replicated). */
int ug_img_u8_to_chw(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, int32_t C, void* dst, int32_t dst_dtype,
                     int32_t Cout, int32_t normalize, ug_stream_t stream);
/* Contiguous NCHW [B, C, H, W] of src_dtype -> uint8 NHWC with the rounding points of diffusers' denormalize + numpy_to_pil: x * 0.5 + 0.5 in the
 * input's dtype (skipped with denormalize = 0: a processor built with do_normalize = False), clamp to [0, 1], to fp32, * 255.0f, round half to even.
 * C from 1 to 4. */
int ug_img_chw_to_u8(const void* src, int32_t src_dtype, int64_t B, int32_t C, int64_t H, int64_t W, uint8_t* dst, int64_t dst_bstride, int64_t dst_rstride,
                     int32_t denormalize, ug_stream_t stream);
/* PIL's BoxBlur / GaussianBlur of 8-bit images (BoxBlur.c): `passes` passes along rows with (rx, wwx, fwx), then `passes` along columns with
 * (ry, wwy, fwy), uint8 after every pass. One pass along a line of `size` pixels, per channel, in uint32:
 *   out[x] = (ww * sum_{i=-r..r} in[clamp(x+i)] + fw * (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + 2^23) >> 24,  clamp(p) = min(max(p, 0), size - 1).
 * The constants come from the host (unigen_amd/image.py box_blur_constants, gaussian_box_radius): 0 <= r < 2^24, weights >= 0 with
 * (2 r + 1) ww + 2 fw <= 2^24. (0, 2^24, 0), the constants of radius 0, skips the axis as PIL does; both axes skipped is a copy. BoxBlur(R) is
 * passes = 1, GaussianBlur(radius) is passes = 3 with the box radius of _gaussian_blur_radius. C is 1 or 3; dst must not alias src.
 * fuse = 1: an axis whose halo of passes * (r + 1) pixels fits in LDS (up to 128 along rows, 48 along columns) runs all its passes in ONE launch;
 * fuse = 0, or a larger halo: one launch per pass, any radius (r + 1 >= size included). The launches alternate between the two images of the
 * caller-owned, 16-byte aligned workspace of the size the query returns. */
int64_t ug_img_blur_workspace_bytes(int64_t B, int64_t H, int64_t W, int32_t C);
int ug_img_box_blur_u8(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, int32_t C, uint8_t* dst,
                       int64_t dst_bstride, int64_t dst_rstride, int32_t rx, int32_t wwx, int32_t fwx, int32_t ry, int32_t wwy, int32_t fwy, int32_t passes,
                       int32_t fuse, void* workspace, int64_t workspace_bytes, ug_stream_t stream);

/* ---- depth condition (csrc/depth.hip; unigen_amd/depth.py: transformers' DepthAnythingForDepthEstimation, DPTImageProcessor and the
 * depth-estimation pipeline's post-processing - the reference builds its depth condition with them in src/condition.py:52-62). The glue that is
 * neither a GEMM nor a convolution; activations are NHWC. Every bf16 entry has an `_f32` twin (fp32 storage, no intermediate rounding) declared
 * beside it. Outputs are fully written, pad channels included; 16-byte aligned bases take the 8-channel paths, anything else single elements. ---- */
/* uint8 NHWC [B, H, W, C] (byte strides as for the image front end; C = 3, or 1: gray replicated) -> rows [B (H/P) (W/P)][ld_out] of the
 * patch-embedding GEMM: column c P^2 + ky P + kx (the flattening of the conv weight [D][3][P][P]) of the row of patch (py, px) is
 *   ((float)((double)v * rescale) - mean_host[c]) / std_host[c]          v = img[b][py P + ky][px P + kx][c]
 * with DPTImageProcessor's rounding points (rescale: a float64 product cast to float32; normalize: float32 subtraction and IEEE division);
 * columns [3 P^2, Kp) are zero. Kp a multiple of 64; H, W multiples of P <= 64. mean_host, std_host: 3 floats each. bf16 rounds once, at the store. */
int ug_img_u8_to_patches(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t P, double rescale,
                         const float* mean_host, const float* std_host, void* out, int64_t ld_out, int64_t Kp, ug_stream_t stream);
int ug_img_u8_to_patches_f32(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t P, double rescale,
                             const float* mean_host, const float* std_host, void* out, int64_t ld_out, int64_t Kp, ug_stream_t stream);
/* y = x < 0 ? +0 : x over n contiguous elements, n a multiple of 8; y may be x. torch.relu's values bit for bit: a NaN propagates (it is not
 * laundered into 0, which would hide an upstream fault), -0 stays -0, +-inf give +0 / +inf. The head's fused ReLU (ug_depth_head_out) is a
 * different contract: it feeds a dot product and is specified on finite inputs. */
int ug_relu(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_relu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);
/* Second half of nn.ConvTranspose2d(C, C, kernel = stride = f): `prod` is the fp32 product (UG_EPI_F32) of the input rows [B h w][Cin] with the
 * weight re-laid as [(ky, kx, co)][Cin], rows of f f Cout floats with leading dimension ld_prod.
 *   out[b][y f + ky][x f + kx][co] = rnd(prod[(b, y, x)][(ky f + kx) Cout + co] + bias[co]),  zeros in channels [Cout, Cp)
 * out NHWC [B][h f][w f][Cp], Cp a multiple of 8: accumulate, add the bias, round once, as the module does in bf16. */
int ug_deconv_scatter_nhwc(const float* prod, int64_t ld_prod, const void* bias, void* out, int64_t B, int64_t h, int64_t w, int32_t f, int64_t Cout,
                           int64_t Cp, ug_stream_t stream);
int ug_deconv_scatter_nhwc_f32(const float* prod, int64_t ld_prod, const void* bias, void* out, int64_t B, int64_t h, int64_t w, int32_t f, int64_t Cout,
                               int64_t Cp, ug_stream_t stream);
/* F.interpolate(mode="bilinear", align_corners) of NHWC [B][H][W][C] to [B][Ho][Wo][C], C a multiple of 8, any Ho, Wo >= 1. Source index and
 * weights in fp32 as torch's area_pixel_compute_source_index: align_corners: scale = (in - 1) / (out - 1) (0 when out == 1), src = o scale;
 * otherwise scale = in / out, src = max(0, (o + 0.5) scale - 0.5), the upper index clamped. One rounding, at the store. */
int ug_bilinear_nhwc(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* out, int64_t Ho, int64_t Wo, int32_t align_corners,
                     ug_stream_t stream);
int ug_bilinear_nhwc_f32(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* out, int64_t Ho, int64_t Wo, int32_t align_corners,
                         ug_stream_t stream);
/* DepthAnythingDepthEstimationHead's activation1 + conv3 (1x1 to one channel) + activation2 + max_depth on x [pixels][Cp] (channels [0, C) used):
 *   out[p] = act(rnd(bias[0] + sum_c w[c] relu(x[p][c]))) * max_depth,  act = ReLU, or sigmoid with metric != 0
 * out fp32 [pixels]; w [C], bias [1] in the activation dtype. The bf16 entry rounds conv3's output, the sigmoid and the product to bf16. */
int ug_depth_head_out(const void* x, int64_t pixels, int64_t C, int64_t Cp, const void* w, const void* bias, float max_depth, int32_t metric, float* out,
                      ug_stream_t stream);
int ug_depth_head_out_f32(const void* x, int64_t pixels, int64_t C, int64_t Cp, const void* w, const void* bias, float max_depth, int32_t metric,
                          float* out, ug_stream_t stream);
/* F.interpolate(mode="bicubic", align_corners=False) of fp32 [B][H][W] to [B][Ho][Wo] (the pipeline's post_process_depth_estimation): A = -0.75, the
 * four taps per axis index-clamped as upsample_bicubic2d does. fp32 only. B, Ho < 65536. */
int ug_bicubic_f32(const float* x, int64_t B, int64_t H, int64_t W, float* out, int64_t Ho, int64_t Wo, ug_stream_t stream);
/* The pipeline's depth image: per image of d fp32 [B][HW], uint8(trunc(((d - min) / (max - min)) * 255.0f)) with numpy's float32 order of operations,
 * written to uint8 [B][HW][channels], channels 1 or 3 (replicated). One right answer per element. max == min writes 0 (numpy yields NaN there and
 * its cast is unspecified). Min and max are reduced in two deterministic stages, no float atomics; the caller-owned, 8-byte aligned workspace of the
 * size the query returns needs no initialisation. B < 65536. */
int64_t ug_minmax_workspace_bytes(int64_t B, int64_t HW);
int ug_minmax_to_u8(const float* d, int64_t B, int64_t HW, uint8_t* out, int32_t channels, void* workspace, int64_t workspace_bytes, ug_stream_t stream);

/* ---- Sana transformer block (csrc/sana.hip; unigen_amd/sana.py: diffusers' SanaTransformerBlock). The two kernel classes of that block which are
 * neither a GEMM nor a softmax attention. Every bf16 entry has an `_f32` twin (fp32 storage, no intermediate rounding) declared beside it. ---- */
/* SanaLinearAttnProcessor2_0: ReLU linear attention without a softmax. Head h occupies columns [h dh, (h + 1) dh) of each row, as in ug_flash_attn_fwd;
 * with q' = relu(q), k' = relu(k), per (batch, head):
 *   S[d][j] = sum_n v[n][d] k'[n][j]     z[j] = sum_n k'[n][j]     out[n][d] = sum_j S[d][j] q'[n][j] / (sum_j z[j] q'[n][j] + 1e-15)
 * q, k, v are upcast, everything is fp32 (S and z included: they are never rounded to bf16), the output is rounded once. dh must be 32
 * (UG_ERR_UNSUPPORTED otherwise); any N >= 1. q / k / v / o are views ("Strided attention views"; the packed [q | k | v] output of one GEMM is
 * read in place). The caller-owned, 16-byte aligned
 * workspace of the size the query returns needs no initialisation: the per-chunk partial states are written, then summed in ascending chunk order, then
 * applied - three launches, no atomics, nothing kept between calls, so two calls give the same bits and the call can be captured in a graph.
 * GUARANTEE for the backward: on return the first batches * heads * 1056 floats of the workspace hold the state, per (batch, head) S^T[j][d]
 * (1024 floats) then z[j] (32): this is the `state` operand of ug_linear_attn_bwd. */
int64_t ug_linear_attn_workspace_bytes(int64_t batches, int64_t heads, int64_t N);
int ug_linear_attn(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                   const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                   int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace, ug_stream_t stream);
int ug_linear_attn_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                       const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                       int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace, ug_stream_t stream);
/* The middle of GLUMBConv (norm_type None, no residual) between the conv_inverted and conv_point GEMMs. x NHWC [B][H][W] rows of 2C with row stride ldx:
 * conv_inverted's output BEFORE its SiLU. w9: conv_depth.weight [2C][1][3][3] repacked as [9][2C] (tap ky 3 + kx major), bias [2C].
 *   a = rnd(silu(x))     y = rnd(dwconv3x3(a, zero padding 1) + bias)  (fp32 accumulate)     out[..][c] = rnd(y[..][c] * rnd(silu(y[..][C + c])))
 * out [B][H][W] rows of C with row stride ldo; columns [C, ldo) are written as zeros (the K padding of the conv_point GEMM). C must be a multiple
 * of 8 (UG_ERR_UNSUPPORTED otherwise); ldx, ldo multiples of 8 elements and every base 16-byte aligned (UG_ERR_BAD_ALIGN). */
int ug_glu_dwconv3x3(const void* x, int64_t ldx, const void* w9, const void* bias, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t C,
                     ug_stream_t stream);
int ug_glu_dwconv3x3_f32(const void* x, int64_t ldx, const void* w9, const void* bias, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t C,
                         ug_stream_t stream);
/* Backward of ug_linear_attn (csrc/sana_bwd.hip). q, k, v as in the forward; dout [batch][N][heads * 32] the gradient of its output; state: the
 * batches * heads * 1056 floats (S^T[j][d] | z[j]) that ug_linear_attn leaves at the start of its workspace - REQUIRED (NULL: UG_ERR_BAD_SHAPE), there
 * is no recompute path, and the forward's rounded output is not an input: o = S q' / den is recomputed in fp32. With g = dout / den,
 * c = -(dout . o) / den:  dq' = g S + c z,  dS = g^T q',  dz = c^T q',  dk' = v dS + dz,  dv = k' dS^T,  dq = dq' [q > 0],  dk = dk' [k > 0].
 * dS and dz stay fp32; dq, dk, dv are rounded once, at the store; each takes a row and a batch stride (the three may be the column blocks of one
 * [M][3 D] buffer: the dY of the fused QKV projection). Views ("Strided attention views") and limits as in the forward; dh = 32 only, any
 * N >= 1. The caller-owned, 16-byte aligned workspace of ug_linear_attn_bwd_workspace_bytes() needs no initialisation (smaller: UG_ERR_BAD_SHAPE): the
 * query pass writes dq and one partial dS | dz per 128 query rows, the partials are summed in ascending order, the key pass writes dk and dv - three
 * launches, no atomics, nothing kept between calls: two calls give the same bits, and the call can be captured in a graph. */
int64_t ug_linear_attn_bwd_workspace_bytes(int64_t batches, int64_t heads, int64_t N);
int ug_linear_attn_bwd(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                       const void* v, int64_t v_row_stride, int64_t v_batch_stride, const void* dout, int64_t do_row_stride, int64_t do_batch_stride,
                       const float* state, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride, void* dk, int64_t dk_row_stride, int64_t dk_batch_stride,
                       void* dv, int64_t dv_row_stride, int64_t dv_batch_stride, int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace,
                       int64_t workspace_bytes, ug_stream_t stream);
int ug_linear_attn_bwd_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                           const void* v, int64_t v_row_stride, int64_t v_batch_stride, const void* dout, int64_t do_row_stride, int64_t do_batch_stride,
                           const float* state, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride, void* dk, int64_t dk_row_stride, int64_t dk_batch_stride,
                           void* dv, int64_t dv_row_stride, int64_t dv_batch_stride, int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace,
                           int64_t workspace_bytes, ug_stream_t stream);
/* Backward of ug_glu_dwconv3x3 (csrc/sana_bwd.hip). x, w9, bias: what the forward read; dout [B][H][W] rows of C with row stride lddo (its pad columns
 * are not read); dx rows of 2C with row stride lddx (columns past 2C are not written). a = rnd(silu(x)), y = rnd(dwconv(a) + bias) and
 * s = rnd(silu(y_gate)) are recomputed as the forward rounds them; the gradient is that of the function as evaluated (roundings straight-through):
 *   dy_val = rnd(dout s)   dy_gate = rnd(dout y_val silu'(y_gate))   da[p] = sum_t w9[t] dy[p - t]   dx = rnd(da silu'(x))
 *   dw9[t][c] = sum_p dy[p][c] a[p + t][c]   dbias[c] = sum_p dy[p][c]
 * fp32 accumulation throughout; dy is rounded once (it passes through the workspace), dx once. dw9 [9][2C] and dbias [2C] leave as fully reduced
 * fp32 (partials per 256 pixels, added in ascending order, no atomics); both may be NULL (frozen convolution weights: no reduction is launched), one
 * alone is UG_ERR_BAD_SHAPE. C a multiple of 8; ldx, lddo, lddx multiples of 8 elements, every base 16-byte aligned. workspace: caller-owned, 16-byte
 * aligned, ug_glu_dwconv3x3_bwd_workspace_bytes(B, H, W, C, elem_bytes) bytes with elem_bytes 2 (bf16) or 4 (the fp32 twin), no initialisation
 * needed (smaller: UG_ERR_BAD_SHAPE). Two calls give the same bits; the call can be captured in a graph. */
int64_t ug_glu_dwconv3x3_bwd_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int32_t elem_bytes);
int ug_glu_dwconv3x3_bwd(const void* x, int64_t ldx, const void* w9, const void* bias, const void* dout, int64_t lddo, void* dx, int64_t lddx, float* dw9,
                         float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, void* workspace, int64_t workspace_bytes, ug_stream_t stream);
int ug_glu_dwconv3x3_bwd_f32(const void* x, int64_t ldx, const void* w9, const void* bias, const void* dout, int64_t lddo, void* dx, int64_t lddx, float* dw9,
                             float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, void* workspace, int64_t workspace_bytes, ug_stream_t stream);

/* ---- Gemma-2 text encoder (csrc/text.hip, whose attention and row-norm templates it shares with T5 and CLIP; the gather: csrc/elementwise.hip;
 * unigen_amd/gemma.py: transformers' Gemma2Model, the prompt encoder of Sana). Its matrix work is ug_gemm_bf16, its gated activation
 * ug_gated_gelu (gelu_pytorch_tanh is gelu_new). Every bf16 entry has an `_f32` twin declared beside it. ---- */
/* Causal self-attention with grouped K/V heads, logit soft-capping, a sliding window and a key length per sample (transformers'
 * eager_attention_forward under Gemma-2's causal / sliding masks and a right-padded attention_mask). Query head h occupies columns [h dh, (h + 1) dh)
 * of a q / o row and reads K/V head h / (heads / kv_heads), at columns [that * dh, ..) of a k / v row; Lq = Lkv = L.
 *   s_qk = softcap ? softcap * tanh(softmax_scale * q.k / softcap) : softmax_scale * q.k
 *   key k gets probability 0 when k > q, or window && k <= q - window, or kv_len && k >= kv_len[b].
 * kv_len: device int32 [batches] or NULL; kv_len[b] >= 1 is the caller's contract (values above L count as L). A row without a live key - a padded
 * row further than `window` behind kv_len[b], nothing else - is written as zeros (the module's additive mask spreads such a row over all keys).
 * Views as in "Strided attention views": q, k, v 8 / 16, o 4 / 8 (the twin: all 4 / 16), no row-stride bound. Order of refusals: nothing to do
 * (batches or L zero: UG_OK), null operands, non-positive counts, heads % kv_heads != 0, a negative softcap or window (UG_ERR_BAD_SHAPE), then
 * dh != 256 and L >= 2^30 (UG_ERR_UNSUPPORTED), then the views. bf16 in / out, fp32 accumulation, online softmax, P rounded to bf16 as the P.V operand; the
 * bf16 entry evaluates tanh through exp2 and a reciprocal, the twin with tanhf. No workspace, no atomics, no state: two launches give the same
 * bits and the launch can be captured in a graph (36.5 KiB of static LDS; one workgroup = 128 query rows of one head). */
int ug_flash_attn_fwd_softcap(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                              const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                              const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                              void* o, int64_t o_row_stride, int64_t o_batch_stride,
                              int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh,
                              float softmax_scale, float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream);
int ug_flash_attn_fwd_softcap_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride,
                                  const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                                  const void* v, int64_t v_row_stride, int64_t v_batch_stride,
                                  void* o, int64_t o_row_stride, int64_t o_batch_stride,
                                  int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh,
                                  float softmax_scale, float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream);
/* apply_rotary_pos_emb of modeling_gemma2.py (rotate_half), in place on `nheads` consecutive dh-wide heads from column col0 of buf [rows][ld]: the
 * q and k heads of a packed q | k | v projection (nheads = heads + kv_heads; the v columns are not touched). Row r has position r % rows_per_batch.
 * cos_tab, sin_tab: [>= rows_per_batch][dh / 2] in the storage dtype (the module casts cos / sin to the activations' dtype), for i < dh / 2:
 *   y[i] = bf16(bf16(x[i] cos[i]) - bf16(x[i + dh/2] sin[i]))     y[i + dh/2] = bf16(bf16(x[i + dh/2] cos[i]) + bf16(x[i] sin[i]))
 * (three rounding points, none in the twin). dh must be 256 (UG_ERR_UNSUPPORTED); ld, col0 multiples of 8 (4) elements, bases 16-byte aligned. */
int ug_rope_half(void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh, const void* cos_tab,
                 const void* sin_tab, ug_stream_t stream);
int ug_rope_half_f32(void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh, const void* cos_tab,
                     const void* sin_tab, ug_stream_t stream);
/* Gemma2RMSNorm with an optional residual: y = bf16((x * rsqrt(mean(x^2) + eps)) * (1 + w)), statistics and both products in fp32, ONE rounding
 * (ug_rmsnorm_rows is T5's: weight w, two roundings); out = residual ? bf16(residual + y) : y, the layer's `residual + hidden_states` (no rounding at
 * all in the twin). residual: rows at ldr, or NULL (ldr ignored); out may be x or the residual itself. D a multiple of 8 (UG_ERR_UNSUPPORTED otherwise), rows
 * 16-byte aligned; one pass over the row up to D = 4608. */
int ug_gemma_rmsnorm_rows(const void* x, int64_t ldx, const void* w, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows, int64_t D,
                          float eps, ug_stream_t stream);
int ug_gemma_rmsnorm_rows_f32(const void* x, int64_t ldx, const void* w, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows, int64_t D,
                              float eps, ug_stream_t stream);
/* ug_gather_rows with a multiplier: out[i][:W] = bf16(src[idx[i]][:W] * scale) (zeros when idx[i] < 0). Gemma2TextScaledWordEmbedding: the caller passes
 * hidden_size ** 0.5 already rounded to the storage dtype, as the module does. */
int ug_gather_rows_scaled(const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W, float scale,
                          ug_stream_t stream);
int ug_gather_rows_scaled_f32(const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W, float scale,
                              ug_stream_t stream);

/* ---- DC-AE (csrc/dcae.hip; unigen_amd/dcae.py: diffusers' AutoencoderDC, the 32x autoencoder of Sana). Its convolutions are ug_conv2d_nhwc, its 1x1
 * convolutions and linears ug_gemm_bf16, its attention ug_linear_attn, the middle of its GLUMBConv ug_glu_dwconv3x3. Below are the remaining passes over
 * NHWC activations: rows with an explicit row stride in elements. Every bf16 entry has an `_f32` twin (fp32 storage, no intermediate rounding)
 * declared beside it. No workspace, no atomics, no state: two calls give the same bits and each call can be captured in a graph. Zero-sized calls
 * return UG_OK without a launch. ---- */
/* diffusers' RMSNorm(C, eps, elementwise_affine = True, bias = True) over the channel row, fused with what follows it in DC-AE:
 *   y = rnd((x * rsqrt(mean(x^2) + eps)) * w + b)      fp32 statistics and arithmetic, ONE rounding
 *   out = residual ? rnd(y + residual) : act == 1 ? relu(y) : y
 * (the residual of ResBlock, GLUMBConv and the attention; the decoder's norm_out + ReLU). residual: rows at ldr, or NULL (ldr ignored); a residual
 * together with act = 1 is UG_ERR_UNSUPPORTED. x, residual and out may be one another. C a multiple of 8, at most 4608 (UG_ERR_UNSUPPORTED): the row
 * is read once, with 16-byte accesses, and kept in registers. ldx, ldo, ldr multiples of 8 (twin: 4) elements, every base 16-byte aligned. */
int ug_rmsnorm_bias_rows(const void* x, int64_t ldx, const void* w, const void* bias, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows,
                         int64_t C, float eps, int32_t act, ug_stream_t stream);
int ug_rmsnorm_bias_rows_f32(const void* x, int64_t ldx, const void* w, const void* bias, const void* residual, int64_t ldr, void* out, int64_t ldo,
                             int64_t rows, int64_t C, float eps, int32_t act, ug_stream_t stream);
/* SanaMultiscaleAttentionProjection, one scale: a depthwise k x k convolution (zero padding k / 2, no bias), then a grouped 1x1 convolution with G
 * groups of 32 channels in and 32 out (no bias). x NHWC [B][H][W] rows of G * 32 channels with row stride ldx; w_dw: proj_in.weight [G*32][1][k][k]
 * repacked as [k*k][G*32] (tap ky k + kx major); w_pw: proj_out.weight [G*32][32][1][1], that is [G][32 out][32 in] as stored.
 *   a = rnd(dwconv(x))  (fp32 accumulate)      out[..][g*32 + o] = rnd(sum_i a[..][g*32 + i] * w_pw[g][o][i])  (fp32 accumulate, on the matrix cores)
 * out rows have row stride ldo; columns from G * 32 on are not written. `a` never goes to memory. k = 5 (every published configuration) and k = 3
 * are built, any other k is UG_ERR_UNSUPPORTED. ldx, ldo multiples of 8 elements and every base 16-byte aligned (UG_ERR_BAD_ALIGN). */
int ug_msconv_proj(const void* x, int64_t ldx, const void* w_dw, const void* w_pw, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t G,
                   int32_t k, ug_stream_t stream);
int ug_msconv_proj_f32(const void* x, int64_t ldx, const void* w_dw, const void* w_pw, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t G,
                       int32_t k, ug_stream_t stream);
/* The non-parametric shortcuts of DCDownBlock2d / DCUpBlock2d, of the encoder's out_shortcut and the decoder's in_shortcut, with the add. h NHWC
 * [B][H][W] rows of Cin channels (row stride ldh); factor f is 1 or 2 (UG_ERR_UNSUPPORTED otherwise).
 * down: out [B][H / f][W / f] rows of Cout.  u = pixel_unshuffle(h, f): u[c f^2 + dy f + dx] at (y, x) is h[c] at (f y + dy, f x + dx);
 *       y[n] = rnd(mean_{j < g} u[n g + j]), g = Cin f^2 / Cout, the sum in fp32 in ascending j.
 * up:   out [B][H f][W f] rows of Cout.      rep[m] = h[m / r], r = Cout f^2 / Cin;  y = pixel_shuffle(rep, f): y[c] at (f y + dy, f x + dx) is
 *       rep[c f^2 + dy f + dx] at (y, x).
 * out = x ? rnd(x + y) : y. x (row stride ldx), when x_shuffle = 0, has the layout of out and may be out itself. x_shuffle = 1: x is itself still to
 * be pixel-(un)shuffled - it has h's pixel grid [B][H][W] and Cout / f^2 (down) resp. Cout f^2 (up) channels (the "pixel_unshuffle" / "pixel_shuffle"
 * block types, whose convolution runs before the rearrangement). Without x and with g = 1 (down) resp. always (up) the call is a pure copy, bit for bit.
 * UG_ERR_BAD_SHAPE unless g resp. r is a positive integer and (down) H, W are multiples of f. Cin, Cout multiples of 8 (UG_ERR_UNSUPPORTED); ldh, ldx,
 * ldo multiples of 8 (twin: 4) elements, every base 16-byte aligned. */
int ug_dc_shortcut_down(const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                        int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream);
int ug_dc_shortcut_down_f32(const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                            int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream);
int ug_dc_shortcut_up(const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                      int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream);
int ug_dc_shortcut_up_f32(const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                          int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream);
/* y = rnd(silu(x)) over n contiguous elements (the activation between a ResBlock's two convolutions); y may be x. n a multiple of 8
 * (UG_ERR_UNSUPPORTED), both 16-byte aligned. The bf16 entry evaluates the sigmoid through exp2 and a reciprocal, the twin with expf and a division. */
int ug_silu(const void* x, void* y, int64_t n, ug_stream_t stream);
int ug_silu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);

int ug_version(void);
const char* ug_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UNIGEN_HIP_H */
