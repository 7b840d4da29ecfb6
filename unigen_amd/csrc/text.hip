// Kernels of the text encoders (T5 encoder, CLIP text model: unigen_amd/text.py; Gemma-2, the prompt encoder of Sana: unigen_amd/gemma.py). The
// matrix work of all three is ug_gemm_bf16 and the token embedding ug_gather_rows / ug_gather_rows_scaled; this file holds what sits between them:
//   ug_flash_attn_fwd_bias      attention at head width 64 with T5's additive relative-position bias (a per-head table of k - q, held in LDS)
//                               and / or CLIP's causal mask
//   ug_flash_attn_fwd_softcap   Gemma-2's causal attention at head width 256 with grouped K/V heads, logit soft-capping, a sliding window and a
//                               key length per sample
//   ug_t5_rel_table             the [heads][2L - 1] table of that bias from block 0's relative_attention_bias.weight
//   ug_rope_half                apply_rotary_pos_emb (rotate_half) in place on the q and k heads of the packed q | k | v projection (head width 256)
//   ug_rmsnorm_rows             T5LayerNorm;   ug_layernorm_rows   nn.LayerNorm with weight and bias
//   ug_gemma_rmsnorm_rows       Gemma2RMSNorm, weight 1 + w, one rounding, with the residual sum that follows two of the layer's four norms
//   ug_gated_gelu               gelu_new(a) * b over the two halves of the stacked [wi_0; wi_1] projection;   ug_quick_gelu   x sigmoid(1.702 x)
//   ug_gelu_erf                 0.5 x (1 + erf(x / sqrt 2)), the activation of SD3's second CLIP (OpenCLIP bigG)
// and the `_f32` verification twin of each (fp32 storage, no intermediate rounding); the attention twins run verify_f32.hip's one fp32 kernel.
//
// The attention kernel is deliberately plain next to attention.hip's: at T5-XXL (512 tokens, 64 heads) attention is about 2 % of the encoder's
// FLOPs. One template serves both widths. One workgroup = 4 waves = 128 query rows of one (batch, head), Q fragments in registers, K tiles of KT
// keys staged row-major ([KT][DH + 8] bf16) and V tiles TRANSPOSED into LDS through registers ([DH][KT + 8]; single buffer, two barriers per
// tile). The MFMA formulation is attention.hip's:
//   S^T = K Q^T    v_mfma_f32_32x32x16_bf16, the query index on the lane: scores, bias, cap and masks are lane-local, one exchange with lane ^ 32
//                  for the max;
//   O^T = V^T P^T  accumulator registers 8s .. 8s + 7 of S^T, packed to bf16, are the B operand of k-step s; the A operand reads the matching
//                  keys (16s + 4h + 0..3 and 16s + 8 + 4h + 0..3) of row d of the transposed V image as two 8-byte LDS reads.
// Scores never leave registers. At head width 64 (KT 64: 18 KiB of tiles) the bias is tab[(k - q) + rel_len - 1] from the head's table slice,
// loaded into LDS behind the tiles once per workgroup (pre-multiplied by log2 e: the softmax runs in base 2). At head width 256 the
// kernel runs one wave per SIMD (Q fragments 64 VGPRs, the O^T accumulator 128, S^T 16) on tiles of 32 keys (16.5 + 20 KiB). The soft cap is
// cap * tanh(x / cap) with tanh(y) = 1 - 2 / (e^2y + 1) through v_exp_f32 and v_rcp_f32 (exact limits -1 and 1 at e^2y = 0 and inf; absolute
// error a few 2^-24, which the cap multiplies: far below the bf16 rounding of P). A causal launch ends its key loop at the workgroup's last
// query row (or the sample's key length) and starts it at the window's first key of the workgroup's first row; a wave skips the tiles that lie
// wholly above its own 32 rows' diagonal or behind its window. A row none of whose keys is live (every row of a sample whose kv_len is 0, and
// with a window the padded rows from kv_len + window - 1 on) is written as zeros. K and V rows in [kv_len, L) are still read and enter the
// products with a probability of zero: they must be finite.
#include "pointwise.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int AQ = 128;            // query rows per workgroup
constexpr float LOG2E = 1.4426950408889634f;

// what the two entries hand the launcher beside the views; of the kernel's arguments BIAS reads rel_table / rel_len, RAGGED kv_len / group / window,
// CAP c1 (T5's and CLIP's come first in the kernel's list, at the offsets they always had)
struct attn_plain_args {
    const float* rel_table; int rel_len;
    const int32_t* kv_len; int group, window;
    float c0 /* CAP: 2 log2(e) softmax_scale / cap, else softmax_scale log2(e) */, c1 /* cap log2(e) */;
};

// BIAS: the table; CAUSAL: keys above the diagonal are masked; CAP: the soft cap; RAGGED: a sliding window (0 = none), a key length per sample
// (kv_len, or NULL) and `group` query heads per K/V head - the three things that can leave a row, or a wave's tile, without a live key.
template <int DH, int KT, bool BIAS, bool CAUSAL, bool CAP, bool RAGGED>
__global__ __launch_bounds__(256) void attn_plain_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    const float* __restrict__ rel_table, int rel_len, int heads, int Lq, int Lkv_, int nQ, float c0, float c1, const int32_t* __restrict__ kv_len, int group,
    int window) {
    static_assert(CAUSAL || !RAGGED, "the window and the key length are cut out of a causal mask");
    const int Lkv = RAGGED ? Lq : Lkv_;        // RAGGED is self-attention: one length, one register
    constexpr int KROW = DH + 8;       // bf16 elements per row of the K image (16-byte aligned rows that do not all start in one bank)
    constexpr int VROW = KT + 8;       // bf16 elements per row of the transposed V image
    constexpr int CPR = DH / 8;        // 16-byte chunks per key row
    // the launch's LDS: K, V^T, then the table (static tile arrays cost the dh-64 instantiations four registers: docs/KERNEL_NOTES.md, "Gemma-2 kernels")
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = (bf16_t*)smem;                // [KT keys][KROW]
    bf16_t* Vt = Ks + KT * KROW;               // [DH d][VROW]: Vt[d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qt = blockIdx.x % nQ, bh = blockIdx.x / nQ;
    const int head = bh % heads, b = bh / heads;
    const int kvh = RAGGED ? head / group : head;
    const int tab_n = 2 * rel_len - 1;
    float* tab = nullptr;                      // [2 rel_len - 1], times log2(e)
    if constexpr (BIAS) {
        tab = (float*)(Vt + DH * VROW);
        const float* src = rel_table + (int64_t)head * tab_n;
        for (int i = tid; i < tab_n; i += 256) tab[i] = src[i] * LOG2E;
    }
    int kvl = Lkv;                             // keys at kvl and beyond are padding
    if constexpr (RAGGED) kvl = kv_len ? min(max(kv_len[b], 0), Lkv) : Lkv;
    const int Q0 = qt * AQ;
    const int q0 = Q0 + wave * 32;             // the wave's first query row
    const int qrow = q0 + r;
    const int qcl = qrow < Lq ? qrow : Lq - 1; // rows past the end re-read the last one and are not stored
    const bf16_t* qp = q + (int64_t)b * q_bs + (int64_t)qcl * q_rs + head * DH;
    bf16x8 qf[DH / 16];
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks) qf[ks] = *(const bf16x8*)(qp + 16 * ks + 8 * h);
    const bf16_t* Kb = k + (int64_t)b * k_bs + kvh * DH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + kvh * DH;
    f32x16 oacc[DH / 32];
#pragma unroll
    for (int db = 0; db < DH / 32; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    int kend = Lkv, klo = 0;
    if constexpr (CAUSAL) kend = min(Lkv, Q0 + AQ);                    // keys beyond the workgroup's last query row are masked for all of its rows
    if constexpr (RAGGED) {
        kend = min(kvl, kend);                                         // ... and so are those beyond the sample's length
        klo = window ? max(0, Q0 - window + 1) : 0;                    // the first key the workgroup's first row still sees
    }
    for (int k0 = (klo / KT) * KT; k0 < kend; k0 += KT) {
        __syncthreads();                       // the previous tile's LDS reads are done (first pass: nothing to wait for)
#pragma unroll
        for (int i = 0; i < KT * CPR / 256; ++i) {
            const int id = tid + 256 * i, row = id / CPR, ch = id % CPR;
            const int kr = min(k0 + row, Lkv - 1);                     // keys past the end re-read the last one and are masked below
            const u32x4 kv = *(const u32x4*)(Kb + (int64_t)kr * k_rs + ch * 8);
            const u32x4 vv = *(const u32x4*)(Vb + (int64_t)kr * v_rs + ch * 8);
            *(u32x4*)(Ks + row * KROW + ch * 8) = kv;
            bf16_t* vt = Vt + (ch * 8) * VROW + row;
            vt[0 * VROW] = (bf16_t)(vv.x & 0xffffu); vt[1 * VROW] = (bf16_t)(vv.x >> 16);
            vt[2 * VROW] = (bf16_t)(vv.y & 0xffffu); vt[3 * VROW] = (bf16_t)(vv.y >> 16);
            vt[4 * VROW] = (bf16_t)(vv.z & 0xffffu); vt[5 * VROW] = (bf16_t)(vv.z >> 16);
            vt[6 * VROW] = (bf16_t)(vv.w & 0xffffu); vt[7 * VROW] = (bf16_t)(vv.w >> 16);
        }
        __syncthreads();                       // also publishes the bias table on the first pass
        // wholly above this wave's diagonal or behind its first row's window: nothing to add (every wave still reaches the barriers)
        if constexpr (RAGGED) { if (k0 > q0 + 31 || (window && k0 + KT - 1 <= q0 - window)) continue; }
        else { if (CAUSAL && k0 > q0 + 31) continue; }
        f32x16 s[KT / 32];
#pragma unroll
        for (int kb = 0; kb < KT / 32; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < DH / 16; ++ks) {
                const bf16x8 af = *(const bf16x8*)(Ks + (kb * 32 + r) * KROW + 16 * ks + 8 * h);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, qf[ks], s[kb], 0, 0, 0);
            }
        }
        // register i of block kb holds key k0 + 32 kb + 8 (i / 4) + 4 h + i % 4 of query qrow
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KT / 32; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = k0 + kb * 32 + (i >> 2) * 8 + 4 * h + (i & 3);
                float x = s[kb][i] * c0;
                if constexpr (CAP) {
                    const float e = __builtin_amdgcn_exp2f(x);         // e^(2 y), y = softmax_scale q.k / cap; 0 and inf give -1 and 1
                    x = (1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f)) * c1;
                }
                if constexpr (BIAS) x += tab[min(max(key - qrow + rel_len - 1, 0), tab_n - 1)];      // in range for every key / query that counts
                if constexpr (RAGGED) { if (key > qrow || key >= kvl || (window && key <= qrow - window)) x = -INFINITY; }
                else { if (key >= Lkv || (CAUSAL && key > qrow)) x = -INFINITY; }
                s[kb][i] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);         // without RAGGED finite from the first tile on: key 0 is never masked
        const float ms = RAGGED && mn == -INFINITY ? 0.f : mn;         // a row with no live key so far: every p below is exp2(-inf) = 0
        const float alpha = exp2f(m - ms);     // 0 until the first live key
        m = mn;
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < KT / 32; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { const float p = exp2f(s[kb][i] - ms); s[kb][i] = p; psum += p; }
        l = l * alpha + psum;
#pragma unroll
        for (int db = 0; db < DH / 32; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
#pragma unroll
        for (int kb = 0; kb < KT / 32; ++kb)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const u32x4 pk = {pack2bf(s[kb][8 * sp + 0], s[kb][8 * sp + 1]), pack2bf(s[kb][8 * sp + 2], s[kb][8 * sp + 3]),
                                  pack2bf(s[kb][8 * sp + 4], s[kb][8 * sp + 5]), pack2bf(s[kb][8 * sp + 6], s[kb][8 * sp + 7])};
                const bf16x8 pb = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
                for (int db = 0; db < DH / 32; ++db) {
                    const bf16_t* vr = Vt + (db * 32 + r) * VROW + kb * 32 + 16 * sp + 4 * h;
                    const bf16x4 lo = *(const bf16x4*)vr, hi = *(const bf16x4*)(vr + 8);
                    const bf16x8 af = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pb, oacc[db], 0, 0, 0);
                }
            }
    }
    l += __shfl_xor(l, 32, 64);
    if (qrow < Lq) {
        const float inv = !RAGGED || l > 0.f ? 1.0f / l : 0.f;         // no live key: zeros
        bf16_t* op = o + (int64_t)b * o_bs + (int64_t)qrow * o_rs + head * DH;
#pragma unroll
        for (int db = 0; db < DH / 32; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {      // registers 4g .. 4g + 3 are d = 32 db + 8 g + 4 h + 0..3
                const u32x2 w = {pack2bf(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv), pack2bf(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
                *(u32x2*)(op + db * 32 + g * 8 + 4 * h) = w;
            }
    }
}

// table[h][j] = weight[bucket(j - (L - 1))][h], j in [0, 2L - 1): T5's bidirectional bucket of the relative position k - q (Raffel et al. 2020;
// transformers T5Attention._relative_position_bucket): the upper half of the buckets for k > q; in each half distances below max_exact =
// num_buckets / 4 have a bucket each, the rest share logarithmically growing ones up to max_distance; fp32 arithmetic, truncation.
template <typename T>
__global__ __launch_bounds__(256) void t5_rel_table_kernel(const T* __restrict__ weight, int num_buckets, int max_distance, int heads, int L,
                                                           float* __restrict__ table) {
    const int n = 2 * L - 1;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int rel = j - (L - 1);
    const int nb = num_buckets / 2, max_exact = nb / 2;
    int bucket = rel > 0 ? nb : 0;
    const int dist = rel < 0 ? -rel : rel;
    if (dist < max_exact) {
        bucket += dist;
    } else {
        const float den = (float)log((double)max_distance / (double)max_exact);        // a Python float in the module, rounded once to fp32 by the division
        const float f = logf((float)dist / (float)max_exact) / den * (float)(nb - max_exact);
        bucket += min(max_exact + (int)f, nb - 1);
    }
    for (int hd = 0; hd < heads; ++hd) table[(int64_t)hd * n + j] = ElemT<T>::ld(weight + (int64_t)bucket * heads + hd);
}

// Row norms over the model width. One wave per row, four rows per workgroup; with REG the row (up to NORM_MAXC x 64 chunks of 8 elements =
// 4608 columns) is read once with 16-byte accesses and stays in registers for the statistics and the output pass (ug_adaln_modulate's fast
// path); wider rows are read again from memory. The KIND says what is normalised and how a chunk is written:
//   NormT5     T5LayerNorm, y = rnd(w * rnd(x * rsqrt(mean(x^2) + eps))) (no mean subtraction, the module's two bf16 rounding points);
//   NormLN     nn.LayerNorm, y = rnd((x - mean) * rsqrt(var + eps) * w + b), var = mean((x - mean)^2);
//   NormGemma  Gemma2RMSNorm, y = rnd((x * rsqrt(mean(x^2) + eps)) * (1 + w)) in fp32 with one rounding, and out = rnd(residual + y) where a
//              residual is given. out may be x or the residual itself: a lane rewrites only what it has read.
constexpr int NORM_MAXC = 9;
struct NormT5 { static constexpr bool LN = false, GEMMA = false; };
struct NormLN { static constexpr bool LN = true, GEMMA = false; };
struct NormGemma { static constexpr bool LN = false, GEMMA = true; };
template <typename KIND, typename P> using norm_io_ptr = std::conditional_t<KIND::GEMMA, P, P __restrict__>;      // only NormGemma's x and out may alias

template <typename T, typename KIND, bool REG>
__global__ __launch_bounds__(256) void norm_rows_kernel(norm_io_ptr<KIND, const T*> x, int64_t ldx, const T* __restrict__ w, const T* __restrict__ bias,
                                                        norm_io_ptr<KIND, T*> out, int64_t ldo, int64_t rows, int D, float eps, const T* residual, int64_t ldr) {
    using E = ElemT<T>;
    constexpr bool LN = KIND::LN;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                   // whole waves leave; no barrier below
    const T* xr = x + row * ldx;
    const T* rr = KIND::GEMMA && residual ? residual + row * ldr : nullptr;
    T* orow = out + row * ldo;
    const int nch = D / 8;
    constexpr int NC = REG ? NORM_MAXC : 1;
    float xv[NC][8];
    float s = 0.f;
    if constexpr (REG) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int ch = lane + 64 * cc;
            if (ch < nch) {
                E::load8(xr + 8 * ch, xv[cc]);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += LN ? xv[cc][e] : xv[cc][e] * xv[cc][e];
            }
        }
    } else {
        for (int ch = lane; ch < nch; ch += 64) {
            E::load8(xr + 8 * ch, xv[0]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += LN ? xv[0][e] : xv[0][e] * xv[0][e];
        }
    }
    s = wave_sum(s);
    float mean = 0.f, var;
    if constexpr (LN) {
        mean = s / (float)D;
        float s2 = 0.f;
        if constexpr (REG) {
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                if (lane + 64 * cc < nch) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float d = xv[cc][e] - mean; s2 += d * d; }
                }
            }
        } else {
            for (int ch = lane; ch < nch; ch += 64) {
                E::load8(xr + 8 * ch, xv[0]);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = xv[0][e] - mean; s2 += d * d; }
            }
        }
        var = wave_sum(s2) / (float)D;
    } else {
        var = s / (float)D;
    }
    const float rs = rsqrtf(var + eps);
    auto emit = [&](int ch, const float* xin) {
        float wv[8], bv[8], y[8];              // bv: the bias (NormLN) or the residual (NormGemma)
        E::load8(w + 8 * ch, wv);
        if constexpr (LN) E::load8(bias + 8 * ch, bv);
        if (rr) E::load8(rr + 8 * ch, bv);     // read before the store
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (LN) y[e] = (xin[e] - mean) * rs * wv[e] + bv[e];
            else if constexpr (KIND::GEMMA) y[e] = (xin[e] * rs) * (1.0f + wv[e]);
            else y[e] = wv[e] * E::rnd(xin[e] * rs);
            if (rr) y[e] = bv[e] + E::rnd(y[e]);
        }
        E::store8(orow + 8 * ch, y);
    };
    if constexpr (REG) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int ch = lane + 64 * cc;
            if (ch < nch) emit(ch, xv[cc]);
        }
    } else {
        for (int ch = lane; ch < nch; ch += 64) {
            E::load8(xr + 8 * ch, xv[0]);
            emit(ch, xv[0]);
        }
    }
}

// apply_rotary_pos_emb with rotate_half at head width 256, in place: one thread per 8 columns i .. i + 7 of a head's lower half and the 8 at i + 128.
// y_lo = rnd(rnd(x_lo cos) - rnd(x_hi sin)), y_hi = rnd(rnd(x_hi cos) + rnd(x_lo sin)): the module's two products and one sum, each a bf16 tensor op.
constexpr int ROPE_DH = 256;

template <typename T>
__global__ __launch_bounds__(256) void rope_half_kernel(T* __restrict__ buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int nheads,
                                                        const T* __restrict__ cos_tab, const T* __restrict__ sin_tab) {
    using E = ElemT<T>;
    constexpr int HALF = ROPE_DH / 2, CH = HALF / 8;     // 16 threads per head
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * nheads * CH) return;
    const int ch = (int)(i % CH);
    const int64_t rh = i / CH;
    const int hd = (int)(rh % nheads);
    const int64_t row = rh / nheads;
    const int64_t pos = row % rows_per_batch;
    T* p = buf + row * ld + col0 + (int64_t)hd * ROPE_DH + 8 * ch;
    float lo[8], hi[8], c[8], s[8], ylo[8], yhi[8];
    E::load8(p, lo); E::load8(p + HALF, hi);
    E::load8(cos_tab + pos * HALF + 8 * ch, c); E::load8(sin_tab + pos * HALF + 8 * ch, s);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ylo[e] = E::rnd(lo[e] * c[e]) - E::rnd(hi[e] * s[e]);
        yhi[e] = E::rnd(hi[e] * c[e]) + E::rnd(lo[e] * s[e]);
    }
    E::store8(p, ylo); E::store8(p + HALF, yhi);
}

// out[m][n] = rnd(rnd(gelu_new(ab[m][n])) * ab[m][F + n]): T5DenseGatedActDense between its GEMMs. One thread per 8 columns.
template <typename T>
__global__ __launch_bounds__(256) void gated_gelu_kernel(const T* __restrict__ ab, int64_t ld, T* __restrict__ out, int64_t ldo, int64_t M, int64_t F8) {
    using E = ElemT<T>;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * F8) return;
    const int64_t mrow = i / F8, ch = i - mrow * F8;
    float a[8], bb[8], y[8];
    E::load8(ab + mrow * ld + 8 * ch, a);
    E::load8(ab + mrow * ld + 8 * (F8 + ch), bb);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = E::rnd(gelu_tanh_exact(a[e])) * bb[e];
    E::store8(out + mrow * ldo + 8 * ch, y);
}

// Contiguous activations between CLIP's fc1 and fc2 (PwMap, pointwise.h), n a multiple of 8, one thread per 16-byte (bf16) / 2 x 16-byte (fp32) chunk; y may alias x.
struct QuickGelu {             // y = x sigmoid(1.702 x): CLIP-L's "quick_gelu"
    static __device__ __forceinline__ float f(float a) { return a / (1.0f + expf(-1.702f * a)); }
};
// y = 0.5 x (1 + erf(x / sqrt 2)): "gelu", OpenCLIP bigG's. Evaluated in fp32 as 0.5 x erfc(-x / sqrt 2) for x < 0 and 0.5 x (1 + erf(x / sqrt 2))
// otherwise: the two are the same function, but 1 + erf cancels in the negative tail (absolute error 2^-24 |x|, the whole value from x = -5 on),
// where erfc keeps its relative accuracy. Both forms stay at 0.09 of the test's bound (|err| <= 2^-20 |x|) with a correctly rounded erf; the
// erfc tail is taken because it leaves the bf16 entry's single rounding as the only error of a small negative output.
struct GeluErf {
    static __device__ __forceinline__ float f(float a) {
        const float u = a * 0.70710678118654752f;
        return a < 0.0f ? 0.5f * a * erfcf(-u) : 0.5f * a * (1.0f + erff(u));
    }
};

constexpr int REL_LEN_MAX = 4096;             // (2 x 4096 - 1) floats = 32 KiB of table beside the 18 KiB of tiles

static int attn_bias_check(const char* who, const void* q, const void* k, const void* v, const void* o, int64_t batches, int32_t heads, int64_t Lq,
                           int64_t Lkv, const float* rel_table, int64_t rel_len) {
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && Lq > 0 && Lkv > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(Lq < (1 << 30) && Lkv < (1 << 30), UG_ERR_UNSUPPORTED, "%s: sequence too long", who);
    if (rel_table) {
        UG_REQUIRE(rel_len >= Lq && rel_len >= Lkv, UG_ERR_BAD_SHAPE, "%s: rel_len %lld must cover max(Lq, Lkv) = %lld", who, (long long)rel_len,
                   (long long)(Lq > Lkv ? Lq : Lkv));
        UG_REQUIRE(rel_len <= REL_LEN_MAX, UG_ERR_UNSUPPORTED, "%s: rel_len %lld above %d (the head's table slice must fit in LDS)", who, (long long)rel_len,
                   REL_LEN_MAX);
        UG_REQUIRE(ug_aligned(rel_table, 4), UG_ERR_BAD_ALIGN, "%s: rel_table must be 4-byte aligned", who);
    }
    return UG_OK;
}

// the checks both soft-cap entries share, before their views: nothing looked at yet but the counts
static int attn_softcap_check(const char* who, const void* q, const void* k, const void* v, const void* o, int64_t batches, int32_t heads, int32_t kv_heads,
                              int64_t L, int32_t dh, float softcap, int64_t window, const int32_t* kv_len) {
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && kv_heads > 0 && L > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(heads % kv_heads == 0, UG_ERR_BAD_SHAPE, "%s: heads = %d is not a multiple of kv_heads = %d", who, heads, kv_heads);
    UG_REQUIRE(softcap >= 0.f && softcap < INFINITY && window >= 0, UG_ERR_BAD_SHAPE, "%s: softcap %g and window %lld must not be negative (0 = off)", who,
               (double)softcap, (long long)window);
    UG_REQUIRE(dh == 256, UG_ERR_UNSUPPORTED, "%s: head dim %d (256 only)", who, dh);
    UG_REQUIRE(L < (1 << 30), UG_ERR_UNSUPPORTED, "%s: sequence too long", who);
    UG_REQUIRE(!kv_len || ug_aligned(kv_len, 4), UG_ERR_BAD_ALIGN, "%s: kv_len must be 4-byte aligned", who);
    return UG_OK;
}

// the grid limit and the launch of one instantiation, after the entry's own checks and view table
template <int DH, int KT, bool BIAS, bool CAUSAL, bool CAP, bool RAGGED>
static int attn_plain_launch(const char* who, ug_view q, ug_view k, ug_view v, ug_view o, int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv,
                             const attn_plain_args& a, ug_stream_t stream) {
    const int nQ = (int)((Lq + AQ - 1) / AQ);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    const size_t lds = (KT * (DH + 8) + DH * (KT + 8)) * sizeof(bf16_t) + (BIAS ? (size_t)(2 * a.rel_len - 1) * sizeof(float) : 0);      // K, V^T, the table
    hipLaunchKernelGGL((attn_plain_kernel<DH, KT, BIAS, CAUSAL, CAP, RAGGED>), dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q.p, q.rs,
                       q.bs, (const bf16_t*)k.p, k.rs, k.bs, (const bf16_t*)v.p, v.rs, v.bs, (bf16_t*)o.p, o.rs, o.bs, a.rel_table, a.rel_len, (int)heads, (int)Lq,
                       (int)Lkv, nQ, a.c0, a.c1, a.kv_len, a.group, a.window);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T>
static int rope_half_launch(const char* who, void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh,
                            const void* cos_tab, const void* sin_tab, ug_stream_t stream) {
    if (rows == 0 || nheads == 0) return UG_OK;
    UG_REQUIRE(buf && cos_tab && sin_tab && rows > 0 && rows_per_batch > 0 && nheads > 0 && col0 >= 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(dh == ROPE_DH, UG_ERR_UNSUPPORTED, "%s: head dim %d (256 only)", who, dh);
    UG_REQUIRE(ld >= col0 + (int64_t)nheads * ROPE_DH, UG_ERR_BAD_SHAPE, "%s: ld = %lld below col0 + nheads * dh = %lld", who, (long long)ld,
               (long long)(col0 + (int64_t)nheads * ROPE_DH));
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ld % per16 == 0 && col0 % per16 == 0 && ug_aligned(buf, 16) && ug_aligned(cos_tab, 16) && ug_aligned(sin_tab, 16), UG_ERR_BAD_ALIGN,
               "%s: rows, the first column and the tables must be 16-byte aligned", who);
    UG_REQUIRE(rows < (1ll << 40) / nheads, UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    const int64_t nblk = (rows * nheads * (ROPE_DH / 16) + 255) / 256;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    hipLaunchKernelGGL((rope_half_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (T*)buf, ld, rows, rows_per_batch, col0, (int)nheads,
                       (const T*)cos_tab, (const T*)sin_tab);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

// bias: NormLN's (required there); residual, ldr: NormGemma's (optional). The entries of the other kinds pass NULL and 0.
template <typename T, typename KIND>
static int norm_rows_launch(const char* who, KIND, const void* x, int64_t ldx, const void* w, const void* bias, const void* residual, int64_t ldr, void* out,
                            int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream) {
    if (rows == 0) return UG_OK;
    UG_REQUIRE(x && w && out && (!KIND::LN || bias) && rows > 0 && D > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(D % 8 == 0 && D < (1 << 24), UG_ERR_UNSUPPORTED, "%s: D = %lld must be a multiple of 8 (below 2^24)", who, (long long)D);
    UG_REQUIRE(ldx >= D && ldo >= D && (!residual || ldr >= D), UG_ERR_BAD_SHAPE, "%s: leading dimensions below D", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ldx % per16 == 0 && ldo % per16 == 0 && ug_aligned(x, 16) && ug_aligned(out, 16) && ug_aligned(w, 16) && (!KIND::LN || ug_aligned(bias, 16)) &&
               (!residual || (ldr % per16 == 0 && ug_aligned(residual, 16))), UG_ERR_BAD_ALIGN, "%s: rows and weights must be 16-byte aligned", who);
    const int64_t nblk = (rows + 3) / 4;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w, (const T*)bias, (T*)out, ldo, rows,
                           (int)D, eps, (const T*)residual, ldr);
    };
    if (D / 8 <= 64 * NORM_MAXC) launch(norm_rows_kernel<T, KIND, true>);
    else launch(norm_rows_kernel<T, KIND, false>);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T>
static int gated_gelu_launch(const char* who, const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream) {
    if (M == 0) return UG_OK;
    UG_REQUIRE(ab && out && M > 0 && F > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(F % 8 == 0, UG_ERR_UNSUPPORTED, "%s: F = %lld must be a multiple of 8", who, (long long)F);
    UG_REQUIRE(ld >= 2 * F && ldo >= F, UG_ERR_BAD_SHAPE, "%s: leading dimensions too small", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ld % per16 == 0 && ldo % per16 == 0 && ug_aligned(ab, 16) && ug_aligned(out, 16), UG_ERR_BAD_ALIGN, "%s: rows must be 16-byte aligned", who);
    const int64_t n = M * (F / 8), nblk = (n + 255) / 256;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many elements", who);
    hipLaunchKernelGGL((gated_gelu_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)ab, ld, (T*)out, ldo, M, F / 8);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T, typename Act>
static int act8_launch(const char* who, Act, const void* x, void* y, int64_t n, ug_stream_t stream) {
    if (n == 0) return UG_OK;
    UG_REQUIRE(x && y && n > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(n % 8 == 0, UG_ERR_UNSUPPORTED, "%s: n = %lld must be a multiple of 8", who, (long long)n);
    UG_REQUIRE(ug_aligned(x, 16) && ug_aligned(y, 16), UG_ERR_BAD_ALIGN, "%s: tensors must be 16-byte aligned", who);
    UG_REQUIRE(ug_cdiv(n / 8, 256) < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many elements", who);
    return pointwise_launch<T, PwMap<T, Act>, PwLoop::One>(who, ug_grid1d(n / 8, 256), stream, (const T*)x, (T*)y, n / 8);
}

template <typename T>
static int rel_table_launch(const char* who, const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table,
                            ug_stream_t stream) {
    UG_REQUIRE(weight && table && heads > 0 && L > 0 && L < (1 << 29), UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(num_buckets >= 4 && num_buckets % 4 == 0 && max_distance > num_buckets / 4, UG_ERR_UNSUPPORTED,
               "%s: num_buckets %d must be a multiple of 4 and max_distance %d above num_buckets / 4", who, num_buckets, max_distance);
    const int64_t n = 2 * L - 1;
    hipLaunchKernelGGL((t5_rel_table_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)weight, (int)num_buckets,
                       (int)max_distance, (int)heads, (int)L, table);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

}  // namespace

extern "C" int ug_flash_attn_fwd_bias(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                      int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride,
                                      int64_t o_batch_stride, int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                                      const float* rel_table, int64_t rel_len, int32_t causal, ug_stream_t stream) {
    if (!rel_table && !causal)                 // no bias, no mask: this IS ug_flash_attn_fwd
        return ug_flash_attn_fwd(q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                                 o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, stream);
    if (batches == 0 || Lq == 0) return UG_OK;
    if (const int rc = attn_bias_check(__func__, q, k, v, o, batches, heads, Lq, Lkv, rel_table, rel_len)) return rc;
    UG_REQUIRE(dh == 64, UG_ERR_UNSUPPORTED, "%s: head dim %d with a bias or a causal mask (64 only)", __func__, dh);
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, false}, {"k", UG_VIEW(k), 8, 16, false}, {"v", UG_VIEW(v), 8, 16, false}, {"o", UG_VIEW(o), 4, 8, false}};
    if (const int vrc = ug_check_views(__func__, views)) return vrc;
    const attn_plain_args a = {rel_table, (int)rel_len, nullptr, 1, 0, softmax_scale * LOG2E, 0.f};
    const auto launch = !rel_table ? attn_plain_launch<64, 64, false, true, false, false>
                        : causal   ? attn_plain_launch<64, 64, true, true, false, false> : attn_plain_launch<64, 64, true, false, false, false>;
    return launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, Lq, Lkv, a, stream);
}

extern "C" int ug_flash_attn_fwd_bias_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                          int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o,
                                          int64_t o_row_stride, int64_t o_batch_stride, int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                                          float softmax_scale, const float* rel_table, int64_t rel_len, int32_t causal, ug_stream_t stream) {
    if (!rel_table && !causal)
        return ug_flash_attn_fwd_f32(q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                                     o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, stream);
    if (batches == 0 || Lq == 0) return UG_OK;
    if (const int rc = attn_bias_check(__func__, q, k, v, o, batches, heads, Lq, Lkv, rel_table, rel_len)) return rc;
    UG_REQUIRE(dh == 64, UG_ERR_UNSUPPORTED, "%s: head dim %d with a bias or a causal mask (64 only)", __func__, dh);
    ug_attn_f32_mods mods = {};
    mods.rel_table = rel_table; mods.rel_len = (int)rel_len; mods.causal = causal;
    return ug_flash_attn_f32_launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, Lq, Lkv, dh, softmax_scale, mods, stream);
}

extern "C" int ug_flash_attn_fwd_softcap(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                         int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride,
                                         int64_t o_batch_stride, int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh, float softmax_scale,
                                         float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream) {
    if (batches == 0 || L == 0) return UG_OK;
    if (const int rc = attn_softcap_check(__func__, q, k, v, o, batches, heads, kv_heads, L, dh, softcap, window, kv_len)) return rc;
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, false}, {"k", UG_VIEW(k), 8, 16, false}, {"v", UG_VIEW(v), 8, 16, false}, {"o", UG_VIEW(o), 4, 8, false}};
    if (const int vrc = ug_check_views(__func__, views)) return vrc;
    const int win = window >= L ? 0 : (int)window;                     // a window of L or more masks nothing
    const bool cap = softcap > 0.f;
    const attn_plain_args a = {nullptr, 0, kv_len, (int)(heads / kv_heads), win, cap ? 2.0f * LOG2E * (softmax_scale / softcap) : softmax_scale * LOG2E,
                               cap ? softcap * LOG2E : 0.f};
    const auto launch = cap ? attn_plain_launch<256, 32, false, true, true, true> : attn_plain_launch<256, 32, false, true, false, true>;
    return launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, L, L, a, stream);
}

extern "C" int ug_flash_attn_fwd_softcap_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                             int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o,
                                             int64_t o_row_stride, int64_t o_batch_stride, int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh,
                                             float softmax_scale, float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream) {
    if (batches == 0 || L == 0) return UG_OK;
    if (const int rc = attn_softcap_check(__func__, q, k, v, o, batches, heads, kv_heads, L, dh, softcap, window, kv_len)) return rc;
    ug_attn_f32_mods mods = {};
    mods.causal = 1; mods.softcap = softcap; mods.window = window >= L ? 0 : (int)window; mods.kv_len = kv_len; mods.group = heads / kv_heads;
    return ug_flash_attn_f32_launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, L, L, dh, softmax_scale, mods, stream);
}

UG_TWINS(ug_t5_rel_table, rel_table_launch, (const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table, ug_stream_t stream),
         (__func__, weight, num_buckets, max_distance, heads, L, table, stream))
UG_TWINS(ug_rope_half, rope_half_launch,
         (void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh, const void* cos_tab, const void* sin_tab,
          ug_stream_t stream),
         (__func__, buf, ld, rows, rows_per_batch, col0, nheads, dh, cos_tab, sin_tab, stream))
UG_TWINS(ug_rmsnorm_rows, norm_rows_launch, (const void* x, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream),
         (__func__, NormT5{}, x, ldx, w, nullptr, nullptr, 0, out, ldo, rows, D, eps, stream))
UG_TWINS(ug_layernorm_rows, norm_rows_launch,
         (const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream),
         (__func__, NormLN{}, x, ldx, w, bias, nullptr, 0, out, ldo, rows, D, eps, stream))
UG_TWINS(ug_gemma_rmsnorm_rows, norm_rows_launch,
         (const void* x, int64_t ldx, const void* w, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
          ug_stream_t stream),
         (__func__, NormGemma{}, x, ldx, w, nullptr, residual, ldr, out, ldo, rows, D, eps, stream))
UG_TWINS(ug_gated_gelu, gated_gelu_launch, (const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream),
         (__func__, ab, ld, out, ldo, M, F, stream))
UG_TWINS(ug_quick_gelu, act8_launch, (const void* x, void* y, int64_t n, ug_stream_t stream), (__func__, QuickGelu{}, x, y, n, stream))
UG_TWINS(ug_gelu_erf, act8_launch, (const void* x, void* y, int64_t n, ug_stream_t stream), (__func__, GeluErf{}, x, y, n, stream))

