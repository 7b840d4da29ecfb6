// Kernels of the text encoders (T5 encoder, CLIP text model; unigen_amd/text.py). The matrix work of both models is ug_gemm_bf16 and the
// token embedding ug_gather_rows; this file holds what sits between them:
//   ug_flash_attn_fwd_bias   attention with T5's additive relative-position bias (a per-head table of k - q, held in LDS) and / or CLIP's causal mask
//   ug_t5_rel_table          the [heads][2L - 1] table of that bias from block 0's relative_attention_bias.weight
//   ug_rmsnorm_rows          T5LayerNorm;   ug_layernorm_rows   nn.LayerNorm with weight and bias
//   ug_gated_gelu            gelu_new(a) * b over the two halves of the stacked [wi_0; wi_1] projection;   ug_quick_gelu   x sigmoid(1.702 x)
//   ug_gelu_erf              0.5 x (1 + erf(x / sqrt 2)), the activation of SD3's second CLIP (OpenCLIP bigG)
// and the `_f32` verification twin of each (fp32 storage, no intermediate rounding); the attention twin runs verify_f32.hip's one fp32 kernel.
//
// The attention kernel is deliberately plain next to attention.hip's: at T5-XXL (512 tokens, 64 heads) attention is about 2 % of the encoder's
// FLOPs. One workgroup = 4 waves = 128 query rows of one (batch, head), Q fragments in registers, K tiles of 64 keys staged row-major and V
// tiles TRANSPOSED into LDS through registers (single buffer, two barriers per tile). The MFMA formulation is attention.hip's:
//   S^T = K Q^T    v_mfma_f32_32x32x16_bf16, the query index on the lane: scores, bias and masks are lane-local, one exchange with lane ^ 32 for the max;
//   O^T = V^T P^T  accumulator registers 8s .. 8s + 7 of S^T, packed to bf16, are the B operand of k-step s; the A operand reads the matching
//                  keys (16s + 4h + 0..3 and 16s + 8 + 4h + 0..3) of row d of the transposed V image as two 8-byte LDS reads.
// Scores never leave registers; the bias is tab[(k - q) + rel_len - 1] from the head's table slice, loaded into LDS once per workgroup
// (pre-multiplied by log2 e: the softmax runs in base 2). A causal launch ends its key loop at the workgroup's last query row and a wave skips
// the tiles that lie wholly above its own 32 rows' diagonal.
#include "ug_common.h"
#include <math.h>

namespace {

constexpr int AQ = 128;            // query rows per workgroup
constexpr int AK = 64;             // keys per tile
constexpr int AROW = 64 + 8;       // bf16 elements per LDS row (144 bytes: 16-byte aligned rows that do not all start in one bank)
constexpr int ATILE = AK * AROW;   // elements of the K image [key][d]; the V image [d][key] has the same size at head width 64
constexpr float LOG2E = 1.4426950408889634f;

template <bool BIAS, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_bias_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    const float* __restrict__ rel_table, int rel_len, int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bf16_t* Ks = (bf16_t*)smem;                // [64 keys][AROW]
    bf16_t* Vt = Ks + ATILE;                   // [64 d][AROW]: Vt[d][key]
    float* tab = (float*)(Vt + ATILE);         // [2 rel_len - 1], times log2(e)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qt = blockIdx.x % nQ, bh = blockIdx.x / nQ;
    const int head = bh % heads, b = bh / heads;
    const int tab_n = 2 * rel_len - 1;
    if constexpr (BIAS) {
        const float* src = rel_table + (int64_t)head * tab_n;
        for (int i = tid; i < tab_n; i += 256) tab[i] = src[i] * LOG2E;
    }
    const int q0 = qt * AQ + wave * 32;        // the wave's first query row
    const int qrow = q0 + r;
    const int qcl = qrow < Lq ? qrow : Lq - 1; // rows past the end re-read the last one and are not stored
    const bf16_t* qp = q + (int64_t)b * q_bs + (int64_t)qcl * q_rs + head * 64;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(qp + 16 * ks + 8 * h);
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * 64;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * 64;
    f32x16 oacc[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    int kend = Lkv;
    if constexpr (CAUSAL) kend = min(Lkv, qt * AQ + AQ);      // keys beyond the workgroup's last query row are masked for all of its rows
    const int ntiles = (kend + AK - 1) / AK;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * AK;
        __syncthreads();                       // the previous tile's LDS reads are done (first pass: nothing to wait for)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = id & 7;
            const int kr = min(k0 + row, Lkv - 1);                 // keys past the end re-read the last one and are masked below
            const u32x4 kv = *(const u32x4*)(Kb + (int64_t)kr * k_rs + ch * 8);
            const u32x4 vv = *(const u32x4*)(Vb + (int64_t)kr * v_rs + ch * 8);
            *(u32x4*)(Ks + row * AROW + ch * 8) = kv;
            bf16_t* vt = Vt + (ch * 8) * AROW + row;
            vt[0 * AROW] = (bf16_t)(vv.x & 0xffffu); vt[1 * AROW] = (bf16_t)(vv.x >> 16);
            vt[2 * AROW] = (bf16_t)(vv.y & 0xffffu); vt[3 * AROW] = (bf16_t)(vv.y >> 16);
            vt[4 * AROW] = (bf16_t)(vv.z & 0xffffu); vt[5 * AROW] = (bf16_t)(vv.z >> 16);
            vt[6 * AROW] = (bf16_t)(vv.w & 0xffffu); vt[7 * AROW] = (bf16_t)(vv.w >> 16);
        }
        __syncthreads();                       // also publishes the bias table on the first pass
        if (CAUSAL && k0 > q0 + 31) continue;  // wholly above this wave's diagonal: nothing to add (the barriers above are still reached by every wave)
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 a = *(const bf16x8*)(Ks + (kb * 32 + r) * AROW + 16 * ks + 8 * h);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], s[kb], 0, 0, 0);
            }
        }
        // register i of block kb holds key k0 + 32 kb + 8 (i / 4) + 4 h + i % 4 of query qrow
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = k0 + kb * 32 + (i >> 2) * 8 + 4 * h + (i & 3);
                float x = s[kb][i] * c;
                if constexpr (BIAS) x += tab[min(max(key - qrow + rel_len - 1, 0), tab_n - 1)];      // in range for every key / query that counts
                if (key >= Lkv || (CAUSAL && key > qrow)) x = -INFINITY;
                s[kb][i] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);         // finite from the first tile on: key 0 is never masked
        const float alpha = exp2f(m - mn);     // 0 on the first tile
        m = mn;
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { const float p = exp2f(s[kb][i] - mn); s[kb][i] = p; psum += p; }
        l = l * alpha + psum;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                const u32x4 pk = {pack2bf(s[kb][8 * sp + 0], s[kb][8 * sp + 1]), pack2bf(s[kb][8 * sp + 2], s[kb][8 * sp + 3]),
                                  pack2bf(s[kb][8 * sp + 4], s[kb][8 * sp + 5]), pack2bf(s[kb][8 * sp + 6], s[kb][8 * sp + 7])};
                const bf16x8 pb = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const bf16_t* vr = Vt + (db * 32 + r) * AROW + kb * 32 + 16 * sp + 4 * h;
                    const bf16x4 lo = *(const bf16x4*)vr, hi = *(const bf16x4*)(vr + 8);
                    const bf16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, oacc[db], 0, 0, 0);
                }
            }
    }
    l += __shfl_xor(l, 32, 64);
    if (qrow < Lq) {
        const float inv = 1.0f / l;
        bf16_t* op = o + (int64_t)b * o_bs + (int64_t)qrow * o_rs + head * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
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
// path); wider rows are read again from memory. LN = false: T5LayerNorm, y = rnd(w * rnd(x * rsqrt(mean(x^2) + eps))) (no mean subtraction, the
// module's two bf16 rounding points); LN = true: nn.LayerNorm, y = rnd((x - mean) * rsqrt(var + eps) * w + b), var = mean((x - mean)^2).
constexpr int NORM_MAXC = 9;

template <typename T, bool LN, bool REG>
__global__ __launch_bounds__(256) void norm_rows_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, const T* __restrict__ bias,
                                                        T* __restrict__ out, int64_t ldo, int64_t rows, int D, float eps) {
    using E = ElemT<T>;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                   // whole waves leave; no barrier below
    const T* xr = x + row * ldx;
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
        float wv[8], bv[8], y[8];
        E::load8(w + 8 * ch, wv);
        if constexpr (LN) E::load8(bias + 8 * ch, bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (LN) y[e] = (xin[e] - mean) * rs * wv[e] + bv[e];
            else y[e] = wv[e] * E::rnd(xin[e] * rs);
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

__device__ __forceinline__ float gelu_new_f(float x) {          // 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    return 0.5f * x * (1.0f + tanhf(u));
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
    for (int e = 0; e < 8; ++e) y[e] = E::rnd(gelu_new_f(a[e])) * bb[e];
    E::store8(out + mrow * ldo + 8 * ch, y);
}

// Contiguous activations between CLIP's fc1 and fc2, n a multiple of 8, one thread per 16-byte (bf16) / 2 x 16-byte (fp32) chunk; y may alias x.
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

template <typename T, typename Act>
__global__ __launch_bounds__(256) void act8_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n8) {
    using E = ElemT<T>;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float a[8], r[8];
    E::load8(x + 8 * i, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = Act::f(a[e]);
    E::store8(y + 8 * i, r);
}

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

template <typename T, bool LN>
static int norm_rows_launch(const char* who, const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D,
                            float eps, ug_stream_t stream) {
    if (rows == 0) return UG_OK;
    UG_REQUIRE(x && w && out && (!LN || bias) && rows > 0 && D > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(D % 8 == 0 && D < (1 << 24), UG_ERR_UNSUPPORTED, "%s: D = %lld must be a multiple of 8 (below 2^24)", who, (long long)D);
    UG_REQUIRE(ldx >= D && ldo >= D, UG_ERR_BAD_SHAPE, "%s: leading dimensions below D", who);
    constexpr size_t al = sizeof(T) == 2 ? 16 : 16;
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ldx % per16 == 0 && ldo % per16 == 0 && ug_aligned(x, al) && ug_aligned(out, al) && ug_aligned(w, al) && (!LN || ug_aligned(bias, al)),
               UG_ERR_BAD_ALIGN, "%s: rows and weights must be 16-byte aligned", who);
    const int64_t nblk = (rows + 3) / 4;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    if (D / 8 <= 64 * NORM_MAXC)
        hipLaunchKernelGGL((norm_rows_kernel<T, LN, true>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w,
                           (const T*)bias, (T*)out, ldo, rows, (int)D, eps);
    else
        hipLaunchKernelGGL((norm_rows_kernel<T, LN, false>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w,
                           (const T*)bias, (T*)out, ldo, rows, (int)D, eps);
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
static int act8_launch(const char* who, const void* x, void* y, int64_t n, ug_stream_t stream) {
    if (n == 0) return UG_OK;
    UG_REQUIRE(x && y && n > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(n % 8 == 0, UG_ERR_UNSUPPORTED, "%s: n = %lld must be a multiple of 8", who, (long long)n);
    UG_REQUIRE(ug_aligned(x, 16) && ug_aligned(y, 16), UG_ERR_BAD_ALIGN, "%s: tensors must be 16-byte aligned", who);
    const int64_t nblk = (n / 8 + 255) / 256;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many elements", who);
    hipLaunchKernelGGL((act8_kernel<T, Act>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, n / 8);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
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
    const int rc = attn_bias_check("ug_flash_attn_fwd_bias", q, k, v, o, batches, heads, Lq, Lkv, rel_table, rel_len);
    if (rc != UG_OK) return rc;
    UG_REQUIRE(dh == 64, UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_bias: head dim %d with a bias or a causal mask (64 only)", dh);
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, false}, {"k", UG_VIEW(k), 8, 16, false}, {"v", UG_VIEW(v), 8, 16, false}, {"o", UG_VIEW(o), 4, 8, false}};
    if (const int vrc = ug_check_views(__func__, views)) return vrc;
    const int nQ = (int)((Lq + AQ - 1) / AQ);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_bias: grid too large");
    const float c = softmax_scale * LOG2E;
    const size_t lds = 2 * ATILE * sizeof(bf16_t) + (rel_table ? (size_t)(2 * rel_len - 1) * sizeof(float) : 0);
#define UG_ATTN_BIAS_LAUNCH(B, CZ)                                                                                                                  \
    hipLaunchKernelGGL((attn_bias_kernel<B, CZ>), dim3((unsigned)nwg), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride, \
                       (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride,     \
                       o_batch_stride, rel_table, (int)rel_len, (int)heads, (int)Lq, (int)Lkv, nQ, c)
    if (rel_table && causal) UG_ATTN_BIAS_LAUNCH(true, true);
    else if (rel_table) UG_ATTN_BIAS_LAUNCH(true, false);
    else UG_ATTN_BIAS_LAUNCH(false, true);
#undef UG_ATTN_BIAS_LAUNCH
    UG_CHECK_LAUNCH("ug_flash_attn_fwd_bias");
    return UG_OK;
}

extern "C" int ug_flash_attn_fwd_bias_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                          int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o,
                                          int64_t o_row_stride, int64_t o_batch_stride, int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                                          float softmax_scale, const float* rel_table, int64_t rel_len, int32_t causal, ug_stream_t stream) {
    if (!rel_table && !causal)
        return ug_flash_attn_fwd_f32(q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                                     o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, stream);
    if (batches == 0 || Lq == 0) return UG_OK;
    const int rc = attn_bias_check("ug_flash_attn_fwd_bias_f32", q, k, v, o, batches, heads, Lq, Lkv, rel_table, rel_len);
    if (rc != UG_OK) return rc;
    UG_REQUIRE(dh == 64, UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_bias_f32: head dim %d with a bias or a causal mask (64 only)", dh);
    return ug_flash_attn_f32_launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, Lq, Lkv, dh, softmax_scale, rel_table, rel_len,
                                    causal, stream);
}

extern "C" int ug_t5_rel_table(const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table, ug_stream_t stream) {
    return rel_table_launch<bf16_t>("ug_t5_rel_table", weight, num_buckets, max_distance, heads, L, table, stream);
}
extern "C" int ug_t5_rel_table_f32(const void* weight, int32_t num_buckets, int32_t max_distance, int32_t heads, int64_t L, float* table, ug_stream_t stream) {
    return rel_table_launch<float>("ug_t5_rel_table_f32", weight, num_buckets, max_distance, heads, L, table, stream);
}

extern "C" int ug_rmsnorm_rows(const void* x, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream) {
    return norm_rows_launch<bf16_t, false>("ug_rmsnorm_rows", x, ldx, w, nullptr, out, ldo, rows, D, eps, stream);
}
extern "C" int ug_rmsnorm_rows_f32(const void* x, int64_t ldx, const void* w, void* out, int64_t ldo, int64_t rows, int64_t D, float eps, ug_stream_t stream) {
    return norm_rows_launch<float, false>("ug_rmsnorm_rows_f32", x, ldx, w, nullptr, out, ldo, rows, D, eps, stream);
}
extern "C" int ug_layernorm_rows(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
                                 ug_stream_t stream) {
    return norm_rows_launch<bf16_t, true>("ug_layernorm_rows", x, ldx, w, bias, out, ldo, rows, D, eps, stream);
}
extern "C" int ug_layernorm_rows_f32(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
                                     ug_stream_t stream) {
    return norm_rows_launch<float, true>("ug_layernorm_rows_f32", x, ldx, w, bias, out, ldo, rows, D, eps, stream);
}

extern "C" int ug_gated_gelu(const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream) {
    return gated_gelu_launch<bf16_t>("ug_gated_gelu", ab, ld, out, ldo, M, F, stream);
}
extern "C" int ug_gated_gelu_f32(const void* ab, int64_t ld, void* out, int64_t ldo, int64_t M, int64_t F, ug_stream_t stream) {
    return gated_gelu_launch<float>("ug_gated_gelu_f32", ab, ld, out, ldo, M, F, stream);
}
extern "C" int ug_quick_gelu(const void* x, void* y, int64_t n, ug_stream_t stream) { return act8_launch<bf16_t, QuickGelu>("ug_quick_gelu", x, y, n, stream); }
extern "C" int ug_quick_gelu_f32(const void* x, void* y, int64_t n, ug_stream_t stream) { return act8_launch<float, QuickGelu>("ug_quick_gelu_f32", x, y, n, stream); }
extern "C" int ug_gelu_erf(const void* x, void* y, int64_t n, ug_stream_t stream) { return act8_launch<bf16_t, GeluErf>("ug_gelu_erf", x, y, n, stream); }
extern "C" int ug_gelu_erf_f32(const void* x, void* y, int64_t n, ug_stream_t stream) { return act8_launch<float, GeluErf>("ug_gelu_erf_f32", x, y, n, stream); }
