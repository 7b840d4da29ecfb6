// Kernels of the Gemma-2 text encoder (unigen_amd/gemma.py: transformers' Gemma2Model, the prompt encoder of Sana). The matrix work is
// ug_gemm_bf16 and the gated activation ug_gated_gelu (text.hip); this file holds what else sits between the GEMMs:
//   ug_flash_attn_fwd_softcap   causal attention at head width 256 with grouped K/V heads, logit soft-capping, a sliding window and a key length per sample
//   ug_rope_half                apply_rotary_pos_emb (rotate_half) in place on the q and k heads of the packed q | k | v projection
//   ug_gemma_rmsnorm_rows       Gemma2RMSNorm, weight 1 + w, one rounding, with the residual sum that follows two of the layer's four norms
//   ug_gather_rows_scaled       Gemma2TextScaledWordEmbedding: the gathered row times sqrt(hidden_size)
// and the `_f32` verification twin of each (fp32 storage, no intermediate rounding).
//
// The attention kernel is text.hip's, widened: one workgroup = 4 waves = 128 query rows of one (batch, head), one wave per SIMD (Q fragments 64 VGPRs,
// the O^T accumulator 128, S^T 16), K tiles of 32 keys staged row-major ([32][256 + 8] bf16 = 16.5 KiB) and V tiles TRANSPOSED through registers
// ([256][32 + 8] = 20 KiB), single buffer, two barriers per tile:
//   S^T = K Q^T    v_mfma_f32_32x32x16_bf16 over 16 k-steps, the query index on the lane: the cap's tanh and all three masks are lane-local;
//   O^T = V^T P^T  accumulator registers 8s .. 8s + 7 of S^T, packed to bf16, are the B operand of k-step s, as in text.hip.
// The soft cap is cap * tanh(x / cap) with tanh(y) = 1 - 2 / (e^2y + 1) through v_exp_f32 and v_rcp_f32 (exact limits -1 and 1 at e^2y = 0 and inf;
// absolute error a few 2^-24, which the cap multiplies: far below the bf16 rounding of P). The key loop covers only the tiles between the window's
// first key of the workgroup's first row and the last key any of its rows may see (its last row, or the sample's key length); a wave skips tiles wholly
// above its diagonal or behind its window. A row none of whose keys is live (possible only with a window, on padded rows beyond kv_len + window) is
// written as zeros. The fp32 twin is a plain kernel of its own: verify_f32.hip's keeps a whole head row of the accumulator in one thread's
// registers, which at 256 floats would spill; here four adjacent lanes share a query row, 64 columns each.
#include "ug_common.h"
#include <math.h>

namespace {

constexpr int GQ = 128;            // query rows per workgroup
constexpr int GK = 32;             // keys per tile
constexpr int GD = 256;            // head width
constexpr int KROW = GD + 8;       // bf16 elements per row of the K image (528 bytes)
constexpr int VROW = GK + 8;       // bf16 elements per row of the transposed V image (80 bytes)
constexpr float LOG2E = 1.4426950408889634f;

template <bool CAP>
__global__ __launch_bounds__(256) void attn_softcap_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    const int32_t* __restrict__ kv_len, int heads, int group, int L, int nQ, int window,
    float c0 /* CAP: 2 log2(e) softmax_scale / cap, else softmax_scale log2(e) */, float c1 /* cap log2(e) */) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[GK * KROW];      // [32 keys][KROW]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[GD * VROW];      // [256 d][VROW]: Vt[d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qt = blockIdx.x % nQ, bh = blockIdx.x / nQ;
    const int head = bh % heads, b = bh / heads;
    const int kvh = head / group;
    const int kvl = kv_len ? min(max(kv_len[b], 0), L) : L;            // keys at kvl and beyond are padding
    const int Q0 = qt * GQ;
    const int q0 = Q0 + wave * 32;             // the wave's first query row
    const int qrow = q0 + r;
    const int qcl = qrow < L ? qrow : L - 1;   // rows past the end re-read the last one and are not stored
    const bf16_t* qp = q + (int64_t)b * q_bs + (int64_t)qcl * q_rs + head * GD;
    bf16x8 qf[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) qf[ks] = *(const bf16x8*)(qp + 16 * ks + 8 * h);
    const bf16_t* Kb = k + (int64_t)b * k_bs + kvh * GD;
    const bf16_t* Vb = v + (int64_t)b * v_bs + kvh * GD;
    f32x16 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int kend = min(kvl, min(L, Q0 + GQ));                        // keys beyond the workgroup's last row, or the sample's length, are masked for all of its rows
    const int klo = window ? max(0, Q0 - window + 1) : 0;              // the first key the workgroup's first row still sees
    for (int k0 = (klo / GK) * GK; k0 < kend; k0 += GK) {
        __syncthreads();                       // the previous tile's LDS reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = tid + 256 * i, row = id >> 5, ch = id & 31;
            const int kr = min(k0 + row, L - 1);                       // keys past the end re-read the last one and are masked below
            const u32x4 kv = *(const u32x4*)(Kb + (int64_t)kr * k_rs + ch * 8);
            const u32x4 vv = *(const u32x4*)(Vb + (int64_t)kr * v_rs + ch * 8);
            *(u32x4*)(Ks + row * KROW + ch * 8) = kv;
            bf16_t* vt = Vt + (ch * 8) * VROW + row;
            vt[0 * VROW] = (bf16_t)(vv.x & 0xffffu); vt[1 * VROW] = (bf16_t)(vv.x >> 16);
            vt[2 * VROW] = (bf16_t)(vv.y & 0xffffu); vt[3 * VROW] = (bf16_t)(vv.y >> 16);
            vt[4 * VROW] = (bf16_t)(vv.z & 0xffffu); vt[5 * VROW] = (bf16_t)(vv.z >> 16);
            vt[6 * VROW] = (bf16_t)(vv.w & 0xffffu); vt[7 * VROW] = (bf16_t)(vv.w >> 16);
        }
        __syncthreads();
        // wholly above this wave's diagonal or behind its first row's window: nothing to add (every wave still reaches the barriers)
        if (k0 > q0 + 31 || (window && k0 + GK - 1 <= q0 - window)) continue;
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const bf16x8 a = *(const bf16x8*)(Ks + r * KROW + 16 * ks + 8 * h);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], s, 0, 0, 0);
        }
        // register i holds key k0 + 8 (i / 4) + 4 h + i % 4 of query qrow
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + (i >> 2) * 8 + 4 * h + (i & 3);
            float x = s[i] * c0;
            if constexpr (CAP) {
                const float e = __builtin_amdgcn_exp2f(x);             // e^(2 y), y = softmax_scale q.k / cap; 0 and inf give -1 and 1
                x = (1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f)) * c1;
            }
            if (key > qrow || key >= kvl || (window && key <= qrow - window)) x = -INFINITY;
            s[i] = x;
            mx = fmaxf(mx, x);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float ms = mn == -INFINITY ? 0.f : mn;                   // a row with no live key so far: every p below is exp2(-inf) = 0
        const float alpha = exp2f(m - ms);     // 0 until the first live key
        m = mn;
        float psum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { const float p = exp2f(s[i] - ms); s[i] = p; psum += p; }
        l = l * alpha + psum;
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
            const u32x4 pk = {pack2bf(s[8 * sp + 0], s[8 * sp + 1]), pack2bf(s[8 * sp + 2], s[8 * sp + 3]),
                              pack2bf(s[8 * sp + 4], s[8 * sp + 5]), pack2bf(s[8 * sp + 6], s[8 * sp + 7])};
            const bf16x8 pb = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
            for (int db = 0; db < 8; ++db) {
                const bf16_t* vr = Vt + (db * 32 + r) * VROW + 16 * sp + 4 * h;
                const bf16x4 lo = *(const bf16x4*)vr, hi = *(const bf16x4*)(vr + 8);
                const bf16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, oacc[db], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (qrow < L) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;                    // no live key: zeros
        bf16_t* op = o + (int64_t)b * o_bs + (int64_t)qrow * o_rs + head * GD;
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {      // registers 4g .. 4g + 3 are d = 32 db + 8 g + 4 h + 0..3
                const u32x2 w = {pack2bf(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv), pack2bf(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv)};
                *(u32x2*)(op + db * 32 + g * 8 + 4 * h) = w;
            }
    }
}

// The fp32 twin: 64 query rows of one (batch, head) per workgroup, four adjacent lanes per row with 64 columns of q and of the accumulator each
// (the dot product's four partial sums meet through two lane exchanges), keys streamed one at a time over the row's own live range, exact online
// softmax with expf and the cap with tanhf. No LDS, no barrier.
__global__ __launch_bounds__(256) void attn_softcap_f32_kernel(
    const float* __restrict__ q, int64_t q_rs, int64_t q_bs, const float* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const float* __restrict__ v, int64_t v_rs, int64_t v_bs, float* __restrict__ o, int64_t o_rs, int64_t o_bs,
    const int32_t* __restrict__ kv_len, int heads, int group, int L, int nQ, int window, float scale, float cap) {
    const int tid = threadIdx.x, part = tid & 3;
    const int qt = blockIdx.x % nQ, bh = blockIdx.x / nQ;
    const int head = bh % heads, b = bh / heads;
    const int kvh = head / group;
    const int kvl = kv_len ? min(max(kv_len[b], 0), L) : L;
    const int row = qt * 64 + (tid >> 2);
    const int rl = row < L ? row : L - 1;      // rows past the end repeat the last one (the four lanes of a row stay together) and are not stored
    const float* qp = q + (int64_t)b * q_bs + (int64_t)rl * q_rs + head * GD + part * 64;
    float qv[64], acc[64];
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
        const f32x4 t = *(const f32x4*)(qp + d);
        qv[d] = t[0]; qv[d + 1] = t[1]; qv[d + 2] = t[2]; qv[d + 3] = t[3];
        acc[d] = acc[d + 1] = acc[d + 2] = acc[d + 3] = 0.f;
    }
    const float* Kb = k + (int64_t)b * k_bs + kvh * GD + part * 64;
    const float* Vb = v + (int64_t)b * v_bs + kvh * GD + part * 64;
    float m = -INFINITY, l = 0.f;
    const int jlo = window ? max(0, rl - window + 1) : 0, jhi = min(rl + 1, kvl);
    for (int j = jlo; j < jhi; ++j) {
        const float* kr = Kb + (int64_t)j * k_rs;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            const f32x4 kv = *(const f32x4*)(kr + d);
            s = fmaf(qv[d], kv[0], s); s = fmaf(qv[d + 1], kv[1], s); s = fmaf(qv[d + 2], kv[2], s); s = fmaf(qv[d + 3], kv[3], s);
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s *= scale;
        if (cap > 0.f) s = cap * tanhf(s / cap);
        const float mn = fmaxf(m, s);
        const float alpha = expf(m - mn);      // exp(-inf) = 0 on the first key
        const float pj = expf(s - mn);
        l = l * alpha + pj;
        m = mn;
        const float* vr = Vb + (int64_t)j * v_rs;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            const f32x4 vv = *(const f32x4*)(vr + d);
            acc[d] = fmaf(pj, vv[0], acc[d] * alpha); acc[d + 1] = fmaf(pj, vv[1], acc[d + 1] * alpha);
            acc[d + 2] = fmaf(pj, vv[2], acc[d + 2] * alpha); acc[d + 3] = fmaf(pj, vv[3], acc[d + 3] * alpha);
        }
    }
    if (row < L) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        float* op = o + (int64_t)b * o_bs + (int64_t)row * o_rs + head * GD + part * 64;
#pragma unroll
        for (int d = 0; d < 64; d += 4) *(f32x4*)(op + d) = (f32x4){acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
    }
}

// apply_rotary_pos_emb with rotate_half, in place: one thread per 8 columns i .. i + 7 of a head's lower half and the 8 at i + 128.
// y_lo = rnd(rnd(x_lo cos) - rnd(x_hi sin)), y_hi = rnd(rnd(x_hi cos) + rnd(x_lo sin)): the module's two products and one sum, each a bf16 tensor op.
template <typename T>
__global__ __launch_bounds__(256) void rope_half_kernel(T* __restrict__ buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int nheads,
                                                        const T* __restrict__ cos_tab, const T* __restrict__ sin_tab) {
    using E = ElemT<T>;
    constexpr int HALF = GD / 2, CH = HALF / 8;          // 16 threads per head
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * nheads * CH) return;
    const int ch = (int)(i % CH);
    const int64_t rh = i / CH;
    const int hd = (int)(rh % nheads);
    const int64_t row = rh / nheads;
    const int64_t pos = row % rows_per_batch;
    T* p = buf + row * ld + col0 + (int64_t)hd * GD + 8 * ch;
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

// Gemma2RMSNorm: y = rnd((x * rsqrt(mean(x^2) + eps)) * (1 + w)) in fp32 with one rounding, and out = rnd(residual + y) where a residual is given.
// One wave per row, four rows per workgroup, the row in registers up to GN_MAXC x 64 chunks of 8 (4608 columns), as text.hip's norm_rows_kernel.
constexpr int GN_MAXC = 9;

template <typename T, bool REG>
__global__ __launch_bounds__(256) void gemma_norm_rows_kernel(const T* x, int64_t ldx, const T* __restrict__ w, const T* residual, int64_t ldr,
                                                              T* out, int64_t ldo, int64_t rows, int D, float eps) {
    using E = ElemT<T>;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                   // whole waves leave; no barrier below
    const T* xr = x + row * ldx;
    const T* rr = residual ? residual + row * ldr : nullptr;
    T* orow = out + row * ldo;
    const int nch = D / 8;
    constexpr int NC = REG ? GN_MAXC : 1;
    float xv[NC][8];
    float s = 0.f;
    if constexpr (REG) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int ch = lane + 64 * cc;
            if (ch < nch) {
                E::load8(xr + 8 * ch, xv[cc]);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += xv[cc][e] * xv[cc][e];
            }
        }
    } else {
        for (int ch = lane; ch < nch; ch += 64) {
            E::load8(xr + 8 * ch, xv[0]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += xv[0][e] * xv[0][e];
        }
    }
    const float rs = rsqrtf(wave_sum(s) / (float)D + eps);
    auto emit = [&](int ch, const float* xin) {
        float wv[8], rv[8], y[8];
        E::load8(w + 8 * ch, wv);
        if (rr) E::load8(rr + 8 * ch, rv);     // read before the store: out may be x or the residual itself (a lane rewrites only what it has read)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            y[e] = (xin[e] * rs) * (1.0f + wv[e]);
            if (rr) y[e] = rv[e] + E::rnd(y[e]);
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

// out[i][:W] = rnd(src[idx[i]][:W] * scale) (zeros when idx[i] < 0): ug_gather_rows with the embedding's multiplier.
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_scaled_kernel(const T* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ idx, T* __restrict__ out,
                                                                 int64_t ld_out, int64_t n, int chunks_per_row, float scale) {
    const int64_t total = n * chunks_per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / chunks_per_row; const int c = (int)(i - r * chunks_per_row);
        const int s = idx[r];
        if (s >= 0) {
            float f[8];
            ElemT<T>::load8(src + (int64_t)s * ld_src + c * 8, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= scale;
            ElemT<T>::store8(out + r * ld_out + c * 8, f);
        } else {
            ElemT<T>::zero8(out + r * ld_out + c * 8);
        }
    }
}

// the checks both attention entries share, before their views: nothing looked at yet but the counts
static int attn_softcap_check(const char* who, const void* q, const void* k, const void* v, const void* o, int64_t batches, int32_t heads, int32_t kv_heads,
                              int64_t L, int32_t dh, float softmax_scale, float softcap, int64_t window, const int32_t* kv_len) {
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && kv_heads > 0 && L > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(heads % kv_heads == 0, UG_ERR_BAD_SHAPE, "%s: heads = %d is not a multiple of kv_heads = %d", who, heads, kv_heads);
    UG_REQUIRE(softcap >= 0.f && softcap < INFINITY && window >= 0, UG_ERR_BAD_SHAPE, "%s: softcap %g and window %lld must not be negative (0 = off)", who,
               (double)softcap, (long long)window);
    UG_REQUIRE(dh == GD, UG_ERR_UNSUPPORTED, "%s: head dim %d (256 only)", who, dh);
    UG_REQUIRE(L < (1 << 30), UG_ERR_UNSUPPORTED, "%s: sequence too long", who);
    UG_REQUIRE(!kv_len || ug_aligned(kv_len, 4), UG_ERR_BAD_ALIGN, "%s: kv_len must be 4-byte aligned", who);
    return UG_OK;
}

template <typename T>
static int rope_half_launch(const char* who, void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh,
                            const void* cos_tab, const void* sin_tab, ug_stream_t stream) {
    if (rows == 0 || nheads == 0) return UG_OK;
    UG_REQUIRE(buf && cos_tab && sin_tab && rows > 0 && rows_per_batch > 0 && nheads > 0 && col0 >= 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(dh == GD, UG_ERR_UNSUPPORTED, "%s: head dim %d (256 only)", who, dh);
    UG_REQUIRE(ld >= col0 + (int64_t)nheads * GD, UG_ERR_BAD_SHAPE, "%s: ld = %lld below col0 + nheads * dh = %lld", who, (long long)ld,
               (long long)(col0 + (int64_t)nheads * GD));
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ld % per16 == 0 && col0 % per16 == 0 && ug_aligned(buf, 16) && ug_aligned(cos_tab, 16) && ug_aligned(sin_tab, 16), UG_ERR_BAD_ALIGN,
               "%s: rows, the first column and the tables must be 16-byte aligned", who);
    UG_REQUIRE(rows < (1ll << 40) / nheads, UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    const int64_t nblk = (rows * nheads * (GD / 16) + 255) / 256;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    hipLaunchKernelGGL((rope_half_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (T*)buf, ld, rows, rows_per_batch, col0, (int)nheads,
                       (const T*)cos_tab, (const T*)sin_tab);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T>
static int gemma_norm_launch(const char* who, const void* x, int64_t ldx, const void* w, const void* residual, int64_t ldr, void* out, int64_t ldo,
                             int64_t rows, int64_t D, float eps, ug_stream_t stream) {
    if (rows == 0) return UG_OK;
    UG_REQUIRE(x && w && out && rows > 0 && D > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(D % 8 == 0 && D < (1 << 24), UG_ERR_UNSUPPORTED, "%s: D = %lld must be a multiple of 8 (below 2^24)", who, (long long)D);
    UG_REQUIRE(ldx >= D && ldo >= D && (!residual || ldr >= D), UG_ERR_BAD_SHAPE, "%s: leading dimensions below D", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ldx % per16 == 0 && ldo % per16 == 0 && ug_aligned(x, 16) && ug_aligned(out, 16) && ug_aligned(w, 16) &&
               (!residual || (ldr % per16 == 0 && ug_aligned(residual, 16))), UG_ERR_BAD_ALIGN, "%s: rows and the weight must be 16-byte aligned", who);
    const int64_t nblk = (rows + 3) / 4;
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    if (D / 8 <= 64 * GN_MAXC)
        hipLaunchKernelGGL((gemma_norm_rows_kernel<T, true>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w,
                           (const T*)residual, ldr, (T*)out, ldo, rows, (int)D, eps);
    else
        hipLaunchKernelGGL((gemma_norm_rows_kernel<T, false>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w,
                           (const T*)residual, ldr, (T*)out, ldo, rows, (int)D, eps);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T>
static int gather_rows_scaled_launch(const char* who, const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W,
                                     float scale, ug_stream_t stream) {
    if (n == 0 || W == 0) return UG_OK;
    UG_REQUIRE(src && idx && out && n > 0 && W > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(ld_src >= W && ld_out >= W, UG_ERR_BAD_SHAPE, "%s: leading dimensions below W", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(W % 8 == 0 && ld_src % per16 == 0 && ld_out % per16 == 0 && ug_aligned(src, 16) && ug_aligned(out, 16) && ug_aligned(idx, 4), UG_ERR_BAD_ALIGN,
               "%s: W must be a multiple of 8 and rows 16-byte aligned", who);
    const int64_t total = n * (W / 8);
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL((gather_rows_scaled_kernel<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)src, ld_src, idx, (T*)out, ld_out, n, (int)(W / 8),
                       scale);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

}  // namespace

extern "C" int ug_flash_attn_fwd_softcap(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                         int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride,
                                         int64_t o_batch_stride, int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh, float softmax_scale,
                                         float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream) {
    if (batches == 0 || L == 0) return UG_OK;
    if (const int rc = attn_softcap_check(__func__, q, k, v, o, batches, heads, kv_heads, L, dh, softmax_scale, softcap, window, kv_len)) return rc;
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, false}, {"k", UG_VIEW(k), 8, 16, false}, {"v", UG_VIEW(v), 8, 16, false}, {"o", UG_VIEW(o), 4, 8, false}};
    if (const int vrc = ug_check_views(__func__, views)) return vrc;
    const int nQ = (int)((L + GQ - 1) / GQ);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: grid too large", __func__);
    const int win = window >= L ? 0 : (int)window;                     // a window of L or more masks nothing
#define UG_SOFTCAP_LAUNCH(CAP, C0, C1)                                                                                                              \
    hipLaunchKernelGGL((attn_softcap_kernel<CAP>), dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride, \
                       (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride,     \
                       o_batch_stride, kv_len, (int)heads, (int)(heads / kv_heads), (int)L, nQ, win, C0, C1)
    if (softcap > 0.f) UG_SOFTCAP_LAUNCH(true, 2.0f * LOG2E * (softmax_scale / softcap), softcap * LOG2E);
    else UG_SOFTCAP_LAUNCH(false, softmax_scale * LOG2E, 0.f);
#undef UG_SOFTCAP_LAUNCH
    UG_CHECK_LAUNCH(__func__);
    return UG_OK;
}

extern "C" int ug_flash_attn_fwd_softcap_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                                             int64_t k_batch_stride, const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o,
                                             int64_t o_row_stride, int64_t o_batch_stride, int64_t batches, int32_t heads, int32_t kv_heads, int64_t L, int32_t dh,
                                             float softmax_scale, float softcap, int64_t window, const int32_t* kv_len, ug_stream_t stream) {
    if (batches == 0 || L == 0) return UG_OK;
    if (const int rc = attn_softcap_check(__func__, q, k, v, o, batches, heads, kv_heads, L, dh, softmax_scale, softcap, window, kv_len)) return rc;
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 4, 16, false}, {"k", UG_VIEW(k), 4, 16, false}, {"v", UG_VIEW(v), 4, 16, false}, {"o", UG_VIEW(o), 4, 16, false}};
    if (const int vrc = ug_check_views(__func__, views)) return vrc;
    const int nQ = (int)((L + 63) / 64);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: grid too large", __func__);
    const int win = window >= L ? 0 : (int)window;
    hipLaunchKernelGGL(attn_softcap_f32_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const float*)q, q_row_stride, q_batch_stride,
                       (const float*)k, k_row_stride, k_batch_stride, (const float*)v, v_row_stride, v_batch_stride, (float*)o, o_row_stride, o_batch_stride,
                       kv_len, (int)heads, (int)(heads / kv_heads), (int)L, nQ, win, softmax_scale, softcap);
    UG_CHECK_LAUNCH(__func__);
    return UG_OK;
}

UG_TWINS(ug_rope_half, rope_half_launch,
         (void* buf, int64_t ld, int64_t rows, int64_t rows_per_batch, int64_t col0, int32_t nheads, int32_t dh, const void* cos_tab, const void* sin_tab,
          ug_stream_t stream),
         (__func__, buf, ld, rows, rows_per_batch, col0, nheads, dh, cos_tab, sin_tab, stream))
UG_TWINS(ug_gemma_rmsnorm_rows, gemma_norm_launch,
         (const void* x, int64_t ldx, const void* w, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows, int64_t D, float eps,
          ug_stream_t stream),
         (__func__, x, ldx, w, residual, ldr, out, ldo, rows, D, eps, stream))
UG_TWINS(ug_gather_rows_scaled, gather_rows_scaled_launch,
         (const void* src, int64_t ld_src, const int32_t* idx, void* out, int64_t ld_out, int64_t n, int64_t W, float scale, ug_stream_t stream),
         (__func__, src, ld_src, idx, out, ld_out, n, W, scale, stream))
