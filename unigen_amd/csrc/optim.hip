// Optimizer step of the control-module training loop (reference train.py:652-662): gradient-norm clipping
// (accelerator.clip_grad_norm_, :658) and torch.optim.AdamW (:660) over every trainable tensor in one multi-tensor pass.
//   ug_grad_sumsq    squared L2 norm of all grads -> total_norm and clip_coef (two launches: per-chunk partials, one fixed-order fp64 sum)
//   ug_grad_scale    grad *= clip_coef in place (the stand-alone clip_grad_norm_)
//   ug_adamw_step    one fp32 pass per element with torch.optim.AdamW's single-tensor arithmetic, clipping optionally fused (grads only read)
//   ug_adamw_step_lowp  the same arithmetic for bf16 params without fp32 masters and / or with bf16 moments: what is kept in bf16 is written
//                    with stochastic rounding (Philox4x32-10 draws, ug_sr_round_bf16 exposes the rounding alone)
// Work list: a device table of ug_optim_tensor descriptors and a host-built list of (tensor, chunk) pairs of UG_OPTIM_CHUNK elements, so
// one launch covers every tensor. Each block takes one chunk: 16-byte vector accesses on the body where every stream of the chunk is 16-byte
// aligned at a common element, scalar head and tail (views into the engine's packs may start mid-buffer). No atomics: reproducible bitwise.
#include "ug_common.h"
#include <type_traits>

namespace {

constexpr int OPT_THREADS = 256;
constexpr int RED_THREADS = 1024;

struct AdamwGroups { ug_adamw_group g[UG_ADAMW_MAX_GROUPS]; };

// 8 grad elements at p + i (16-byte aligned body) / one element
__device__ __forceinline__ void ld_grad8(const void* p, int64_t i, bool bf, float* f) {
    if (bf) ElemT<bf16_t>::load8((const bf16_t*)p + i, f);
    else ElemT<float>::load8((const float*)p + i, f);
}
__device__ __forceinline__ float ld_grad1(const void* p, int64_t i, bool bf) { return bf ? bf2f(((const bf16_t*)p)[i]) : ((const float*)p)[i]; }

// first element index h in [0, 8) at which every stream of the chunk is 16-byte aligned, or n (scalar chunk)
__device__ __forceinline__ int body_start(const void* const* ptrs, const int* esz, int np, int n) {
    for (int h = 0; h < 8; ++h) {
        bool ok = true;
        for (int j = 0; j < np; ++j) ok = ok && ((reinterpret_cast<uintptr_t>(ptrs[j]) + (uintptr_t)h * esz[j]) % 16 == 0);
        if (ok) return h < n ? h : n;
    }
    return n;
}

__device__ __forceinline__ void chunk_of(const ug_optim_tensor* table, const int32_t* chunks, const ug_optim_tensor*& d, int64_t& off, int& n) {
    const int t = chunks[2 * (int64_t)blockIdx.x], c = chunks[2 * (int64_t)blockIdx.x + 1];
    d = table + t;
    off = (int64_t)c * UG_OPTIM_CHUNK;
    const int64_t rem = d->numel - off;
    n = rem < UG_OPTIM_CHUNK ? (int)rem : UG_OPTIM_CHUNK;
}

// ---- squared norm: fp32 per lane and inside the wave, fp64 across the waves of the chunk -> partial[chunk] --------------------------------
__global__ __launch_bounds__(OPT_THREADS) void sumsq_kernel(const ug_optim_tensor* __restrict__ table, const int32_t* __restrict__ chunks,
                                                            double* __restrict__ partial) {
    const ug_optim_tensor* d; int64_t off; int n;
    chunk_of(table, chunks, d, off, n);
    const bool bf = d->grad_dtype == UG_DT_BF16;
    const int es = bf ? 2 : 4;
    const void* g = (const char*)d->grad + off * es;
    const int h = body_start(&g, &es, 1, n);
    const int tid = threadIdx.x;
    float acc = 0.f;
    int i = h + tid * 8;
    for (; i + 8 <= n; i += OPT_THREADS * 8) {
        float f[8];
        ld_grad8(g, i, bf, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += f[j] * f[j];
    }
    const int tail = h + (n - h) / 8 * 8;
    for (int k = tid; k < h; k += OPT_THREADS) { const float x = ld_grad1(g, k, bf); acc += x * x; }
    for (int k = tail + tid; k < n; k += OPT_THREADS) { const float x = ld_grad1(g, k, bf); acc += x * x; }
    acc = wave_sum(acc);
    __shared__ double wsum[OPT_THREADS / UG_WAVE];
    if ((tid & 63) == 0) wsum[tid >> 6] = (double)acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < OPT_THREADS / UG_WAVE; ++w) s += wsum[w];
        partial[blockIdx.x] = s;
    }
}

// ---- the partials in a fixed order (fp64) -> norm_coef[0] = total_norm, norm_coef[1] = clip_coef -----------------------------------------
__global__ __launch_bounds__(RED_THREADS) void sumsq_final_kernel(const double* __restrict__ partial, int64_t n, float max_norm, float* __restrict__ norm_coef) {
    __shared__ double s[RED_THREADS];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += RED_THREADS) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s[0]);
        // torch/nn/utils/clip_grad.py: clip_coef = max_norm / (total_norm + 1e-6) (Tensor.__rdiv__: reciprocal, then the product),
        // clamp(max=1.0): inf -> 0, NaN propagates
        const float coef = (1.0f / (norm + 1e-6f)) * max_norm;
        norm_coef[0] = norm;
        norm_coef[1] = coef > 1.0f ? 1.0f : coef;
    }
}

// ---- grad *= *coef -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void scale_kernel(const ug_optim_tensor* __restrict__ table, const int32_t* __restrict__ chunks,
                                                            const float* __restrict__ coef_p) {
    const ug_optim_tensor* d; int64_t off; int n;
    chunk_of(table, chunks, d, off, n);
    const float coef = *coef_p;
    const bool bf = d->grad_dtype == UG_DT_BF16;
    const int es = bf ? 2 : 4;
    void* g = (char*)d->grad + off * es;
    const void* gc = g;
    const int h = body_start(&gc, &es, 1, n);
    const int tid = threadIdx.x;
    for (int i = h + tid * 8; i + 8 <= n; i += OPT_THREADS * 8) {
        float f[8];
        ld_grad8(g, i, bf, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = f[j] * coef;
        if (bf) ElemT<bf16_t>::store8((bf16_t*)g + i, f);
        else ElemT<float>::store8((float*)g + i, f);
    }
    const int tail = h + (n - h) / 8 * 8;
    auto one = [&](int k) {
        const float x = ld_grad1(g, k, bf) * coef;
        if (bf) ((bf16_t*)g)[k] = f2bf(x);
        else ((float*)g)[k] = x;
    };
    for (int k = tid; k < h; k += OPT_THREADS) one(k);
    for (int k = tail + tid; k < n; k += OPT_THREADS) one(k);
}

// ---- AdamW ---------------------------------------------------------------------------------------------------------------------------------
// torch.optim.adam._single_tensor_adam with decoupled weight decay, in its order of operations (fp32, -ffp-contract=off, IEEE sqrt / div);
// torch divides a tensor by a Python scalar as a product with the scalar's fp32 reciprocal (ATen div_true_kernel_cuda), hence inv_bc2_sqrt
__device__ __forceinline__ void adamw1(float& p, float& m, float& v, float g, const ug_adamw_group& h) {
    p = p * h.decay;                                                                    // param.mul_(1 - lr * wd)
    m = h.lerp_w < 0.5f ? m + h.lerp_w * (g - m) : g - (g - m) * (1.0f - h.lerp_w);     // exp_avg.lerp_(grad, 1 - beta1)
    v = v * h.beta2 + h.one_minus_beta2 * g * g;                                        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) * h.inv_bc2_sqrt + h.eps;                              // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - h.step_size * (m / denom);                                                  // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// GBF: bf16 grads; MASTER: bf16 param + fp32 master (else the fp32 param is the master)
template <bool GBF, bool MASTER>
__device__ __forceinline__ void adamw_chunk(const ug_optim_tensor* d, int64_t off, int n, const ug_adamw_group& hp, float coef, bool scaled) {
    const void* g = (const char*)d->grad + off * (GBF ? 2 : 4);
    float* pm = (MASTER ? d->master : (float*)d->param) + off;
    bf16_t* pb = MASTER ? (bf16_t*)d->param + off : nullptr;
    float* m = d->exp_avg + off;
    float* v = d->exp_avg_sq + off;
    const void* ptrs[5] = {g, pm, m, v, pb};
    const int es[5] = {GBF ? 2 : 4, 4, 4, 4, 2};
    const int h = body_start(ptrs, es, MASTER ? 5 : 4, n);
    const int tid = threadIdx.x;
    for (int i = h + tid * 8; i + 8 <= n; i += OPT_THREADS * 8) {
        float gf[8], pf[8], mf[8], vf[8];
        ld_grad8(g, i, GBF, gf);
        ElemT<float>::load8(pm + i, pf);
        ElemT<float>::load8(m + i, mf);
        ElemT<float>::load8(v + i, vf);
#pragma unroll
        for (int j = 0; j < 8; ++j) adamw1(pf[j], mf[j], vf[j], scaled ? gf[j] * coef : gf[j], hp);
        ElemT<float>::store8(pm + i, pf);
        ElemT<float>::store8(m + i, mf);
        ElemT<float>::store8(v + i, vf);
        if (MASTER) ElemT<bf16_t>::store8(pb + i, pf);
    }
    const int tail = h + (n - h) / 8 * 8;
    auto one = [&](int k) {
        float p = pm[k], mm = m[k], vv = v[k];
        const float gg = ld_grad1(g, k, GBF);
        adamw1(p, mm, vv, scaled ? gg * coef : gg, hp);
        pm[k] = p; m[k] = mm; v[k] = vv;
        if (MASTER) pb[k] = f2bf(p);
    };
    for (int k = tid; k < h; k += OPT_THREADS) one(k);
    for (int k = tail + tid; k < n; k += OPT_THREADS) one(k);
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(const ug_optim_tensor* __restrict__ table, const int32_t* __restrict__ chunks,
                                                            const AdamwGroups groups, const float* __restrict__ coef_p) {
    const ug_optim_tensor* d; int64_t off; int n;
    chunk_of(table, chunks, d, off, n);
    const ug_adamw_group hp = groups.g[d->group];
    const bool scaled = coef_p != nullptr;
    const float coef = scaled ? *coef_p : 1.0f;
    const bool gbf = d->grad_dtype == UG_DT_BF16, master = d->master != nullptr;
    if (gbf && master) adamw_chunk<true, true>(d, off, n, hp, coef, scaled);
    else if (gbf) adamw_chunk<true, false>(d, off, n, hp, coef, scaled);
    else if (master) adamw_chunk<false, true>(d, off, n, hp, coef, scaled);
    else adamw_chunk<false, false>(d, off, n, hp, coef, scaled);
}

// ---- AdamW with bf16 state and stochastic rounding (ug_adamw_step_lowp, ug_sr_round_bf16) ------------------------------------------------
// Philox4x32-10 (Salmon et al., Random123): counter (c0, c1, c2, c3), key (k0, k1), ten rounds, the key bumped between rounds. Stateless:
// a draw is a function of (seed, param_index, step, element index, word) and of nothing else (the layout is written out in unigen_hip.h).
__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (u32x4){c0, c1, c2, c3};
}

struct SrStream { uint32_t k0, k1, param_index, step; };

// the four words of the element pair j = e >> 1 of this stream
__device__ __forceinline__ u32x4 sr_words(const SrStream& s, int64_t j) {
    return philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), s.param_index, s.step, s.k0, s.k1);
}

// fp32 -> bf16 with the 16-bit draw r: finite values (u + r) >> 16 (sign-magnitude: symmetric about zero, a grid value never moves, up with
// probability (u & 0xffff) / 65536); Inf stays Inf, NaN becomes a quiet NaN
__device__ __forceinline__ bf16_t sr_bf16(float x, uint32_t r) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return (bf16_t)((u & 0x007fffffu) ? ((u >> 16) | 0x0040u) : (u >> 16));
    return (bf16_t)((u + r) >> 16);
}

// the 16-bit draws of the 8 elements e .. e + 7, words 0..2 -> r[word][t]. ODD = e & 1: the 8 elements then span five pairs, not four
template <bool ODD>
__device__ __forceinline__ void sr_draws8(const SrStream& s, int64_t e, uint32_t (*r)[8]) {
    constexpr int NP = ODD ? 5 : 4;
    u32x4 w[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) w[k] = sr_words(s, (e >> 1) + k);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int q = (t + (ODD ? 1 : 0)) >> 1, sh = 16 * ((t + (ODD ? 1 : 0)) & 1);
        r[0][t] = (w[q].x >> sh) & 0xffffu; r[1][t] = (w[q].y >> sh) & 0xffffu; r[2][t] = (w[q].z >> sh) & 0xffffu;
    }
}

__device__ __forceinline__ void st_sr8(bf16_t* p, const float* f, const uint32_t* r) {
    u32x4 v;
    v.x = sr_bf16(f[0], r[0]) | ((uint32_t)sr_bf16(f[1], r[1]) << 16); v.y = sr_bf16(f[2], r[2]) | ((uint32_t)sr_bf16(f[3], r[3]) << 16);
    v.z = sr_bf16(f[4], r[4]) | ((uint32_t)sr_bf16(f[5], r[5]) << 16); v.w = sr_bf16(f[6], r[6]) | ((uint32_t)sr_bf16(f[7], r[7]) << 16);
    *(u32x4*)p = v;
}

// a bf16 param in one of the three low-precision arrangements. GBF: bf16 grads; MASTER: fp32 master kept, the param its RNE (else the param is
// read as bf16 and written with the draw of word 0); SBF: bf16 moments, written with the draws of words 1 and 2 (else fp32 moments)
template <bool GBF, bool MASTER, bool SBF>
__device__ __forceinline__ void adamw_lp_chunk(const ug_optim_tensor_lp* d, int64_t off, int n, const ug_adamw_group& hp, const SrStream& rs, float coef,
                                               bool scaled) {
    typedef typename std::conditional<SBF, bf16_t, float>::type S;
    const void* g = (const char*)d->grad + off * (GBF ? 2 : 4);
    float* pm = MASTER ? d->master + off : nullptr;
    bf16_t* pb = (bf16_t*)d->param + off;
    S* m = (S*)d->exp_avg + off;
    S* v = (S*)d->exp_avg_sq + off;
    const void* ptrs[5] = {g, pb, m, v, pm};
    const int es[5] = {GBF ? 2 : 4, 2, (int)sizeof(S), (int)sizeof(S), 4};
    const int h = body_start(ptrs, es, MASTER ? 5 : 4, n);
    const int tid = threadIdx.x;
    const bool odd = (off + h) & 1;                        // parity of the element index at the head of every 8-element vector of this chunk
    for (int i = h + tid * 8; i + 8 <= n; i += OPT_THREADS * 8) {
        float gf[8], pf[8], mf[8], vf[8];
        uint32_t r[3][8];
        ld_grad8(g, i, GBF, gf);
        if (MASTER) ElemT<float>::load8(pm + i, pf);
        else ElemT<bf16_t>::load8(pb + i, pf);
        ElemT<S>::load8(m + i, mf);
        ElemT<S>::load8(v + i, vf);
        if (odd) sr_draws8<true>(rs, off + i, r);
        else sr_draws8<false>(rs, off + i, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) adamw1(pf[j], mf[j], vf[j], scaled ? gf[j] * coef : gf[j], hp);
        if (MASTER) { ElemT<float>::store8(pm + i, pf); ElemT<bf16_t>::store8(pb + i, pf); }
        else st_sr8(pb + i, pf, r[0]);
        if (SBF) { st_sr8((bf16_t*)m + i, mf, r[1]); st_sr8((bf16_t*)v + i, vf, r[2]); }
        else { ElemT<float>::store8((float*)m + i, mf); ElemT<float>::store8((float*)v + i, vf); }
    }
    const int tail = h + (n - h) / 8 * 8;
    auto one = [&](int k) {
        float p = MASTER ? pm[k] : bf2f(pb[k]), mm = ElemT<S>::ld(m + k), vv = ElemT<S>::ld(v + k);
        const float gg = ld_grad1(g, k, GBF);
        adamw1(p, mm, vv, scaled ? gg * coef : gg, hp);
        const int64_t e = off + k;
        const u32x4 w = sr_words(rs, e >> 1);
        const int sh = 16 * (int)(e & 1);
        if (MASTER) { pm[k] = p; pb[k] = f2bf(p); }
        else pb[k] = sr_bf16(p, (w.x >> sh) & 0xffffu);
        if (SBF) { ((bf16_t*)m)[k] = sr_bf16(mm, (w.y >> sh) & 0xffffu); ((bf16_t*)v)[k] = sr_bf16(vv, (w.z >> sh) & 0xffffu); }
        else { ((float*)m)[k] = mm; ((float*)v)[k] = vv; }
    };
    for (int k = tid; k < h; k += OPT_THREADS) one(k);
    for (int k = tail + tid; k < n; k += OPT_THREADS) one(k);
}

struct AdamwGroupsLp { ug_adamw_group_lp g[UG_ADAMW_MAX_GROUPS]; };

__global__ __launch_bounds__(OPT_THREADS) void adamw_lowp_kernel(const ug_optim_tensor_lp* __restrict__ table, const int32_t* __restrict__ chunks,
                                                                 const AdamwGroupsLp groups, const float* __restrict__ coef_p) {
    const int t = chunks[2 * (int64_t)blockIdx.x], c = chunks[2 * (int64_t)blockIdx.x + 1];
    const ug_optim_tensor_lp* d = table + t;
    const int64_t off = (int64_t)c * UG_OPTIM_CHUNK;
    const int64_t rem = d->numel - off;
    const int n = rem < UG_OPTIM_CHUNK ? (int)rem : UG_OPTIM_CHUNK;
    const ug_adamw_group_lp& gl = groups.g[d->group];
    const ug_adamw_group hp = {gl.decay, gl.lerp_w, gl.beta2, gl.one_minus_beta2, gl.eps, gl.step_size, gl.inv_bc2_sqrt, 0.f};
    const SrStream rs = {(uint32_t)gl.seed, (uint32_t)(gl.seed >> 32), d->param_index, gl.step};
    const bool scaled = coef_p != nullptr;
    const float coef = scaled ? *coef_p : 1.0f;
    const bool gbf = d->grad_dtype == UG_DT_BF16, master = d->master != nullptr, sbf = d->state_dtype == UG_DT_BF16;
    if (d->param_dtype == UG_DT_F32 || (master && !sbf)) {
        // an fp32 param, or a bf16 param with fp32 master and moments: today's arrangements through today's code, no draws
        const ug_optim_tensor o = {d->param, d->grad, d->master, (float*)d->exp_avg, (float*)d->exp_avg_sq, d->numel, d->param_dtype, d->grad_dtype, d->group, 0};
        if (gbf && master) adamw_chunk<true, true>(&o, off, n, hp, coef, scaled);
        else if (gbf) adamw_chunk<true, false>(&o, off, n, hp, coef, scaled);
        else if (master) adamw_chunk<false, true>(&o, off, n, hp, coef, scaled);
        else adamw_chunk<false, false>(&o, off, n, hp, coef, scaled);
    } else if (master) {
        if (gbf) adamw_lp_chunk<true, true, true>(d, off, n, hp, rs, coef, scaled);
        else adamw_lp_chunk<false, true, true>(d, off, n, hp, rs, coef, scaled);
    } else if (sbf) {
        if (gbf) adamw_lp_chunk<true, false, true>(d, off, n, hp, rs, coef, scaled);
        else adamw_lp_chunk<false, false, true>(d, off, n, hp, rs, coef, scaled);
    } else {
        if (gbf) adamw_lp_chunk<true, false, false>(d, off, n, hp, rs, coef, scaled);
        else adamw_lp_chunk<false, false, false>(d, off, n, hp, rs, coef, scaled);
    }
}

// out[i] = sr_bf16(x[i], draw `word` of element first_index + i): one block per UG_OPTIM_CHUNK elements
__global__ __launch_bounds__(OPT_THREADS) void sr_round_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int64_t total, int64_t first_index,
                                                               SrStream rs, int word) {
    const int64_t off = (int64_t)blockIdx.x * UG_OPTIM_CHUNK;
    const int64_t rem = total - off;
    const int n = rem < UG_OPTIM_CHUNK ? (int)rem : UG_OPTIM_CHUNK;
    x += off; out += off;
    const void* ptrs[2] = {x, out};
    const int es[2] = {4, 2};
    const int h = body_start(ptrs, es, 2, n);
    const int tid = threadIdx.x;
    const int64_t e0 = first_index + off;
    const bool odd = (e0 + h) & 1;
    for (int i = h + tid * 8; i + 8 <= n; i += OPT_THREADS * 8) {
        float f[8];
        uint32_t r[3][8];
        ElemT<float>::load8(x + i, f);
        if (odd) sr_draws8<true>(rs, e0 + i, r);
        else sr_draws8<false>(rs, e0 + i, r);
        uint32_t rw[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) rw[t] = word == 0 ? r[0][t] : word == 1 ? r[1][t] : r[2][t];
        st_sr8(out + i, f, rw);
    }
    const int tail = h + (n - h) / 8 * 8;
    auto one = [&](int k) {
        const int64_t e = e0 + k;
        const u32x4 w = sr_words(rs, e >> 1);
        const uint32_t ww = word == 0 ? w.x : word == 1 ? w.y : w.z;
        out[k] = sr_bf16(x[k], (ww >> (16 * (int)(e & 1))) & 0xffffu);
    };
    for (int k = tid; k < h; k += OPT_THREADS) one(k);
    for (int k = tail + tid; k < n; k += OPT_THREADS) one(k);
}

int check_list(const char* who, const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks) {
    UG_REQUIRE(table, UG_ERR_BAD_SHAPE, "%s: null table", who);
    UG_REQUIRE(n_tensors > 0 && n_chunks >= 0 && n_chunks < (1ll << 31), UG_ERR_BAD_SHAPE, "%s: bad tensor / chunk count", who);
    UG_REQUIRE(chunks || n_chunks == 0, UG_ERR_BAD_SHAPE, "%s: null chunk list", who);
    return UG_OK;
}

}  // namespace

extern "C" int ug_optim_check_table(const ug_optim_tensor* table_host, int32_t n_tensors, int32_t n_groups) {
    UG_REQUIRE(table_host, UG_ERR_BAD_SHAPE, "ug_optim_check_table: null table");
    UG_REQUIRE(n_tensors > 0, UG_ERR_BAD_SHAPE, "ug_optim_check_table: no tensors");
    UG_REQUIRE(n_groups >= 0 && n_groups <= UG_ADAMW_MAX_GROUPS, UG_ERR_UNSUPPORTED, "ug_optim_check_table: n_groups %d outside [0, %d]", n_groups,
               UG_ADAMW_MAX_GROUPS);
    for (int32_t i = 0; i < n_tensors; ++i) {
        const ug_optim_tensor& d = table_host[i];
        UG_REQUIRE(d.numel >= 0, UG_ERR_BAD_SHAPE, "ug_optim_check_table: tensor %d: numel < 0", i);
        UG_REQUIRE(d.numel / UG_OPTIM_CHUNK < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_optim_check_table: tensor %d: too many elements", i);
        UG_REQUIRE(d.grad_dtype == UG_DT_BF16 || d.grad_dtype == UG_DT_F32, UG_ERR_UNSUPPORTED, "ug_optim_check_table: tensor %d: unknown grad dtype %d", i,
                   d.grad_dtype);
        UG_REQUIRE(d.grad || d.numel == 0, UG_ERR_BAD_SHAPE, "ug_optim_check_table: tensor %d: null grad", i);
        if (n_groups == 0) continue;        // a gradient-only table (ug_grad_sumsq / ug_grad_scale)
        UG_REQUIRE(d.param_dtype == UG_DT_BF16 || d.param_dtype == UG_DT_F32, UG_ERR_UNSUPPORTED, "ug_optim_check_table: tensor %d: unknown param dtype %d", i,
                   d.param_dtype);
        UG_REQUIRE(d.group >= 0 && d.group < n_groups, UG_ERR_BAD_SHAPE, "ug_optim_check_table: tensor %d: group %d outside [0, %d)", i, d.group, n_groups);
        if (d.numel == 0) continue;
        UG_REQUIRE(d.param && d.exp_avg && d.exp_avg_sq, UG_ERR_BAD_SHAPE, "ug_optim_check_table: tensor %d: null param or moment", i);
        UG_REQUIRE((d.param_dtype == UG_DT_BF16) == (d.master != nullptr), UG_ERR_UNSUPPORTED,
                   "ug_optim_check_table: tensor %d: a bf16 param needs an fp32 master, an fp32 param has none", i);
        UG_REQUIRE(ug_aligned(d.exp_avg, 4) && ug_aligned(d.exp_avg_sq, 4) && (!d.master || ug_aligned(d.master, 4)) &&
                   ug_aligned(d.param, d.param_dtype == UG_DT_BF16 ? 2 : 4) && ug_aligned(d.grad, d.grad_dtype == UG_DT_BF16 ? 2 : 4),
                   UG_ERR_BAD_ALIGN, "ug_optim_check_table: tensor %d: misaligned element pointer", i);
    }
    return UG_OK;
}

extern "C" int64_t ug_grad_sumsq_workspace_bytes(int64_t n_chunks) { return (n_chunks > 0 ? n_chunks : 1) * (int64_t)sizeof(double); }

extern "C" int ug_grad_sumsq(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, float max_norm, float* norm_coef,
                             void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    if (int rc = check_list("ug_grad_sumsq", table, n_tensors, chunks, n_chunks)) return rc;
    UG_REQUIRE(norm_coef, UG_ERR_BAD_SHAPE, "ug_grad_sumsq: null norm_coef");
    UG_REQUIRE(workspace && workspace_bytes >= ug_grad_sumsq_workspace_bytes(n_chunks) && ug_aligned(workspace, 8), UG_ERR_BAD_SHAPE,
               "ug_grad_sumsq: workspace of ug_grad_sumsq_workspace_bytes() needed (8-byte aligned)");
    if (n_chunks > 0)
        hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, (double*)workspace);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, (const double*)workspace, n_chunks, max_norm, norm_coef);
    UG_CHECK_LAUNCH("ug_grad_sumsq");
    return UG_OK;
}

extern "C" int ug_grad_scale(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, const float* coef,
                             ug_stream_t stream) {
    if (int rc = check_list("ug_grad_scale", table, n_tensors, chunks, n_chunks)) return rc;
    UG_REQUIRE(coef, UG_ERR_BAD_SHAPE, "ug_grad_scale: null coef");
    if (n_chunks == 0) return UG_OK;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, coef);
    UG_CHECK_LAUNCH("ug_grad_scale");
    return UG_OK;
}

extern "C" int ug_adamw_step(const ug_optim_tensor* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, const ug_adamw_group* groups_host,
                             int32_t n_groups, const float* coef, ug_stream_t stream) {
    if (int rc = check_list("ug_adamw_step", table, n_tensors, chunks, n_chunks)) return rc;
    UG_REQUIRE(groups_host && n_groups > 0, UG_ERR_BAD_SHAPE, "ug_adamw_step: null group table");
    UG_REQUIRE(n_groups <= UG_ADAMW_MAX_GROUPS, UG_ERR_UNSUPPORTED, "ug_adamw_step: %d groups > UG_ADAMW_MAX_GROUPS (%d)", n_groups, UG_ADAMW_MAX_GROUPS);
    if (n_chunks == 0) return UG_OK;
    AdamwGroups g = {};
    for (int i = 0; i < n_groups; ++i) g.g[i] = groups_host[i];
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, g, coef);
    UG_CHECK_LAUNCH("ug_adamw_step");
    return UG_OK;
}

extern "C" int ug_optim_check_table_lowp(const ug_optim_tensor_lp* table_host, int32_t n_tensors, int32_t n_groups) {
    UG_REQUIRE(table_host, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: null table");
    UG_REQUIRE(n_tensors > 0, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: no tensors");
    UG_REQUIRE(n_groups > 0 && n_groups <= UG_ADAMW_MAX_GROUPS, UG_ERR_UNSUPPORTED, "ug_optim_check_table_lowp: n_groups %d outside [1, %d]", n_groups,
               UG_ADAMW_MAX_GROUPS);
    for (int32_t i = 0; i < n_tensors; ++i) {
        const ug_optim_tensor_lp& d = table_host[i];
        const bool pbf = d.param_dtype == UG_DT_BF16, gbf = d.grad_dtype == UG_DT_BF16, sbf = d.state_dtype == UG_DT_BF16;
        UG_REQUIRE(d.numel >= 0, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: tensor %d: numel < 0", i);
        UG_REQUIRE(d.numel / UG_OPTIM_CHUNK < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_optim_check_table_lowp: tensor %d: too many elements", i);
        UG_REQUIRE(gbf || d.grad_dtype == UG_DT_F32, UG_ERR_UNSUPPORTED, "ug_optim_check_table_lowp: tensor %d: unknown grad dtype %d", i, d.grad_dtype);
        UG_REQUIRE(pbf || d.param_dtype == UG_DT_F32, UG_ERR_UNSUPPORTED, "ug_optim_check_table_lowp: tensor %d: unknown param dtype %d", i, d.param_dtype);
        UG_REQUIRE(sbf || d.state_dtype == UG_DT_F32, UG_ERR_UNSUPPORTED, "ug_optim_check_table_lowp: tensor %d: unknown state dtype %d", i, d.state_dtype);
        UG_REQUIRE(d.group >= 0 && d.group < n_groups, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: tensor %d: group %d outside [0, %d)", i, d.group, n_groups);
        UG_REQUIRE(pbf || (!sbf && !d.master), UG_ERR_UNSUPPORTED,
                   "ug_optim_check_table_lowp: tensor %d: an fp32 param is updated in place with fp32 moments (no master, no bf16 state)", i);
        if (d.numel == 0) continue;
        UG_REQUIRE(d.grad, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: tensor %d: null grad", i);
        UG_REQUIRE(d.param && d.exp_avg && d.exp_avg_sq, UG_ERR_BAD_SHAPE, "ug_optim_check_table_lowp: tensor %d: null param or moment", i);
        UG_REQUIRE(ug_aligned(d.exp_avg, sbf ? 2 : 4) && ug_aligned(d.exp_avg_sq, sbf ? 2 : 4) && (!d.master || ug_aligned(d.master, 4)) &&
                   ug_aligned(d.param, pbf ? 2 : 4) && ug_aligned(d.grad, gbf ? 2 : 4),
                   UG_ERR_BAD_ALIGN, "ug_optim_check_table_lowp: tensor %d: misaligned element pointer", i);
    }
    return UG_OK;
}

extern "C" int ug_adamw_step_lowp(const ug_optim_tensor_lp* table, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks,
                                  const ug_adamw_group_lp* groups_host, int32_t n_groups, const float* coef, ug_stream_t stream) {
    UG_REQUIRE(table, UG_ERR_BAD_SHAPE, "ug_adamw_step_lowp: null table");
    UG_REQUIRE(n_tensors > 0 && n_chunks >= 0 && n_chunks < (1ll << 31), UG_ERR_BAD_SHAPE, "ug_adamw_step_lowp: bad tensor / chunk count");
    UG_REQUIRE(chunks || n_chunks == 0, UG_ERR_BAD_SHAPE, "ug_adamw_step_lowp: null chunk list");
    UG_REQUIRE(groups_host && n_groups > 0, UG_ERR_BAD_SHAPE, "ug_adamw_step_lowp: null group table");
    UG_REQUIRE(n_groups <= UG_ADAMW_MAX_GROUPS, UG_ERR_UNSUPPORTED, "ug_adamw_step_lowp: %d groups > UG_ADAMW_MAX_GROUPS (%d)", n_groups, UG_ADAMW_MAX_GROUPS);
    for (int i = 0; i < n_groups; ++i)
        UG_REQUIRE(groups_host[i].step >= 1, UG_ERR_BAD_SHAPE, "ug_adamw_step_lowp: group %d: step 0 (the count after this step's increment is >= 1)", i);
    if (n_chunks == 0) return UG_OK;
    AdamwGroupsLp g = {};
    for (int i = 0; i < n_groups; ++i) g.g[i] = groups_host[i];
    hipLaunchKernelGGL(adamw_lowp_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, table, chunks, g, coef);
    UG_CHECK_LAUNCH("ug_adamw_step_lowp");
    return UG_OK;
}

extern "C" int ug_sr_round_bf16(const float* x, void* out, int64_t n, int64_t first_index, uint64_t seed, uint32_t param_index, uint32_t step,
                                int32_t word, ug_stream_t stream) {
    UG_REQUIRE(n >= 0 && first_index >= 0, UG_ERR_BAD_SHAPE, "ug_sr_round_bf16: n or first_index < 0");
    UG_REQUIRE(word >= 0 && word <= 2, UG_ERR_UNSUPPORTED, "ug_sr_round_bf16: word %d outside [0, 2]", word);
    UG_REQUIRE(n / UG_OPTIM_CHUNK < (1ll << 31) - 1 && first_index <= INT64_MAX - n, UG_ERR_UNSUPPORTED, "ug_sr_round_bf16: too many elements");
    if (n == 0) return UG_OK;
    UG_REQUIRE(x && out, UG_ERR_BAD_SHAPE, "ug_sr_round_bf16: null x or out");
    UG_REQUIRE(ug_aligned(x, 4) && ug_aligned(out, 2), UG_ERR_BAD_ALIGN, "ug_sr_round_bf16: misaligned element pointer");
    const SrStream rs = {(uint32_t)seed, (uint32_t)(seed >> 32), param_index, step};
    const int64_t blocks = (n + UG_OPTIM_CHUNK - 1) / UG_OPTIM_CHUNK;
    hipLaunchKernelGGL(sr_round_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, x, (bf16_t*)out, n, first_index, rs, (int)word);
    UG_CHECK_LAUNCH("ug_sr_round_bf16");
    return UG_OK;
}
