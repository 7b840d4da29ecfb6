// Optimizer step of the control-module training loop (reference train.py:652-662): gradient-norm clipping
// (accelerator.clip_grad_norm_, :658) and torch.optim.AdamW (:660) over every trainable tensor in one multi-tensor pass.
//   ug_grad_sumsq    squared L2 norm of all grads -> total_norm and clip_coef (two launches: per-chunk partials, one fixed-order fp64 sum)
//   ug_grad_scale    grad *= clip_coef in place (the stand-alone clip_grad_norm_)
//   ug_adamw_step    one fp32 pass per element with torch.optim.AdamW's single-tensor arithmetic, clipping optionally fused (grads only read)
// Work list: a device table of ug_optim_tensor descriptors and a host-built list of (tensor, chunk) pairs of UG_OPTIM_CHUNK elements, so
// one launch covers every tensor. Each block takes one chunk: 16-byte vector accesses on the body where every stream of the chunk is 16-byte
// aligned at a common element, scalar head and tail (views into the engine's packs may start mid-buffer). No atomics: reproducible bitwise.
#include "ug_common.h"

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
