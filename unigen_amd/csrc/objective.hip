// Flow-matching training objective (reference train.py:589-613 and :644-652): what sits between the data and the differentiable forward, and
// between the forward's prediction and the backward.
//   ug_flow_noise     per sample: sigma from a uniform draw and the scheduler's table, timestep, loss weight; per element:
//                     noisy = (1 - sigma) x + sigma noise and target = noise - x, written in [B, C, H, W] or in _pack_latents layout (one launch)
//   ug_flow_loss      loss_per_sample[b] = mean_i(w_b (pred - target)^2), loss = their mean: per-block fp32 partials, then a one-block launch
//                     that adds them in a fixed order
//   ug_flow_loss_bwd  grad = gout * 2 w_b (pred - target) / (n B), gout read from device memory (one launch)
// Every tensor is contiguous. A sample's elements are split into a scalar head up to the first element that is 16-byte aligned in every
// stream, a body of 8-element groups (16-byte accesses) and a scalar tail; unaligned base pointers make the whole sample scalar. No atomics:
// every sum has an order fixed by the shape alone, so a repeat run is bit-identical. bf16 form and fp32 twin come from the same templates.
#include "ug_common.h"

namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_WAVES = OBJ_THREADS / UG_WAVE;
constexpr int OBJ_MAX_BLOCKS = 1024;        // blocks per sample of the element-wise kernels (grid-stride beyond)
constexpr int LOSS_GROUPS_PER_BLOCK = OBJ_THREADS * 4;   // 8-element groups one block of the reduction takes (8192 elements)
constexpr int LOSS_MAX_BLOCKS = 256;        // blocks per sample of the reduction
constexpr int FIN_THREADS = 256;

// head / body split of sample b whose first element is element b * per of a 16-byte aligned buffer: [0, h) scalar, then groups of 8
__device__ __forceinline__ void split(int64_t b, int64_t per, bool vec, int64_t& h, int64_t& groups) {
    h = vec ? (8 - (b * per) % 8) % 8 : per;
    if (h > per) h = per;
    groups = (per - h) / 8;
}

// in-sample index of the [C, H, W] element that packed element i of [(H/2)(W/2), C, 2, 2] holds
__device__ __forceinline__ int64_t unpacked_index(int64_t i, int C, int H, int W) {
    const int dx = (int)(i & 1), dy = (int)((i >> 1) & 1);
    const int64_t r = i >> 2;
    const int c = (int)(r % C);
    const int64_t tok = r / C;
    const int w2 = W >> 1;
    const int ti = (int)(tok / w2), tj = (int)(tok - (int64_t)ti * w2);
    return ((int64_t)c * H + (2 * ti + dy)) * W + (2 * tj + dx);
}

struct FlowScalars { float sigma, one_minus, timestep, weight; };

// the per-sample scalars of train.py:594-603,630,644: every thread of the sample computes the same values from u[b]
template <typename T>
__device__ __forceinline__ FlowScalars flow_scalars(float u, const float* __restrict__ table, int Tn, int scheme) {
    int idx = (int)(u * (float)Tn);                        // (u * num_train_timesteps).long()
    idx = idx < Tn - 1 ? idx : Tn - 1;                     // u * T rounds up to T for u next to 1: the reference would index out of range
    idx = idx > 0 ? idx : 0;
    const float s32 = table[idx];
    FlowScalars r;
    r.timestep = (s32 * (float)Tn) / 1000.0f;              // scheduler.timesteps = sigmas * T, then timesteps / 1000 (:630)
    r.sigma = ElemT<T>::rnd(s32);                          // get_sigmas(..., dtype=latents.dtype)
    r.one_minus = ElemT<T>::rnd(1.0f - r.sigma);
    const float s = r.sigma;
    if (scheme == UG_FLOW_SIGMA_SQRT) r.weight = 1.0f / (s * s);
    else if (scheme == UG_FLOW_COSMAP) r.weight = 2.0f / (3.14159265358979323846f * (1.0f - 2.0f * s + 2.0f * s * s));
    else r.weight = 1.0f;
    return r;
}

// (1.0 - sigmas) * x + sigmas * noise with a rounding after every tensor op (none in the twin); noise - x
template <typename T>
__device__ __forceinline__ void flow_elem(const FlowScalars& f, float x, float z, float& noisy, float& target) {
    noisy = ElemT<T>::rnd(ElemT<T>::rnd(f.one_minus * x) + ElemT<T>::rnd(f.sigma * z));
    target = ElemT<T>::rnd(z - x);
}

template <typename T, bool PACK>
__global__ __launch_bounds__(OBJ_THREADS) void flow_noise_kernel(const T* __restrict__ x, const T* __restrict__ noise, const float* __restrict__ u,
                                                                 const float* __restrict__ table, int Tn, int scheme, int C, int H, int W, bool vec,
                                                                 T* __restrict__ noisy, T* __restrict__ target, float* __restrict__ sigma,
                                                                 float* __restrict__ timestep, float* __restrict__ weight) {
    const int64_t b = blockIdx.y;
    const int64_t per = (int64_t)C * H * W;
    const FlowScalars f = flow_scalars<T>(u[b], table, Tn, scheme);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sigma[b] = f.sigma;
        timestep[b] = f.timestep;
        weight[b] = f.weight;
    }
    const T* xs = x + b * per;
    const T* zs = noise + b * per;
    T* ns = noisy + b * per;
    T* ts = target + b * per;
    int64_t h, groups;
    split(b, per, vec, h, groups);
    for (int64_t g = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * OBJ_THREADS) {
        const int64_t i = h + g * 8;
        float xf[8], zf[8], nf[8], tf[8];
        if (PACK) {
            // h is a multiple of 4, so the group is four (dx = 0, 1) pairs, each contiguous in the source
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t s = unpacked_index(i + 2 * j, C, H, W);
                ElemT<T>::load2(xs + s, xf + 2 * j);
                ElemT<T>::load2(zs + s, zf + 2 * j);
            }
        } else {
            ElemT<T>::load8(xs + i, xf);
            ElemT<T>::load8(zs + i, zf);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) flow_elem<T>(f, xf[j], zf[j], nf[j], tf[j]);
        ElemT<T>::store8(ns + i, nf);
        ElemT<T>::store8(ts + i, tf);
    }
    if (blockIdx.x == 0) {
        const int64_t tail = h + groups * 8;
        auto one = [&](int64_t i) {
            const int64_t s = PACK ? unpacked_index(i, C, H, W) : i;
            float n_, t_;
            flow_elem<T>(f, ElemT<T>::ld(xs + s), ElemT<T>::ld(zs + s), n_, t_);
            ElemT<T>::st(ns + i, n_);
            ElemT<T>::st(ts + i, t_);
        };
        for (int64_t i = threadIdx.x; i < h; i += OBJ_THREADS) one(i);
        for (int64_t i = tail + threadIdx.x; i < per; i += OBJ_THREADS) one(i);
    }
}

// ---- loss: partial[b][k] = sum over block k's share of sample b of w_b (pred - target)^2 --------------------------------------------------
template <typename T>
__global__ __launch_bounds__(OBJ_THREADS) void flow_loss_partial_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                                        const float* __restrict__ weight, int64_t n, bool vec, float* __restrict__ partial) {
    const int64_t b = blockIdx.y;
    const float w = weight[b];
    const T* ps = pred + b * n;
    const T* ts = target + b * n;
    int64_t h, groups;
    split(b, n, vec, h, groups);
    float acc = 0.f;
    for (int64_t g = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * OBJ_THREADS) {
        float pf[8], tf[8];
        ElemT<T>::load8(ps + h + g * 8, pf);
        ElemT<T>::load8(ts + h + g * 8, tf);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = pf[j] - tf[j]; acc += w * (d * d); }
    }
    if (blockIdx.x == 0) {
        const int64_t tail = h + groups * 8;
        for (int64_t i = threadIdx.x; i < h; i += OBJ_THREADS) { const float d = ElemT<T>::ld(ps + i) - ElemT<T>::ld(ts + i); acc += w * (d * d); }
        for (int64_t i = tail + threadIdx.x; i < n; i += OBJ_THREADS) { const float d = ElemT<T>::ld(ps + i) - ElemT<T>::ld(ts + i); acc += w * (d * d); }
    }
    acc = wave_sum(acc);
    __shared__ float wsum[OBJ_WAVES];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int k = 0; k < OBJ_WAVES; ++k) s += wsum[k];
        partial[b * gridDim.x + blockIdx.x] = s;
    }
}

// ---- the partials of a sample in block order -> loss_per_sample[b] = sum / n; the samples in a fixed tree -> loss = sum / B -----------------
__global__ __launch_bounds__(FIN_THREADS) void flow_loss_final_kernel(const float* __restrict__ partial, int nblk, int64_t B, int64_t n,
                                                                      float* __restrict__ per_sample, float* __restrict__ loss) {
    __shared__ float s[FIN_THREADS];
    float acc = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += FIN_THREADS) {
        float t = 0.f;
        for (int k = 0; k < nblk; ++k) t += partial[b * nblk + k];
        t = t / (float)n;
        per_sample[b] = t;
        acc += t;
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = FIN_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = s[0] / (float)B;
}

// ---- backward: torch autograd's order of operations through mean(), mean(1), weighting * and ** 2 (a tensor divided by a Python scalar is a
// product with the scalar's fp32 reciprocal): grad = (((gout * 1/B) * 1/n) * w_b) * (2 (pred - target)), one rounding to the output dtype ------
template <typename T>
__global__ __launch_bounds__(OBJ_THREADS) void flow_loss_bwd_kernel(const T* __restrict__ pred, const T* __restrict__ target, const float* __restrict__ weight,
                                                                    const float* __restrict__ gout, int64_t B, int64_t n, bool vec, T* __restrict__ grad) {
    const int64_t b = blockIdx.y;
    const float c = (((*gout) * (1.0f / (float)B)) * (1.0f / (float)n)) * weight[b];
    const T* ps = pred + b * n;
    const T* ts = target + b * n;
    T* gs = grad + b * n;
    int64_t h, groups;
    split(b, n, vec, h, groups);
    for (int64_t g = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * OBJ_THREADS) {
        float pf[8], tf[8], gf[8];
        ElemT<T>::load8(ps + h + g * 8, pf);
        ElemT<T>::load8(ts + h + g * 8, tf);
#pragma unroll
        for (int j = 0; j < 8; ++j) gf[j] = c * (2.0f * (pf[j] - tf[j]));
        ElemT<T>::store8(gs + h + g * 8, gf);
    }
    if (blockIdx.x == 0) {
        const int64_t tail = h + groups * 8;
        auto one = [&](int64_t i) { ElemT<T>::st(gs + i, c * (2.0f * (ElemT<T>::ld(ps + i) - ElemT<T>::ld(ts + i)))); };
        for (int64_t i = threadIdx.x; i < h; i += OBJ_THREADS) one(i);
        for (int64_t i = tail + threadIdx.x; i < n; i += OBJ_THREADS) one(i);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
constexpr int64_t OBJ_MAX_BATCH = 65535;        // gridDim.y

unsigned elem_blocks(int64_t per) {
    const int64_t g = (per / 8 + OBJ_THREADS - 1) / OBJ_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > OBJ_MAX_BLOCKS ? OBJ_MAX_BLOCKS : g));
}

int loss_blocks(int64_t n) {
    const int64_t g = (n / 8 + LOSS_GROUPS_PER_BLOCK - 1) / LOSS_GROUPS_PER_BLOCK;
    return (int)(g < 1 ? 1 : (g > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : g));
}

template <typename T>
int flow_noise_impl(const char* who, const void* x, const void* noise, const float* u, const float* sigma_table, int64_t T_, int32_t scheme, int32_t pack,
                    int64_t B, int64_t C, int64_t H, int64_t W, void* noisy, void* target, float* sigma, float* timestep, float* weight,
                    ug_stream_t stream) {
    UG_REQUIRE(x && noise && u && sigma_table && noisy && target && sigma && timestep && weight, UG_ERR_BAD_SHAPE, "%s: null pointer", who);
    UG_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0, UG_ERR_BAD_SHAPE, "%s: need [B, C, H, W] with positive C, H, W", who);
    UG_REQUIRE(T_ > 0, UG_ERR_BAD_SHAPE, "%s: the sigma table needs T > 0 entries, got %lld", who, (long long)T_);
    UG_REQUIRE(T_ <= (1 << 24), UG_ERR_UNSUPPORTED, "%s: T = %lld > 2^24 (u * T is an fp32 product)", who, (long long)T_);
    UG_REQUIRE(scheme >= UG_FLOW_NONE && scheme <= UG_FLOW_MODE, UG_ERR_UNSUPPORTED, "%s: unknown weighting scheme %d", who, scheme);
    UG_REQUIRE(pack == 0 || pack == 1, UG_ERR_UNSUPPORTED, "%s: pack must be 0 or 1, got %d", who, pack);
    UG_REQUIRE(!pack || (H % 2 == 0 && W % 2 == 0), UG_ERR_BAD_SHAPE, "%s: pack = 1 needs even H and W, got %lld x %lld", who, (long long)H, (long long)W);
    UG_REQUIRE(B <= OBJ_MAX_BATCH && C < (1 << 20) && H < (1 << 20) && W < (1 << 20) && B * C * H * W < (1ll << 40), UG_ERR_UNSUPPORTED, "%s: too large", who);
    UG_REQUIRE(ug_aligned(x, sizeof(T)) && ug_aligned(noise, sizeof(T)) && ug_aligned(noisy, sizeof(T)) && ug_aligned(target, sizeof(T)) &&
               ug_aligned(u, 4) && ug_aligned(sigma_table, 4) && ug_aligned(sigma, 4) && ug_aligned(timestep, 4) && ug_aligned(weight, 4),
               UG_ERR_BAD_ALIGN, "%s: misaligned element pointer", who);
    if (B == 0) return UG_OK;
    const bool vec = ug_aligned(x, 16) && ug_aligned(noise, 16) && ug_aligned(noisy, 16) && ug_aligned(target, 16);
    const dim3 grid(elem_blocks(C * H * W), (unsigned)B);
    if (pack)
        hipLaunchKernelGGL((flow_noise_kernel<T, true>), grid, dim3(OBJ_THREADS), 0, (hipStream_t)stream, (const T*)x, (const T*)noise, u, sigma_table, (int)T_,
                           (int)scheme, (int)C, (int)H, (int)W, vec, (T*)noisy, (T*)target, sigma, timestep, weight);
    else
        hipLaunchKernelGGL((flow_noise_kernel<T, false>), grid, dim3(OBJ_THREADS), 0, (hipStream_t)stream, (const T*)x, (const T*)noise, u, sigma_table, (int)T_,
                           (int)scheme, (int)C, (int)H, (int)W, vec, (T*)noisy, (T*)target, sigma, timestep, weight);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

int check_loss_shape(const char* who, const void* pred, const void* target, const float* weight, int64_t B, int64_t n, size_t esz) {
    UG_REQUIRE(pred && target && weight, UG_ERR_BAD_SHAPE, "%s: null pointer", who);
    UG_REQUIRE(B > 0 && n > 0, UG_ERR_BAD_SHAPE, "%s: need [B, n] with B, n > 0, got %lld x %lld", who, (long long)B, (long long)n);
    UG_REQUIRE(B <= OBJ_MAX_BATCH && n < (1ll << 40) && B * n < (1ll << 40), UG_ERR_UNSUPPORTED, "%s: too large", who);
    UG_REQUIRE(ug_aligned(pred, esz) && ug_aligned(target, esz) && ug_aligned(weight, 4), UG_ERR_BAD_ALIGN, "%s: misaligned element pointer", who);
    return UG_OK;
}

template <typename T>
int flow_loss_impl(const char* who, const void* pred, const void* target, const float* weight, int64_t B, int64_t n, float* loss_per_sample, float* loss,
                   void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    if (int rc = check_loss_shape(who, pred, target, weight, B, n, sizeof(T))) return rc;
    UG_REQUIRE(loss_per_sample && loss, UG_ERR_BAD_SHAPE, "%s: null output", who);
    UG_REQUIRE(ug_aligned(loss_per_sample, 4) && ug_aligned(loss, 4), UG_ERR_BAD_ALIGN, "%s: misaligned output", who);
    UG_REQUIRE(workspace && workspace_bytes >= ug_flow_loss_workspace_bytes(B, n) && ug_aligned(workspace, 4), UG_ERR_BAD_SHAPE,
               "%s: workspace of ug_flow_loss_workspace_bytes() needed (4-byte aligned)", who);
    const int nblk = loss_blocks(n);
    const bool vec = ug_aligned(pred, 16) && ug_aligned(target, 16);
    hipLaunchKernelGGL(flow_loss_partial_kernel<T>, dim3((unsigned)nblk, (unsigned)B), dim3(OBJ_THREADS), 0, (hipStream_t)stream, (const T*)pred, (const T*)target,
                       weight, n, vec, (float*)workspace);
    hipLaunchKernelGGL(flow_loss_final_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, (const float*)workspace, nblk, B, n, loss_per_sample, loss);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

template <typename T>
int flow_loss_bwd_impl(const char* who, const void* pred, const void* target, const float* weight, const float* gout, int64_t B, int64_t n, void* grad,
                       ug_stream_t stream) {
    if (int rc = check_loss_shape(who, pred, target, weight, B, n, sizeof(T))) return rc;
    UG_REQUIRE(gout && grad, UG_ERR_BAD_SHAPE, "%s: null gout or grad", who);
    UG_REQUIRE(ug_aligned(gout, 4) && ug_aligned(grad, sizeof(T)), UG_ERR_BAD_ALIGN, "%s: misaligned gout or grad", who);
    const bool vec = ug_aligned(pred, 16) && ug_aligned(target, 16) && ug_aligned(grad, 16);
    hipLaunchKernelGGL(flow_loss_bwd_kernel<T>, dim3(elem_blocks(n), (unsigned)B), dim3(OBJ_THREADS), 0, (hipStream_t)stream, (const T*)pred, (const T*)target,
                       weight, gout, B, n, vec, (T*)grad);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

}  // namespace

UG_TWINS(ug_flow_noise, flow_noise_impl,
         (const void* x, const void* noise, const float* u, const float* sigma_table, int64_t T, int32_t scheme, int32_t pack, int64_t B, int64_t C, int64_t H, int64_t W,
          void* noisy, void* target, float* sigma, float* timestep, float* weight, ug_stream_t s),
         (__func__, x, noise, u, sigma_table, T, scheme, pack, B, C, H, W, noisy, target, sigma, timestep, weight, s))

extern "C" int64_t ug_flow_loss_workspace_bytes(int64_t B, int64_t n) { return (B > 0 ? B : 1) * (int64_t)loss_blocks(n > 0 ? n : 1) * (int64_t)sizeof(float); }

UG_TWINS(ug_flow_loss, flow_loss_impl,
         (const void* pred, const void* target, const float* weight, int64_t B, int64_t n, float* loss_per_sample, float* loss, void* workspace, int64_t workspace_bytes,
          ug_stream_t s),
         (__func__, pred, target, weight, B, n, loss_per_sample, loss, workspace, workspace_bytes, s))
UG_TWINS(ug_flow_loss_bwd, flow_loss_bwd_impl,
         (const void* pred, const void* target, const float* weight, const float* gout, int64_t B, int64_t n, void* grad, ug_stream_t s),
         (__func__, pred, target, weight, gout, B, n, grad, s))
