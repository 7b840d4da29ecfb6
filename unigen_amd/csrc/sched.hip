// Scheduler steps that are more than one Euler update (ug_euler_step lives in elementwise.hip).
//   ug_dpm_step(_f32): one step of DPMSolverMultistepScheduler as Sana configures it (dpmsolver++, midpoint, order <= 2, flow prediction), with
//   classifier-free guidance in front and the next forward's input behind, in one launch of pointwise_kernel (pointwise.h).
#include "pointwise.h"

namespace {

// diffusers 0.32.2, DPMSolverMultistepScheduler.step on fp32 latents, as torch evaluates it: guidance `u + gs * (t - u)` on the predictions widened
// to fp32, convert_model_output `x0 = sample - sigma * p`, then dpm_solver_first_order_update `(sigma_t / sigma_s) * sample - (alpha_t * (exp(-h) - 1)) * x0`
// or multistep_dpm_solver_second_order_update (midpoint) `... - 0.5 * (alpha_t * (exp(-h) - 1)) * ((1 / r0) * (x0 - m1))`. The coefficients are 0-dim
// tensors there and floats here (a, b, rinv; the host forms them with the same fp32 ops), so every tensor op of the step is one fp32 multiply, add or
// subtract with one rounding. The operations are spelled __fmul_rn / __fadd_rn / __fsub_rn: those intrinsics are never contracted into an FMA, whatever
// -ffp-contract says, and an FMA would skip the product's rounding that each of torch's kernels makes - the result could differ from the unfused
// loop's in the last bit, and the step is defined bit for bit.
template <typename T, int ORDER> struct DpmStep {
    const T* u; const T* t; float gs; float* x; float* m1; T* mi; int32_t copies; float sigma, a, b, rinv; int64_t n;      // n in chunks of 8
    template <int W> __device__ __forceinline__ void at(int64_t i) const {
        static_assert(W == 8, "8 elements per thread: one 16-byte access of bf16, two of fp32");
        float p[8], q[8], xs[8], x0[8], m[8];
        pw_load<T, 8>(u + i, p);
        if (t) {                                         // uniform: NULL = no guidance
            pw_load<T, 8>(t + i, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = __fadd_rn(p[e], __fmul_rn(gs, __fsub_rn(q[e], p[e])));
        }
        pw_load<float, 8>(x + i, xs);
        if constexpr (ORDER == 2) pw_load<float, 8>(m1 + i, m);
        const float hb = __fmul_rn(0.5f, b);             // exact (a power of two), formed once as torch forms the 0-dim `0.5 * (alpha_t * (exp(-h) - 1))`
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x0[e] = __fsub_rn(xs[e], __fmul_rn(sigma, p[e]));
            float o = __fsub_rn(__fmul_rn(a, xs[e]), __fmul_rn(b, x0[e]));
            if constexpr (ORDER == 2) o = __fsub_rn(o, __fmul_rn(hb, __fmul_rn(rinv, __fsub_rn(x0[e], m[e]))));
            xs[e] = o;
        }
        // everything this thread reads has been read: x and m1 are updated in place, and model_in may be the buffer the predictions came from
        pw_store<float, 8>(m1 + i, x0);
        pw_store<float, 8>(x + i, xs);
        for (int32_t k = 0; k < copies; ++k) pw_store<T, 8>(mi + (int64_t)k * n * 8 + i, xs);
    }
};
template <typename T> using DpmStep1 = DpmStep<T, 1>;
template <typename T> using DpmStep2 = DpmStep<T, 2>;

template <typename T>
int dpm_step_impl(const void* pred_uncond, const void* pred_text, float guidance_scale, float* sample, float* x0_prev, void* model_in, int32_t copies,
                  int32_t order, float sigma, float a, float b, float rinv, int64_t n, ug_stream_t stream) {
    if (n == 0) return UG_OK;
    UG_REQUIRE(pred_uncond && sample && x0_prev, UG_ERR_BAD_SHAPE, "ug_dpm_step: pred_uncond, sample and x0_prev must not be NULL");
    UG_REQUIRE(order == 1 || order == 2, UG_ERR_UNSUPPORTED, "ug_dpm_step: order %d (1 or 2)", order);
    UG_REQUIRE(copies >= 0 && (copies == 0 || model_in), UG_ERR_BAD_SHAPE, "ug_dpm_step: copies = %d with model_in %s", copies, model_in ? "given" : "NULL");
    UG_REQUIRE(n > 0 && n % 8 == 0 && ug_aligned(pred_uncond, 16) && ug_aligned(pred_text, 16) && ug_aligned(sample, 16) && ug_aligned(x0_prev, 16) &&
               ug_aligned(model_in, 16), UG_ERR_BAD_ALIGN, "ug_dpm_step: n must be a multiple of 8 and pointers 16-byte aligned");
    UG_REQUIRE(n < (1ll << 40) && copies <= 65536, UG_ERR_UNSUPPORTED, "ug_dpm_step: too large");
    const unsigned grid = ug_grid1d(n / 8, 256, 2048);
    if (order == 1)
        return pointwise_launch<T, DpmStep1<T>, PwLoop::Chunks>("ug_dpm_step", grid, stream, (const T*)pred_uncond, (const T*)pred_text, guidance_scale, sample,
                                                                 x0_prev, (T*)model_in, copies, sigma, a, b, rinv, n / 8);
    return pointwise_launch<T, DpmStep2<T>, PwLoop::Chunks>("ug_dpm_step", grid, stream, (const T*)pred_uncond, (const T*)pred_text, guidance_scale, sample,
                                                             x0_prev, (T*)model_in, copies, sigma, a, b, rinv, n / 8);
}

}  // namespace

UG_TWINS(ug_dpm_step, dpm_step_impl,
         (const void* pred_uncond, const void* pred_text, float guidance_scale, float* sample, float* x0_prev, void* model_in, int32_t copies, int32_t order,
          float sigma, float a, float b, float rinv, int64_t n, ug_stream_t s),
         (pred_uncond, pred_text, guidance_scale, sample, x0_prev, model_in, copies, order, sigma, a, b, rinv, n, s))
