// The one kernel of the contiguous pointwise ops: out[i] = f(in0[i], in1[i], ...) over n elements that lie back to back. The kernel is the
// traversal; an op is a struct whose fields are its operands, in the order of its entry point, and which applies itself at an element offset:
//     int64_t n;                                                    the op's length, its last field but for Relu's vec (see PwLoop for the unit)
//     template <int W> __device__ void at(int64_t i) const;         elements [i, i + W), W = 8 (one 16-byte access of bf16) or 1
// Ops: EulerStep, CfgCombine (elementwise.hip), DpmStep1 / DpmStep2 (sched.hip), GeluTanhBwd (backward.hip), Relu (depth.hip) and, as PwMap over an
// activation, GeluTanh (backward.hip), QuickGelu and GeluErf (text.hip), Silu (dcae.hip). Each keeps the loop that its own kernel had, as a compile-time parameter.
// Every entry point keeps its own argument checks: they differ in code and message.
#pragma once
#include "ug_common.h"

namespace {

enum class PwLoop {
    One,        // one 8-element chunk per thread, blocks of 256; n in chunks
    Chunks,     // grid-stride over chunks under the launcher's cap; n in chunks
    Elems       // grid-stride over elements, W per thread and trip; n in elements
};

// the kernel's arguments are the op's fields one by one, pointers __restrict__ as the kernels before this one had them: a thread reads its
// elements before it writes them, so an output may still be an input
template <typename F> struct PwArg { using type = F; };
template <typename P> struct PwArg<P*> { using type = P* __restrict__; };
template <typename T, typename Op, PwLoop LOOP, int W, typename... Field>
__global__ __launch_bounds__(LOOP == PwLoop::One ? 256 : 1024) void pointwise_kernel(typename PwArg<Field>::type... field) {
    const Op op = {field...};
    if constexpr (LOOP == PwLoop::One) {
        const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (c >= op.n) return;
        op.template at<W>(c * 8);
    } else if constexpr (LOOP == PwLoop::Chunks) {
        for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < op.n; c += (int64_t)gridDim.x * blockDim.x) op.template at<W>(c * 8);
    } else {
        for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W; i < op.n; i += (int64_t)gridDim.x * blockDim.x * W) op.template at<W>(i);
    }
}

// W elements at p <-> floats
template <typename T, int W> __device__ __forceinline__ void pw_load(const T* p, float* f) {
    if constexpr (W == 8) ElemT<T>::load8(p, f); else f[0] = ElemT<T>::ld(p);
}
template <typename T, int W> __device__ __forceinline__ void pw_store(T* p, const float* f) {
    if constexpr (W == 8) ElemT<T>::store8(p, f); else ElemT<T>::st(p, f[0]);
}

// y[i] = F::f(x[i]): the op of a plain activation F; y may be x
template <typename T, typename F> struct PwMap {
    const T* x; T* y; int64_t n;
    template <int W> __device__ __forceinline__ void at(int64_t i) const {
        float a[W], r[W];
        pw_load<T, W>(x + i, a);
#pragma unroll
        for (int k = 0; k < W; ++k) r[k] = F::f(a[k]);
        pw_store<T, W>(y + i, r);
    }
};

template <typename T, typename Op, PwLoop LOOP, int W = 8, typename... Field>
int pointwise_launch(const char* who, unsigned grid, ug_stream_t stream, Field... field) {
    hipLaunchKernelGGL((pointwise_kernel<T, Op, LOOP, W, Field...>), dim3(grid), dim3(256), 0, (hipStream_t)stream, field...);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

}  // namespace
