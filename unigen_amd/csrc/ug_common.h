// Shared device/host helpers for libunigen_hip.so (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/unigen_hip.h"

typedef unsigned short bf16_t;  // raw bf16 bits
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define UG_WAVE 64

// ---- error plumbing (host) -------------------------------------------------------------
void ug_set_error(const char* fmt, ...);
#define UG_FAIL(code, ...) do { ug_set_error(__VA_ARGS__); return (code); } while (0)
#define UG_REQUIRE(cond, code, ...) do { if (!(cond)) UG_FAIL(code, __VA_ARGS__); } while (0)
#define UG_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) UG_FAIL(UG_ERR_HIP, "%s: launch failed: %s", name, hipGetErrorString(e_)); } while (0)

// integer switch from the environment: cached per call site name, re-read on every call when UG_ENV_DYNAMIC=1 (A/B tools). The PRODUCT library
// uses it only where a switch selects between two SHIPPED kernels that the dispatcher otherwise picks by shape (tests pin each of them):
// UG_GEMM_FORCE_TILE, UG_ADALN_FAST, UG_GN_FAST, UG_SOFTMAX_FAST, UG_CONV256 / UG_CONV256_MIN_TILES.
int ug_env_int(const char* name, int dflt);
// Tuning constants and measured-and-dropped kernel variants: compile-time constants in the product library (one kernel per dispatch decision);
// `python -m unigen_amd.build --probe` builds tools/probe/libunigen_hip_probe.so with -DUG_PROBE_BUILD, where they are environment switches
// again and the dropped variants (one-wave-per-SIMD GEMMs, cross-tile stream, lock-step / 4-wave / one-wave-per-SIMD attention, register-staged
// backward, ...) are compiled in for A/B measurements (tools/probe/README.md).
#ifdef UG_PROBE_BUILD
#define UG_TUNE(name, dflt) ug_env_int(name, dflt)
#else
#define UG_TUNE(name, dflt) (dflt)
#endif

// the bf16 entry point NAME and its fp32 verification twin NAME_f32 from one implementation template IMPL<T>: PARAMS is the parenthesised
// parameter list of both, ARGS the parenthesised arguments handed to IMPL
#define UG_TWINS(NAME, IMPL, PARAMS, ARGS)                                              \
    extern "C" int NAME PARAMS { return IMPL<bf16_t> ARGS; }                            \
    extern "C" int NAME##_f32 PARAMS { return IMPL<float> ARGS; }

static inline bool ug_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
static inline int64_t ug_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// blocks of a 1-D launch over n items, `per` to a block, at most `cap` of them: the cap is each caller's own (it decides how many trips a
// grid-stride loop makes); a kernel that makes one trip passes none and checks the count itself
constexpr int64_t UG_GRID_NOCAP = INT64_MAX;
static inline unsigned ug_grid1d(int64_t n, int64_t per, int64_t cap = UG_GRID_NOCAP) { const int64_t g = ug_cdiv(n, per); return (unsigned)(g < cap ? g : cap); }

// ---- strided attention views (host; unigen_hip.h "Strided attention views") -----------------------------------------------------------
// An attention operand as the entry points take it: base pointer, row stride and batch stride in elements. A plain buffer (workspace, state)
// is a view with both strides 0.
struct ug_view { const void* p; int64_t rs, bs; };
#define UG_VIEW(x) {x, x##_row_stride, x##_batch_stride}      // from an entry point's parameters x, x_row_stride, x_batch_stride
// one line of an entry point's table: both strides multiples of `mult` elements, the base aligned to `align` bytes (powers of two, both), and,
// where `bounded`, the row stride within (0, 2^24)
struct ug_view_rule { const char* name; ug_view v; int mult, align; bool bounded; };
// UG_ERR_BAD_ALIGN for the first view off its multiple or alignment; only when every view passed that, UG_ERR_UNSUPPORTED for the first bounded
// row stride out of range; else UG_OK. The last error starts with `who`, the entry point's name, and names the view.
int ug_check_views(const char* who, const ug_view_rule* rules, int n);
template <int N> static inline int ug_check_views(const char* who, const ug_view_rule (&rules)[N]) { return ug_check_views(who, rules, N); }
// verify_f32.hip: view rules, grid limit and launch of the one fp32 softmax-attention kernel, for ug_flash_attn_fwd_f32 (dh 64, 128), _fwd_bias_f32
// and _fwd_softcap_f32 (text.hip; 64 and 256) and _fwd_wide_f32 (attn_wide.hip; 512). What an entry adds to softmax(scale Q K^T) V, all zero = nothing:
struct ug_attn_f32_mods {
    const float* rel_table; int rel_len;      // dh 64: + rel_table[head][k - q + rel_len - 1]
    int causal;                               // dh 64: keys above the diagonal are masked (dh 256: always)
    float softcap; int window;                // dh 256: softcap * tanh(s / softcap); only the last `window` keys up to the diagonal
    const int32_t* kv_len; int group;         // dh 256: keys per sample (or NULL); query heads per K/V head
};
int ug_flash_attn_f32_launch(const char* who, ug_view q, ug_view k, ug_view v, ug_view o, int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh,
                             float softmax_scale, const ug_attn_f32_mods& mods, ug_stream_t stream);

// ---- bf16 <-> f32 (device) -------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float(((unsigned)u) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {  // RNE, NaN-preserving (v_cvt_pk_bf16_f32)
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }  // round through bf16
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2v;
    typedef __attribute__((ext_vector_type(2))) float f2v;
    f2v x = {lo, hi};
    bf2v y = __builtin_convertvector(x, bf2v);
    return __builtin_bit_cast(unsigned, y);
}
__device__ __forceinline__ float bflo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bfhi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// ---- element traits: one kernel source for the product path (bf16 storage, the reference's bf16 rounding points) and the
// fp32 VERIFICATION path (`*_f32` entry points: fp32 storage, no intermediate rounding). 8 elements per access in both. ------
template <typename T> struct ElemT;
// guarded forms of load8 / store8, in both specialisations: one 16-byte (bf16) / 2 x 16-byte (fp32) access where the caller found the address
// aligned (`vec`), eight element accesses otherwise
#define UG_ELEM_GUARDED8(T)                                                                                               \
    static __device__ __forceinline__ void load8(const T* p, float* f, bool vec) {                                        \
        if (vec) load8(p, f);                                                                                             \
        else { _Pragma("unroll") for (int j = 0; j < 8; ++j) f[j] = ld(p + j); }                                         \
    }                                                                                                                     \
    static __device__ __forceinline__ void store8(T* p, const float* f, bool vec) {                                       \
        if (vec) store8(p, f);                                                                                            \
        else { _Pragma("unroll") for (int j = 0; j < 8; ++j) st(p + j, f[j]); }                                          \
    }
template <> struct ElemT<bf16_t> {
    static constexpr bool kF32 = false;
    static __device__ __forceinline__ void unpack8(const u32x4 v, float* f) {         // the register forms: 8 bf16 in 4 registers <-> 8 floats
        f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
        f[4] = bflo(v.z); f[5] = bfhi(v.z); f[6] = bflo(v.w); f[7] = bfhi(v.w);
    }
    static __device__ __forceinline__ u32x4 pack8(const float* f) {
        u32x4 v;
        v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]); v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
        return v;
    }
    static __device__ __forceinline__ void load8(const bf16_t* p, float* f) { unpack8(*(const u32x4*)p, f); }
    static __device__ __forceinline__ void store8(bf16_t* p, const float* f) { *(u32x4*)p = pack8(f); }
    static __device__ __forceinline__ void zero8(bf16_t* p) { *(u32x4*)p = (u32x4){0u, 0u, 0u, 0u}; }
    static __device__ __forceinline__ void load2(const bf16_t* p, float* f) { const unsigned v = *(const unsigned*)p; f[0] = bflo(v); f[1] = bfhi(v); }
    static __device__ __forceinline__ void store2(bf16_t* p, const float* f) { *(unsigned*)p = pack2bf(f[0], f[1]); }
    static __device__ __forceinline__ float rnd(float x) { return rbf(x); }          // a bf16 tensor op's output
    static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
    static __device__ __forceinline__ void st(bf16_t* p, float x) { *p = f2bf(x); }
    UG_ELEM_GUARDED8(bf16_t)
};
template <> struct ElemT<float> {
    static constexpr bool kF32 = true;
    static __device__ __forceinline__ void load8(const float* p, float* f) {
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
        f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
    }
    static __device__ __forceinline__ void store8(float* p, const float* f) {
        *(f32x4*)p = (f32x4){f[0], f[1], f[2], f[3]};
        *(f32x4*)(p + 4) = (f32x4){f[4], f[5], f[6], f[7]};
    }
    static __device__ __forceinline__ void zero8(float* p) { *(f32x4*)p = (f32x4){0.f, 0.f, 0.f, 0.f}; *(f32x4*)(p + 4) = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void load2(const float* p, float* f) { const float2 v = *(const float2*)p; f[0] = v.x; f[1] = v.y; }
    static __device__ __forceinline__ void store2(float* p, const float* f) { *(float2*)p = make_float2(f[0], f[1]); }
    static __device__ __forceinline__ float rnd(float x) { return x; }
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float x) { *p = x; }
    UG_ELEM_GUARDED8(float)
};
#undef UG_ELEM_GUARDED8

// ---- activations (device): one copy each, so that a forward, its backward and the GEMM epilogue that share a formula share its bits ----------
// tanh GELU, fast form: 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3)  ==  x / (1 + exp(-2u)): 3 multiplies/FMAs, v_exp_f32, add,
// v_rcp_f32, multiply (the textbook form with an IEEE division is ~24 VALU instructions per element; the GEMM epilogue is VALU-bound). No
// cancellation for x << 0, exp -> inf gives rcp -> 0 -> -0. The GEMM epilogues (gemm_epilogue.h) and ug_gelu_tanh (backward.hip).
__device__ __forceinline__ float gelu_tanh(float x) {
    constexpr float C0 = -2.3022081986f;            // -2 sqrt(2/pi) log2(e)
    constexpr float C1 = C0 * 0.044715f;
    const float u = x * fmaf(x * x, C1, C0);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u));
}
// tanh GELU, exact form with tanhf: T5's gelu_new (text.hip) and the fp32 GEMM's epilogue (verify_f32.hip)
__device__ __forceinline__ float gelu_tanh_exact(float x) {
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    return 0.5f * x * (1.0f + tanhf(u));
}
// sigmoid and SiLU: rcp / exp2 on the bf16 path, IEEE division and expf on the fp32 verification path
template <typename T> __device__ __forceinline__ float sigmoid(float x) {
    if constexpr (ElemT<T>::kF32) return 1.0f / (1.0f + expf(-x));
    else return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
template <typename T> __device__ __forceinline__ float silu(float x) {
    if constexpr (ElemT<T>::kF32) return x / (1.0f + expf(-x));
    else return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}

// logical row -> physical row of a concatenated buffer (see unigen_hip.h "row map")
__device__ __forceinline__ int64_t ug_rowmap(int64_t m, int64_t rpb, int64_t bstride) {
    if (rpb <= 0) return m;
    int64_t b = m / rpb;
    return b * bstride + (m - b * rpb);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
