// Depth condition (unigen_amd/depth.py): the glue of transformers' DepthAnythingForDepthEstimation (DINOv2 backbone + DPT neck and head) that is
// neither a GEMM nor a convolution, and the depth-estimation pipeline's post-processing. The linears, norms, attention and convolutions are the
// library's existing entry points (ug_gemm_bf16, ug_layernorm_rows, ug_gelu_erf, ug_flash_attn_fwd, ug_conv2d_nhwc).
//   ug_img_u8_to_patches     DPTImageProcessor's rescale + normalize of a uint8 image, written as the rows of the patch-embedding GEMM
//   ug_relu                  nn.ReLU ahead of a convolution (the convolution gathers its input by LDS-DMA: no pre-activation rides in it)
//   ug_deconv_scatter_nhwc   second half of ConvTranspose2d(k = s = f): bias + pixel shuffle of the GEMM's fp32 product
//   ug_bilinear_nhwc         F.interpolate(mode="bilinear"), both align_corners values
//   ug_depth_head_out        activation1 + conv3 (1 channel) + activation2 + max_depth, fp32 out
//   ug_bicubic_f32           F.interpolate(mode="bicubic", align_corners=False) of the fp32 depth map
//   ug_minmax_to_u8          per-image (d - min) / (max - min) * 255 -> uint8, numpy's float32 order of operations
// Activations are NHWC; all kernels are bandwidth-bound on small tensors: a lane moves 8 channels (16 bytes of bf16) when the bases and leading
// dimensions allow it (`vec`, decided on the host) and single elements otherwise. -ffp-contract=off: every product and sum rounds on its own.
#include "pointwise.h"

// ---- uint8 NHWC -> patch rows [B * ph * pw][Kp]: column c P^2 + ky P + kx = ((float)(v * rescale) - mean[c]) / std[c] ------------------------------
// One workgroup per patch row, a lane makes 8 consecutive columns. The image bytes of a patch are read once each (3 P^2 of them per row).
struct PatchNorm { double rescale; float mean[3], std[3]; };
template <typename T>
__global__ __launch_bounds__(128) void u8_to_patches_kernel(const uint8_t* __restrict__ img, int64_t sb, int64_t sr, int C, int ph, int pw, int P, PatchNorm nm,
                                                            T* __restrict__ out, int64_t ldo, int Kp, int vec) {
    const int64_t row = blockIdx.x;
    const int px = (int)(row % pw), py = (int)((row / pw) % ph);
    const int64_t b = row / ((int64_t)pw * ph);
    const uint8_t* base = img + b * sb + (int64_t)py * P * sr + (int64_t)px * P * C;
    const int PP = P * P, K = 3 * PP;
    for (int c0 = threadIdx.x * 8; c0 < Kp; c0 += 128 * 8) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = c0 + j;
            float v = 0.0f;
            if (col < K) {
                const int ch = col / PP, r = col - ch * PP, ky = r / P, kx = r - ky * P;
                const unsigned byte = base[(int64_t)ky * sr + kx * C + (C == 3 ? ch : 0)];
                const float s = (float)((double)byte * nm.rescale);         // rescale(): float64 product, cast to float32
                v = (s - nm.mean[ch]) / nm.std[ch];                         // normalize(): float32 subtraction, float32 (IEEE) division
            }
            f[j] = v;
        }
        ElemT<T>::store8(out + row * ldo + c0, f, vec != 0);
    }
}

// ---- ReLU over n contiguous elements, 8 per lane: x < 0 ? +0 : x, so NaN and -0 pass through as in torch.relu (fmaxf would launder a NaN into 0) ----
template <typename T> struct Relu {
    const T* x; T* y; int64_t n; int vec;
    template <int W> __device__ __forceinline__ void at(int64_t i) const {
        static_assert(W == 8, "ug_relu moves whole chunks; a base off 16 bytes takes the guarded accesses");
        float f[8];
        ElemT<T>::load8(x + i, f, vec != 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = f[j] < 0.0f ? 0.0f : f[j];
        ElemT<T>::store8(y + i, f, vec != 0);
    }
};

// ---- ConvTranspose2d(k = s = f), second half: out[b][y f + ky][x f + kx][co] = rnd(prod[(b, y, x)][(ky f + kx) Cout + co] + bias[co]), pad = 0 ----
// A lane makes 8 channels of one output pixel.
template <typename T>
__global__ __launch_bounds__(256) void deconv_scatter_kernel(const float* __restrict__ prod, int64_t ldp, const T* __restrict__ bias, T* __restrict__ out, int64_t npix,
                                                             int h, int w, int f, int Cout, int Cp, int vec) {
    const int C8 = Cp >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * C8) return;
    const int64_t pix = i / C8;
    const int c0 = (int)(i - pix * C8) * 8;
    const int Wo = w * f, Ho = h * f;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const int64_t b = pix / ((int64_t)Wo * Ho);
    const int y = oy / f, ky = oy - y * f, x = ox / f, kx = ox - x * f;
    const float* p = prod + ((b * h + y) * w + x) * ldp + (int64_t)(ky * f + kx) * Cout + c0;
    float v[8];
    if (vec && c0 + 8 <= Cout) {
        const f32x4 a = *(const f32x4*)p, c = *(const f32x4*)(p + 4);
        float bv[8];
        ElemT<T>::load8(bias + c0, bv);
        v[0] = a[0] + bv[0]; v[1] = a[1] + bv[1]; v[2] = a[2] + bv[2]; v[3] = a[3] + bv[3];
        v[4] = c[0] + bv[4]; v[5] = c[1] + bv[5]; v[6] = c[2] + bv[6]; v[7] = c[3] + bv[7];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c0 + j < Cout ? p[j] + ElemT<T>::ld(bias + c0 + j) : 0.0f;
    }
    ElemT<T>::store8(out + pix * Cp + c0, v, vec != 0);
}

// ---- F.interpolate(mode="bilinear"): torch's area_pixel_compute_source_index in fp32, one rounding at the store ---------------------------------------
__device__ __forceinline__ void lin_src(int o, float scale, int align, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = align ? scale * (float)o : fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
    l0 = 1.0f - l1;
}
template <typename T>
__global__ __launch_bounds__(256) void bilinear_kernel(const T* __restrict__ x, int H, int W, int C, T* __restrict__ out, int64_t npix, int Ho, int Wo, float sh,
                                                       float sw, int align, int vec) {
    const int C8 = C >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * C8) return;
    const int64_t pix = i / C8;
    const int c0 = (int)(i - pix * C8) * 8;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const int64_t b = pix / ((int64_t)Wo * Ho);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    lin_src(oy, sh, align, H, y0, y1, hy0, hy1);
    lin_src(ox, sw, align, W, x0, x1, wx0, wx1);
    const T* base = x + b * H * W * C + c0;
    float a[8], bq[8], c[8], d[8], r[8];
    ElemT<T>::load8(base + ((int64_t)y0 * W + x0) * C, a, vec != 0);
    ElemT<T>::load8(base + ((int64_t)y0 * W + x1) * C, bq, vec != 0);
    ElemT<T>::load8(base + ((int64_t)y1 * W + x0) * C, c, vec != 0);
    ElemT<T>::load8(base + ((int64_t)y1 * W + x1) * C, d, vec != 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = hy0 * (wx0 * a[j] + wx1 * bq[j]) + hy1 * (wx0 * c[j] + wx1 * d[j]);
    ElemT<T>::store8(out + pix * C + c0, r, vec != 0);
}

// ---- head: out[pix] = act(rnd(bias + sum_c w[c] relu(x[pix][c]))) * max_depth, fp32. Four lanes share a pixel, 8 channels per lane and step -------------
template <typename T>
__global__ __launch_bounds__(256) void depth_head_out_kernel(const T* __restrict__ x, int64_t npix, int C, int Cp, const T* __restrict__ w, const T* __restrict__ bias,
                                                             float max_depth, int metric, float* __restrict__ out, int vec) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pix = t >> 2;
    const int sub = (int)(t & 3);
    float acc = 0.0f;
    if (pix < npix) {
        for (int c0 = sub * 8; c0 < C; c0 += 32) {
            float f[8], g[8];
            if (c0 + 8 <= C) { ElemT<T>::load8(x + pix * Cp + c0, f, vec != 0); ElemT<T>::load8(w + c0, g, vec != 0); }
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const bool ok = c0 + j < C; f[j] = ok ? ElemT<T>::ld(x + pix * Cp + c0 + j) : 0.0f; g[j] = ok ? ElemT<T>::ld(w + c0 + j) : 0.0f; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += g[j] * fmaxf(f[j], 0.0f);
        }
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (pix >= npix || sub != 0) return;
    const float v = ElemT<T>::rnd(acc + ElemT<T>::ld(bias));                     // conv3's output tensor
    const float a = metric ? ElemT<T>::rnd(1.0f / (1.0f + expf(-v))) : fmaxf(v, 0.0f);
    out[pix] = ElemT<T>::rnd(a * max_depth);
}

// ---- F.interpolate(mode="bicubic", align_corners=False) on fp32 [B][H][W]: A = -0.75, taps index-clamped (upsample_bicubic2d) -------------------------
__device__ __forceinline__ void cubic_coef(float t, float* c) {
    constexpr float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
__global__ __launch_bounds__(256) void bicubic_kernel(const float* __restrict__ x, int H, int W, float* __restrict__ out, int Ho, int Wo, float sh, float sw) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= Wo) return;
    const float ry = sh * ((float)oy + 0.5f) - 0.5f, rx = sw * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    float cy[4], cx[4];
    cubic_coef(ry - fy, cy);
    cubic_coef(rx - fx, cx);
    const float* img = x + (int64_t)blockIdx.z * H * W;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* row = img + (int64_t)min(max(iy - 1 + i, 0), H - 1) * W;
        float r = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) r += row[min(max(ix - 1 + j, 0), W - 1)] * cx[j];
        acc += r * cy[i];
    }
    out[((int64_t)blockIdx.z * Ho + oy) * Wo + ox] = acc;
}

// ---- per-image min / max in two deterministic stages, then uint8(trunc((d - min) / (max - min) * 255)) -------------------------------------------------
// Stage 1: workgroup j of image b reduces elements j 1024 + [0, 1024), strided by MM_BLOCKS 1024, to ws[b][j] = (min, max); every slot of the
// MM_BLOCKS is written (an idle workgroup writes (+inf, -inf)), so the workspace needs no initialisation. Stage 2: every workgroup reduces the
// MM_BLOCKS pairs of its image in the same order, then converts 1024 pixels.
constexpr int MM_BLOCKS = 64;
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[2 * wv] = lo; sm[2 * wv + 1] = hi; }
    __syncthreads();
    lo = fminf(fminf(sm[0], sm[2]), fminf(sm[4], sm[6]));
    hi = fmaxf(fmaxf(sm[1], sm[3]), fmaxf(sm[5], sm[7]));
}
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ d, int64_t HW, float* __restrict__ ws, int vec) {
    __shared__ float sm[8];
    const float* img = d + (int64_t)blockIdx.y * HW;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < HW; i += (int64_t)MM_BLOCKS * 1024) {
        if (vec) {                                                                // HW % 4 == 0: whole quads
            const f32x4 v = *(const f32x4*)(img + i);
            lo = fminf(fminf(lo, v[0]), fminf(fminf(v[1], v[2]), v[3]));
            hi = fmaxf(fmaxf(hi, v[0]), fmaxf(fmaxf(v[1], v[2]), v[3]));
        } else {
            for (int j = 0; j < 4 && i + j < HW; ++j) { lo = fminf(lo, img[i + j]); hi = fmaxf(hi, img[i + j]); }
        }
    }
    block_minmax(lo, hi, sm);
    if (threadIdx.x == 0) { float* p = ws + ((int64_t)blockIdx.y * MM_BLOCKS + blockIdx.x) * 2; p[0] = lo; p[1] = hi; }
}
__global__ __launch_bounds__(256) void minmax_to_u8_kernel(const float* __restrict__ d, int64_t HW, const float* __restrict__ ws, uint8_t* __restrict__ out, int ch,
                                                           int vec) {
    __shared__ float sm[8];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (threadIdx.x < MM_BLOCKS) { const float* p = ws + ((int64_t)blockIdx.y * MM_BLOCKS + threadIdx.x) * 2; lo = p[0]; hi = p[1]; }
    block_minmax(lo, hi, sm);
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= HW) return;
    const float range = hi - lo;
    const float* img = d + (int64_t)blockIdx.y * HW;
    uint8_t* o = out + ((int64_t)blockIdx.y * HW + i) * ch;
    unsigned q[4] = {0u, 0u, 0u, 0u};
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int n = (int)min((int64_t)4, HW - i);
    if (vec) { const f32x4 t = *(const f32x4*)(img + i); v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
    else
        for (int j = 0; j < n; ++j) v[j] = img[i + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = range > 0.0f ? (unsigned)(int)(((v[j] - lo) / range) * 255.0f) & 255u : 0u;      // a constant image: 0
    if (vec && ch == 1) *(unsigned*)o = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    else if (vec && ch == 3) {
        unsigned* o32 = (unsigned*)o;
        o32[0] = q[0] * 0x010101u | (q[1] << 24);
        o32[1] = q[1] * 0x0101u | (q[2] << 16) | (q[2] << 24);
        o32[2] = q[2] | (q[3] * 0x01010100u);
    } else {
        for (int j = 0; j < n; ++j)
            for (int c = 0; c < ch; ++c) o[j * ch + c] = (uint8_t)q[j];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
template <typename T>
static int img_u8_to_patches_impl(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t P, double rescale,
                                  const float* mean_host, const float* std_host, void* out, int64_t ld_out, int64_t Kp, ug_stream_t stream) {
    UG_REQUIRE(img && out && mean_host && std_host && (C == 1 || C == 3) && P >= 1 && P <= 64 && B >= 1 && H >= P && W >= P && H < 65536 && W < 65536 && H % P == 0 &&
                   W % P == 0 && rstride >= W * C && (B == 1 || bstride >= (H - 1) * rstride + W * C),
               UG_ERR_BAD_SHAPE, "ug_img_u8_to_patches: bad arguments (B=%lld H=%lld W=%lld C=%d P=%d; H and W are multiples of P, strides cover a row / a sample)",
               (long long)B, (long long)H, (long long)W, C, P);
    UG_REQUIRE(Kp >= 3 * P * P && Kp % 64 == 0 && ld_out >= Kp, UG_ERR_BAD_SHAPE, "ug_img_u8_to_patches: Kp=%lld must be a multiple of 64, >= 3 P^2 = %d and <= ld_out",
               (long long)Kp, 3 * P * P);
    UG_REQUIRE(std_host[0] != 0.0f && std_host[1] != 0.0f && std_host[2] != 0.0f, UG_ERR_BAD_SHAPE, "ug_img_u8_to_patches: a zero std");
    const int64_t rows = B * (H / P) * (W / P);
    UG_REQUIRE(rows < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_img_u8_to_patches: %lld patch rows", (long long)rows);
    PatchNorm nm;
    nm.rescale = rescale;
    for (int i = 0; i < 3; ++i) { nm.mean[i] = mean_host[i]; nm.std[i] = std_host[i]; }
    const int vec = ug_aligned(out, 16) && (ld_out * sizeof(T)) % 16 == 0;
    hipLaunchKernelGGL(u8_to_patches_kernel<T>, dim3((unsigned)rows), dim3(128), 0, (hipStream_t)stream, img, bstride, rstride, (int)C, (int)(H / P), (int)(W / P),
                       (int)P, nm, (T*)out, ld_out, (int)Kp, vec);
    UG_CHECK_LAUNCH("ug_img_u8_to_patches");
    return UG_OK;
}
UG_TWINS(ug_img_u8_to_patches, img_u8_to_patches_impl,
         (const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t P, double rescale, const float* mean_host,
          const float* std_host, void* out, int64_t ld_out, int64_t Kp, ug_stream_t stream),
         (img, bstride, rstride, B, H, W, C, P, rescale, mean_host, std_host, out, ld_out, Kp, stream))

template <typename T> static int relu_impl(const void* x, void* y, int64_t n, ug_stream_t stream) {
    UG_REQUIRE(x && y && n >= 0 && n % 8 == 0 && n / 8 < (1ll << 31) * 256, UG_ERR_BAD_SHAPE, "ug_relu: n=%lld must be a non-negative multiple of 8", (long long)n);
    if (n == 0) return UG_OK;
    const int vec = ug_aligned(x, 16) && ug_aligned(y, 16);
    return pointwise_launch<T, Relu<T>, PwLoop::One>("ug_relu", ug_grid1d(n / 8, 256), stream, (const T*)x, (T*)y, n / 8, vec);
}
UG_TWINS(ug_relu, relu_impl, (const void* x, void* y, int64_t n, ug_stream_t stream), (x, y, n, stream))

template <typename T>
static int deconv_scatter_impl(const float* prod, int64_t ld_prod, const void* bias, void* out, int64_t B, int64_t h, int64_t w, int32_t f, int64_t Cout, int64_t Cp,
                               ug_stream_t stream) {
    UG_REQUIRE(prod && bias && out && B >= 1 && h >= 1 && w >= 1 && f >= 1 && f <= 16 && Cout >= 1 && Cp >= Cout && Cp % 8 == 0 && ld_prod >= (int64_t)f * f * Cout &&
                   h * f < (1 << 24) && w * f < (1 << 24) && Cp < (1 << 24),
               UG_ERR_BAD_SHAPE, "ug_deconv_scatter_nhwc: bad arguments (B=%lld h=%lld w=%lld f=%d Cout=%lld Cp=%lld ld_prod=%lld; Cp a multiple of 8, ld_prod >= f f Cout)",
               (long long)B, (long long)h, (long long)w, f, (long long)Cout, (long long)Cp, (long long)ld_prod);
    const int64_t npix = B * h * f * w * f, n = npix * (Cp / 8);
    UG_REQUIRE(ug_cdiv(n, 256) < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_deconv_scatter_nhwc: too many elements");
    const int vec = ug_aligned(prod, 16) && ld_prod % 4 == 0 && Cout % 8 == 0 && ug_aligned(bias, 16) && ug_aligned(out, 16);
    hipLaunchKernelGGL(deconv_scatter_kernel<T>, dim3(ug_grid1d(n, 256)), dim3(256), 0, (hipStream_t)stream, prod, ld_prod, (const T*)bias, (T*)out, npix, (int)h, (int)w,
                       (int)f, (int)Cout, (int)Cp, vec);
    UG_CHECK_LAUNCH("ug_deconv_scatter_nhwc");
    return UG_OK;
}
UG_TWINS(ug_deconv_scatter_nhwc, deconv_scatter_impl,
         (const float* prod, int64_t ld_prod, const void* bias, void* out, int64_t B, int64_t h, int64_t w, int32_t f, int64_t Cout, int64_t Cp, ug_stream_t stream),
         (prod, ld_prod, bias, out, B, h, w, f, Cout, Cp, stream))

static float lin_scale(int64_t in, int64_t out, int align) {
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    return (float)in / (float)out;
}

template <typename T>
static int bilinear_impl(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* out, int64_t Ho, int64_t Wo, int32_t align_corners, ug_stream_t stream) {
    UG_REQUIRE(x && out && B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && C >= 8 && C % 8 == 0 && H < (1 << 24) && W < (1 << 24) && Ho < (1 << 24) &&
                   Wo < (1 << 24) && C < (1 << 24),
               UG_ERR_BAD_SHAPE, "ug_bilinear_nhwc: bad arguments (B=%lld %lldx%lld -> %lldx%lld C=%lld; C a multiple of 8)", (long long)B, (long long)H, (long long)W,
               (long long)Ho, (long long)Wo, (long long)C);
    const int64_t npix = B * Ho * Wo, n = npix * (C / 8);
    UG_REQUIRE(ug_cdiv(n, 256) < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_bilinear_nhwc: too many elements");
    const int vec = ug_aligned(x, 16) && ug_aligned(out, 16);
    hipLaunchKernelGGL(bilinear_kernel<T>, dim3(ug_grid1d(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (int)H, (int)W, (int)C, (T*)out, npix, (int)Ho, (int)Wo,
                       lin_scale(H, Ho, align_corners), lin_scale(W, Wo, align_corners), align_corners ? 1 : 0, vec);
    UG_CHECK_LAUNCH("ug_bilinear_nhwc");
    return UG_OK;
}
UG_TWINS(ug_bilinear_nhwc, bilinear_impl,
         (const void* x, int64_t B, int64_t H, int64_t W, int64_t C, void* out, int64_t Ho, int64_t Wo, int32_t align_corners, ug_stream_t stream),
         (x, B, H, W, C, out, Ho, Wo, align_corners, stream))

template <typename T>
static int depth_head_out_impl(const void* x, int64_t npix, int64_t C, int64_t Cp, const void* w, const void* bias, float max_depth, int32_t metric, float* out,
                               ug_stream_t stream) {
    UG_REQUIRE(x && w && bias && out && npix >= 1 && C >= 1 && Cp >= C && C < (1 << 24) && Cp < (1 << 24) && npix < (1ll << 37), UG_ERR_BAD_SHAPE,
               "ug_depth_head_out: bad arguments (pixels=%lld C=%lld Cp=%lld)", (long long)npix, (long long)C, (long long)Cp);
    const int vec = ug_aligned(x, 16) && ug_aligned(w, 16) && (Cp * sizeof(T)) % 16 == 0;
    hipLaunchKernelGGL(depth_head_out_kernel<T>, dim3(ug_grid1d(npix * 4, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, npix, (int)C, (int)Cp, (const T*)w,
                       (const T*)bias, max_depth, metric ? 1 : 0, out, vec);
    UG_CHECK_LAUNCH("ug_depth_head_out");
    return UG_OK;
}
UG_TWINS(ug_depth_head_out, depth_head_out_impl,
         (const void* x, int64_t npix, int64_t C, int64_t Cp, const void* w, const void* bias, float max_depth, int32_t metric, float* out, ug_stream_t stream),
         (x, npix, C, Cp, w, bias, max_depth, metric, out, stream))

extern "C" int ug_bicubic_f32(const float* x, int64_t B, int64_t H, int64_t W, float* out, int64_t Ho, int64_t Wo, ug_stream_t stream) {
    UG_REQUIRE(x && out && B >= 1 && B < 65536 && H >= 1 && W >= 1 && Ho >= 1 && Ho < 65536 && Wo >= 1 && H < (1 << 24) && W < (1 << 24) && Wo < (1 << 24),
               UG_ERR_BAD_SHAPE, "ug_bicubic_f32: bad arguments (B=%lld %lldx%lld -> %lldx%lld; B, Ho < 65536)", (long long)B, (long long)H, (long long)W, (long long)Ho,
               (long long)Wo);
    hipLaunchKernelGGL(bicubic_kernel, dim3(ug_grid1d(Wo, 256), (unsigned)Ho, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, (int)H, (int)W, out, (int)Ho, (int)Wo,
                       lin_scale(H, Ho, 0), lin_scale(W, Wo, 0));
    UG_CHECK_LAUNCH("ug_bicubic_f32");
    return UG_OK;
}

extern "C" int64_t ug_minmax_workspace_bytes(int64_t B, int64_t HW) { return (B < 1 || HW < 1) ? 0 : B * MM_BLOCKS * 2 * (int64_t)sizeof(float); }

extern "C" int ug_minmax_to_u8(const float* d, int64_t B, int64_t HW, uint8_t* out, int32_t channels, void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    UG_REQUIRE(d && out && B >= 1 && B < 65536 && HW >= 1 && HW < (1ll << 40) && (channels == 1 || channels == 3), UG_ERR_BAD_SHAPE,
               "ug_minmax_to_u8: bad arguments (B=%lld HW=%lld channels=%d; channels is 1 or 3)", (long long)B, (long long)HW, channels);
    UG_REQUIRE(workspace && ug_aligned(workspace, 8) && workspace_bytes >= ug_minmax_workspace_bytes(B, HW), UG_ERR_BAD_SHAPE,
               "ug_minmax_to_u8: the workspace is smaller than ug_minmax_workspace_bytes or not 8-byte aligned");
    const int64_t nb = ug_cdiv(HW, 1024);
    UG_REQUIRE(nb < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_minmax_to_u8: too many pixels");
    const int vec = HW % 4 == 0 && ug_aligned(d, 16) && ug_aligned(out, 4);
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(MM_BLOCKS, (unsigned)B), dim3(256), 0, (hipStream_t)stream, d, HW, (float*)workspace, vec);
    UG_CHECK_LAUNCH("ug_minmax_to_u8");
    hipLaunchKernelGGL(minmax_to_u8_kernel, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, (hipStream_t)stream, d, HW, (const float*)workspace, out, (int)channels, vec);
    UG_CHECK_LAUNCH("ug_minmax_to_u8");
    return UG_OK;
}
