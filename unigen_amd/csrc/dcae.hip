// The passes over NHWC activations of diffusers' AutoencoderDC (DC-AE; unigen_amd/dcae.py) that are neither a convolution, a GEMM, the ReLU linear
// attention nor the GLU middle (those are ug_conv2d_nhwc, ug_gemm_bf16, ug_linear_attn and ug_glu_dwconv3x3):
//   ug_rmsnorm_bias_rows(_f32)                    RMSNorm with weight and bias over the channel row, then a residual add or a ReLU
//   ug_msconv_proj(_f32)                          SanaMultiscaleAttentionProjection: depthwise k x k, then a grouped 1x1 of 32 -> 32 channels on MFMA
//   ug_dc_shortcut_down / ug_dc_shortcut_up(_f32) the non-parametric shortcuts: pixel-unshuffle + group mean, channel repeat + pixel-shuffle, with the add
//   ug_silu(_f32)                                 SiLU on a contiguous tensor (the Silu op of pointwise_kernel, pointwise.h)
// All are bound by HBM at their byte counts. No atomics, no workspace, nothing kept between calls.
//
// ---- multiscale projection ----
// x [B][H][W] rows of G groups of 32 channels. One workgroup = 32 image columns x MS_ROWS image rows x NG groups, one wave per group. It walks down
// its rows as glu_dwconv3x3_kernel does: the 32 + 2 (K / 2) pixels of an input row go through registers into a ring of K + 1 rows in LDS (zeros outside
// the image: the convolution's zero padding), and an output row is computed when the K / 2 rows below it are in. The ring is laid out
// [row][group][octet][pixel][8] so that the lanes of a wave, one pixel each, read consecutive 16-byte items.
// Lane (pixel r = lane & 31, half h = lane >> 5) computes the depthwise sums of its pixel for the 16 channels 8 h + 16 s + j (s < 2, j < 8) of the
// wave's group: rounded, they ARE the lane's operand of two v_mfma_f32_32x32x16_bf16 (k = 8 h + j of step s) - `a` goes neither to LDS nor to HBM.
// The other operand is the group's 32 x 32 matrix, row o = lane & 31, the same channels. out^T[o][pixel] = sum_i w[o][i] a[pixel][i] leaves the pixel
// on the lane and four runs of four output channels in the registers: four 8-byte stores per lane. The fp32 twin keeps `a` in fp32 and runs the
// 32 k-steps on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains), channel 8 h + 16 s + j as k = h of step (s, j).
#include "pointwise.h"

namespace {

// ---- RMSNorm with weight and bias, + residual or ReLU ----
// `lpr` lanes per row, a power of two: a whole wave (64) from 264 channels on, else the smallest that holds the row's chunks of 8 channels, so that at
// DC-AE's 128 channels a wave normalises four rows and no lane idles. 256 / lpr rows per workgroup. The row (up to RB_MAXC x 64 chunks) is read
// once with 16-byte accesses and stays in registers for the statistic and the output. x, residual and out may be one another: a lane rewrites only
// what it has read.
constexpr int RB_MAXC = 9;                       // 4608 channels

template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_bias_rows_kernel(const T* x, int64_t ldx, const T* __restrict__ w, const T* __restrict__ bias, const T* residual,
                                                                int64_t ldr, T* out, int64_t ldo, int64_t rows, int C, float eps, int act, int lpr) {
    using E = ElemT<T>;
    const int sub = threadIdx.x & (lpr - 1);
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / lpr;
    const bool live = row < rows;              // the lanes of a dead row still take part in the shuffles (of their own group)
    const T* xr = x + row * ldx;
    const T* rr = residual ? residual + row * ldr : nullptr;
    T* orow = out + row * ldo;
    const int nch = live ? C / 8 : 0;
    float xv[RB_MAXC][8];
    float s = 0.f;
#pragma unroll
    for (int cc = 0; cc < RB_MAXC; ++cc) {
        const int ch = sub + lpr * cc;         // lpr < 64: nch <= lpr, only cc = 0 holds a chunk
        if (ch < nch) {
            E::load8(xr + 8 * ch, xv[cc]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += xv[cc][e] * xv[cc][e];
        }
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float rs = rsqrtf(s / (float)C + eps);
#pragma unroll
    for (int cc = 0; cc < RB_MAXC; ++cc) {
        const int ch = sub + lpr * cc;
        if (ch < nch) {
            float wv[8], bv[8], rv[8], y[8];
            E::load8(w + 8 * ch, wv);
            E::load8(bias + 8 * ch, bv);
            if (rr) E::load8(rr + 8 * ch, rv);     // read before the store
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                y[e] = (xv[cc][e] * rs) * wv[e] + bv[e];
                if (rr) y[e] = rv[e] + E::rnd(y[e]);
                else if (act) y[e] = y[e] < 0.f ? 0.f : y[e];          // NaN stays NaN, as torch.relu
            }
            E::store8(orow + 8 * ch, y);
        }
    }
}

template <typename T>
int rmsnorm_bias_rows_impl(const char* who, const void* x, int64_t ldx, const void* w, const void* bias, const void* residual, int64_t ldr, void* out,
                           int64_t ldo, int64_t rows, int64_t C, float eps, int32_t act, ug_stream_t stream) {
    if (rows == 0) return UG_OK;
    UG_REQUIRE(x && w && bias && out && rows > 0 && C > 0 && (act == 0 || act == 1), UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(C % 8 == 0 && C <= 8 * 64 * RB_MAXC, UG_ERR_UNSUPPORTED, "%s: C = %lld must be a multiple of 8, at most %d", who, (long long)C, 8 * 64 * RB_MAXC);
    UG_REQUIRE(!(residual && act), UG_ERR_UNSUPPORTED, "%s: a residual and an activation together", who);
    UG_REQUIRE(ldx >= C && ldo >= C && (!residual || ldr >= C), UG_ERR_BAD_SHAPE, "%s: leading dimensions below C", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ldx % per16 == 0 && ldo % per16 == 0 && ug_aligned(x, 16) && ug_aligned(out, 16) && ug_aligned(w, 16) && ug_aligned(bias, 16) &&
               (!residual || (ldr % per16 == 0 && ug_aligned(residual, 16))), UG_ERR_BAD_ALIGN, "%s: rows, weight and bias must be 16-byte aligned", who);
    int lpr = 1;
    while (lpr < 64 && lpr < C / 8) lpr *= 2;
    const int64_t nblk = ug_cdiv(rows, 256 / lpr);
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many rows", who);
    hipLaunchKernelGGL((rmsnorm_bias_rows_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w, (const T*)bias,
                       (const T*)residual, ldr, (T*)out, ldo, rows, (int)C, eps, (int)act, lpr);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

// ---- multiscale projection ----
constexpr int MS_W = 32;                         // image columns per workgroup: the MFMA's 32 columns
constexpr int MS_ROWS = 16;                      // image rows per workgroup
constexpr int MS_DH = 32;                        // channels per group

template <typename T, int NG, int K>
__global__ __launch_bounds__(64 * NG) void msconv_proj_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w_dw, const T* __restrict__ w_pw,
                                                            T* __restrict__ out, int64_t ldo, int H, int W, int G, int xtiles) {
    using E = ElemT<T>;
    constexpr int NT = 64 * NG, R = K / 2, PX = MS_W + 2 * R, SLOTS = K + 1;
    constexpr int ITEMS = PX * NG * 4;                     // 8-channel items of one ring row: pixel-major, then the octet across the groups
    constexpr int PER = (ITEMS + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) T ring[SLOTS][NG][4][PX][8];
    __shared__ __attribute__((aligned(16))) T wl[K * K][NG * 4][8];      // the taps of this workgroup's channels
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int xt = blockIdx.x % xtiles, yt = blockIdx.x / xtiles;
    const int b = blockIdx.z;
    const int x0 = xt * MS_W, y0 = yt * MS_ROWS;
    const int yend = min(H, y0 + MS_ROWS);
    const int g0 = blockIdx.y * NG;
    const int ng = min(NG, G - g0);                        // groups of this workgroup
    const int C = G * MS_DH;
    const T* xb = x + (int64_t)b * H * W * ldx + (int64_t)g0 * MS_DH;
    T* ob = out + (int64_t)b * H * W * ldo + (int64_t)(g0 + wave) * MS_DH;

    for (int it = tid; it < K * K * NG * 4; it += NT) {
        const int oc = it % (NG * 4), tap = it / (NG * 4);
        float wv[8];
        if (oc < ng * 4) E::load8(w_dw + (int64_t)tap * C + g0 * MS_DH + oc * 8, wv);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) wv[i] = 0.f;
        }
        E::store8(&wl[tap][oc][0], wv);                    // an exact copy: the values are T already
    }
    // the group's matrix as this lane's MFMA operand: row o = r, channels 8 h + 16 s + j
    float wp[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (wave < ng) E::load8(w_pw + ((int64_t)(g0 + wave) * MS_DH + r) * MS_DH + 8 * h + 16 * s, wp[s]);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) wp[s][i] = 0.f;
        }
    }

    float stage[PER][8];
    auto fetch = [&](int y) __attribute__((always_inline)) {       // row y of the image -> registers (zeros outside the image / the groups)
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int it = tid + p * NT;
            const int oc = it % (NG * 4), px = x0 - R + it / (NG * 4);
            if (it < ITEMS && y >= 0 && y < H && px >= 0 && px < W && oc < ng * 4) E::load8(xb + ((int64_t)y * W + px) * ldx + oc * 8, stage[p]);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) stage[p][i] = 0.f;
            }
        }
    };
    auto commit = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int it = tid + p * NT;
            if (it < ITEMS) {
                const int oc = it % (NG * 4);
                E::store8(&ring[slot][oc >> 2][oc & 3][it / (NG * 4)][0], stage[p]);
            }
        }
    };

    const bool live = wave < ng && x0 + r < W;
    const int nsteps = yend - y0 + 2 * R;                  // input rows y0 - R .. yend + R - 1
    fetch(y0 - R);
    for (int s = 0; s < nsteps; ++s) {
        commit(s % SLOTS);
        if (s + 1 < nsteps) fetch(y0 - R + s + 1);
        __syncthreads();                                   // one barrier per row: the slot written next (s + 1) is not among the K read below
        if (s < 2 * R) continue;
        if (wave >= ng) continue;                          // a wave without a group only loads
        const int yo = y0 + s - 2 * R;
        float acc[2][8];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[q][i] = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < K; ++ky) {                   // a row of taps at a time: unrolled over both loops the kernel holds 290 registers
            const int slot = (s - 2 * R + ky) % SLOTS;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float a[8], wv[8];
                    E::load8(&ring[slot][wave][h + 2 * q][r + kx][0], a);
                    E::load8(&wl[ky * K + kx][wave * 4 + h + 2 * q][0], wv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[q][i] = fmaf(a[i], wv[i], acc[q][i]);
                }
            }
        }
        f32x16 d;
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = 0.f;
        if constexpr (E::kF32) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) d = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[q][j], acc[q][j], d, 0, 0, 0);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4 wf = E::pack8(wp[q]), af = E::pack8(acc[q]);     // the weights are bf16 values already; a = rnd(dwconv)
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, af), d, 0, 0, 0);
            }
        }
        if (!live) continue;
        // d[i]: output channel 8 (i / 4) + 4 h + i % 4 of pixel r
        T* orow = ob + ((int64_t)yo * W + x0 + r) * ldo + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (E::kF32) *(f32x4*)(orow + 8 * q) = (f32x4){d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
            else *(u32x2*)(orow + 8 * q) = (u32x2){pack2bf(d[4 * q], d[4 * q + 1]), pack2bf(d[4 * q + 2], d[4 * q + 3])};
        }
    }
}

template <typename T>
int msconv_proj_impl(const char* who, const void* x, int64_t ldx, const void* w_dw, const void* w_pw, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                     int64_t G, int32_t k, ug_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return UG_OK;
    UG_REQUIRE(x && w_dw && w_pw && out && B > 0 && H > 0 && W > 0 && G > 0 && G < (1 << 20) && ldx >= G * MS_DH && ldo >= G * MS_DH, UG_ERR_BAD_SHAPE,
               "%s: bad arguments", who);
    UG_REQUIRE(k == 5 || k == 3, UG_ERR_UNSUPPORTED, "%s: kernel size %d (5 and 3 are built)", who, k);
    UG_REQUIRE(ldx % 8 == 0 && ldo % 8 == 0 && ug_aligned(x, 16) && ug_aligned(w_dw, 16) && ug_aligned(w_pw, 16) && ug_aligned(out, 16), UG_ERR_BAD_ALIGN,
               "%s: row strides must be multiples of 8 elements and bases 16-byte aligned", who);
    UG_REQUIRE(H < (1 << 20) && W < (1 << 20) && ldx < (1 << 24) && ldo < (1 << 24) && B < 65536, UG_ERR_UNSUPPORTED, "%s: too large", who);
    constexpr int NG = ElemT<T>::kF32 ? 2 : 4;
    const int xtiles = (int)((W + MS_W - 1) / MS_W);
    const int64_t tiles = (int64_t)xtiles * ((H + MS_ROWS - 1) / MS_ROWS);
    const int64_t ggroups = (G + NG - 1) / NG;
    UG_REQUIRE(tiles < (1ll << 31) && ggroups < 65536, UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    const dim3 grid((unsigned)tiles, (unsigned)ggroups, (unsigned)B);
    if (k == 5)
        hipLaunchKernelGGL((msconv_proj_kernel<T, NG, 5>), grid, dim3(64 * NG), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w_dw, (const T*)w_pw, (T*)out,
                           ldo, (int)H, (int)W, (int)G, xtiles);
    else
        hipLaunchKernelGGL((msconv_proj_kernel<T, NG, 3>), grid, dim3(64 * NG), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w_dw, (const T*)w_pw, (T*)out,
                           ldo, (int)H, (int)W, (int)G, xtiles);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

// ---- the non-parametric shortcuts ----
// One thread per 8 output channels of an output pixel: a 16-byte store (and a 16-byte load of x where x has the output's layout); h is gathered
// element by element, since consecutive output channels come from different pixels (down) or from one channel r times over (up).
// DOWN: output pixel (yo, xo) of [H / F][W / F]; u[m] = h[F yo + dy][F xo + dx][c] with m = c F^2 + dy F + dx; y[n] = mean_{j < g} u[n g + j].
// UP:   output pixel (Y, X) of [H F][W F], (dy, dx) = (Y % F, X % F); y[c] = h[Y / F][X / F][(c F^2 + dy F + dx) / rep].
// xs: x is still to be rearranged as h is - it has h's pixel grid and Cout / F^2 (down) or Cout F^2 (up) channels.
template <typename T, int F, bool UP>
__global__ __launch_bounds__(256) void dc_shortcut_kernel(const T* __restrict__ hsrc, int64_t ldh, const T* x, int64_t ldx, int xs, T* out, int64_t ldo,
                                                          int64_t npix, int H, int W, int Cin, int Cout, int gr) {
    using E = ElemT<T>;
    constexpr int F2 = F * F;
    const int oct = Cout / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * oct) return;
    const int n0 = (int)(i % oct) * 8;
    const int64_t pix = i / oct;                            // output pixel, batch included
    const int Wo = UP ? W * F : W / F, Ho = UP ? H * F : H / F;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho);
    const int64_t b = pix / ((int64_t)Wo * Ho);
    float y[8];
    if constexpr (UP) {
        const int dy = yo % F, dx = xo % F;
        const int64_t src = (b * H + yo / F) * W + xo / F;                  // the pixel of h (and of an x still to be shuffled)
        const T* hp = hsrc + src * ldh;
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = E::ld(hp + ((n0 + e) * F2 + dy * F + dx) / gr);
        if (x && xs) {
            const T* xp = x + src * ldx;
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = E::ld(xp + (n0 + e) * F2 + dy * F + dx) + y[e];
        }
    } else {
        const int64_t src = (b * H + (int64_t)yo * F) * W + (int64_t)xo * F; // the top-left pixel of the F x F patch
        const float cnt = (float)gr;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float s = 0.f;
            for (int j = 0; j < gr; ++j) {
                const int m = (n0 + e) * gr + j;
                const int c = m / F2, p = m % F2;
                s += E::ld(hsrc + (src + (int64_t)(p / F) * W + p % F) * ldh + c);
            }
            y[e] = E::rnd(s / cnt);                          // g = 1: the element itself
        }
        if (x && xs) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int m = n0 + e, c = m / F2, p = m % F2;
                y[e] = E::ld(x + (src + (int64_t)(p / F) * W + p % F) * ldx + c) + y[e];
            }
        }
    }
    if (x && !xs) {
        float xv[8];
        E::load8(x + pix * ldx + n0, xv);                   // read before the store: out may be x
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = xv[e] + y[e];
    }
    E::store8(out + pix * ldo + n0, y);
}

template <typename T, bool UP>
int dc_shortcut_impl(const char* who, const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H,
                     int64_t W, int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return UG_OK;
    UG_REQUIRE(h && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (x_shuffle == 0 || x_shuffle == 1), UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(factor == 1 || factor == 2, UG_ERR_UNSUPPORTED, "%s: factor %d (1 and 2 are built)", who, factor);
    UG_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, UG_ERR_UNSUPPORTED, "%s: Cin = %lld and Cout = %lld must be multiples of 8", who, (long long)Cin, (long long)Cout);
    const int64_t f2 = (int64_t)factor * factor;
    const int64_t num = UP ? Cout * f2 : Cin * f2, den = UP ? Cin : Cout;      // down: the group averaged into a channel; up: the repeats of a channel
    UG_REQUIRE(num % den == 0, UG_ERR_BAD_SHAPE, "%s: %lld x %lld channels do not divide into %lld", who, (long long)(UP ? Cout : Cin), (long long)f2,
               (long long)den);
    UG_REQUIRE(UP || (H % factor == 0 && W % factor == 0), UG_ERR_BAD_SHAPE, "%s: H = %lld, W = %lld are not multiples of the factor %d", who, (long long)H,
               (long long)W, factor);
    const int64_t xc = !x ? 0 : !x_shuffle ? Cout : UP ? Cout * f2 : Cout / f2;      // the channels of a row of x
    UG_REQUIRE(ldh >= Cin && ldo >= Cout && ldx >= xc, UG_ERR_BAD_SHAPE, "%s: leading dimensions below the channel counts", who);
    constexpr int per16 = 16 / (int)sizeof(T);
    UG_REQUIRE(ldh % per16 == 0 && ldo % per16 == 0 && ug_aligned(h, 16) && ug_aligned(out, 16) && (!x || (ldx % per16 == 0 && ug_aligned(x, 16))),
               UG_ERR_BAD_ALIGN, "%s: rows must be 16-byte aligned", who);
    UG_REQUIRE(H < (1 << 20) && W < (1 << 20) && Cin < (1 << 20) && Cout < (1 << 20) && ldh < (1 << 24) && ldx < (1 << 24) && ldo < (1 << 24) && B < 65536,
               UG_ERR_UNSUPPORTED, "%s: too large", who);
    const int64_t npix = UP ? B * H * W * f2 : B * (H / factor) * (W / factor);
    const int64_t nblk = ug_cdiv(npix * (Cout / 8), 256);
    UG_REQUIRE(nblk < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const T*)h, ldh, (const T*)x, ldx, (int)x_shuffle, (T*)out, ldo, npix,
                           (int)H, (int)W, (int)Cin, (int)Cout, (int)(num / den));
    };
    if (factor == 2) launch(dc_shortcut_kernel<T, 2, UP>);
    else launch(dc_shortcut_kernel<T, 1, UP>);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}
template <typename T> int dc_shortcut_down_impl(const char* who, const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t xs, void* out, int64_t ldo,
                                                int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream) {
    return dc_shortcut_impl<T, false>(who, h, ldh, x, ldx, xs, out, ldo, B, H, W, Cin, Cout, factor, stream);
}
template <typename T> int dc_shortcut_up_impl(const char* who, const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t xs, void* out, int64_t ldo,
                                              int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t factor, ug_stream_t stream) {
    return dc_shortcut_impl<T, true>(who, h, ldh, x, ldx, xs, out, ldo, B, H, W, Cin, Cout, factor, stream);
}

// ---- SiLU on a contiguous tensor (PwMap, pointwise.h): n a multiple of 8, one thread per 8 elements; y may alias x ----
template <typename T> struct Silu {
    static __device__ __forceinline__ float f(float a) { return silu<T>(a); }
};

template <typename T>
int silu_impl(const char* who, const void* x, void* y, int64_t n, ug_stream_t stream) {
    if (n == 0) return UG_OK;
    UG_REQUIRE(x && y && n > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(n % 8 == 0, UG_ERR_UNSUPPORTED, "%s: n = %lld must be a multiple of 8", who, (long long)n);
    UG_REQUIRE(ug_aligned(x, 16) && ug_aligned(y, 16), UG_ERR_BAD_ALIGN, "%s: tensors must be 16-byte aligned", who);
    UG_REQUIRE(ug_cdiv(n / 8, 256) < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: too many elements", who);
    return pointwise_launch<T, PwMap<T, Silu<T>>, PwLoop::One>(who, ug_grid1d(n / 8, 256), stream, (const T*)x, (T*)y, n / 8);
}

}  // namespace

UG_TWINS(ug_rmsnorm_bias_rows, rmsnorm_bias_rows_impl,
         (const void* x, int64_t ldx, const void* w, const void* bias, const void* residual, int64_t ldr, void* out, int64_t ldo, int64_t rows, int64_t C, float eps,
          int32_t act, ug_stream_t stream),
         (__func__, x, ldx, w, bias, residual, ldr, out, ldo, rows, C, eps, act, stream))
UG_TWINS(ug_msconv_proj, msconv_proj_impl,
         (const void* x, int64_t ldx, const void* w_dw, const void* w_pw, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t G, int32_t k,
          ug_stream_t stream),
         (__func__, x, ldx, w_dw, w_pw, out, ldo, B, H, W, G, k, stream))
UG_TWINS(ug_dc_shortcut_down, dc_shortcut_down_impl,
         (const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t Cin,
          int64_t Cout, int32_t factor, ug_stream_t stream),
         (__func__, h, ldh, x, ldx, x_shuffle, out, ldo, B, H, W, Cin, Cout, factor, stream))
UG_TWINS(ug_dc_shortcut_up, dc_shortcut_up_impl,
         (const void* h, int64_t ldh, const void* x, int64_t ldx, int32_t x_shuffle, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t Cin,
          int64_t Cout, int32_t factor, ug_stream_t stream),
         (__func__, h, ldh, x, ldx, x_shuffle, out, ldo, B, H, W, Cin, Cout, factor, stream))
UG_TWINS(ug_silu, silu_impl, (const void* x, void* y, int64_t n, ug_stream_t stream), (__func__, x, y, n, stream))
