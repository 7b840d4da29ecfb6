// Image front end (unigen_amd/image.py, unigen_amd/condition.py): everything between a uint8 control image and the VAE, and between the VAE and a
// uint8 result. All integer or exactly specified fp32 arithmetic - every entry point has ONE right answer per element (docs/PARITY_TOLERANCES.md,
// "Image front end: exact").
//   ug_canny_grad / ug_canny_nms / ug_canny_hysteresis / ug_canny_u8    cv2.Canny(img, low, high) (L2gradient = false), in its three stages
//   ug_img_resize_u8      PIL Image.resize(..., LANCZOS) of 8-bit images from host-built fixed-point tables (ImagingResample, 8bpc)
//   ug_img_rgb_to_l       PIL convert("L")
//   ug_img_box_blur_u8    PIL ImageFilter.BoxBlur / GaussianBlur of 8-bit images from host-built fixed-point constants (BoxBlur.c)
//   ug_img_u8_to_chw      VaeImageProcessor.preprocess' pil_to_numpy + numpy_to_pt + normalize
//   ug_img_chw_to_u8      VaeImageProcessor.postprocess' denormalize + pt_to_numpy + numpy_to_pil
// Images are uint8 NHWC [B, H, W, C] with a byte stride per sample and per row (pixels of a row are contiguous). Byte kernels: memory- or latency-bound;
// every kernel moves 4 to 16 bytes per lane when the bases and strides allow it (`vec` arguments, decided on the host) and falls back to guarded
// byte accesses at ragged edges or with unaligned views. Sobel / NMS / hysteresis work on halo tiles in LDS. Rows and samples come from the grid
// (blockIdx.y / .z), so no kernel divides per element.
#include "ug_common.h"

typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned byte_of(const u32x4& v, int j) { return (v[j >> 2] >> (8 * (j & 3))) & 255u; }

// 4 bytes of a row at byte offset g (may start before 0 or end past row_bytes: those bytes read as `fill`), one dword load when allowed
__device__ __forceinline__ unsigned load4_guarded(const uint8_t* row, int64_t g, int64_t row_bytes, bool vec, unsigned fill) {
    if (vec && g >= 0 && g + 4 <= row_bytes) return *(const unsigned*)(row + g);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v |= ((g + j >= 0 && g + j < row_bytes) ? (unsigned)row[g + j] : fill) << (8 * j);
    return v;
}

// ---- Canny, stage 1: 3x3 Sobel (replicated borders), L1 magnitude, strongest channel -------------------------------------------------------
// One workgroup: a 64 x 16 pixel tile; its 66 x 18 halo tile goes to LDS as dwords (the tile's first byte is 4-byte aligned in a row: 64 C bytes
// per tile). A thread makes 4 consecutive pixels of one row from 6 column sums, and stores 8 + 8 + 16 bytes.
constexpr int CT_W = 64, CT_H = 16;
template <int C>
__global__ __launch_bounds__(256) void canny_grad_kernel(const uint8_t* __restrict__ img, int64_t sb, int64_t sr, int H, int W, int16_t* __restrict__ dx,
                                                         int16_t* __restrict__ dy, int32_t* __restrict__ mag, int vec_in, int vec_out) {
    constexpr int ND = (4 + (CT_W + 1) * C + 3) / 4;        // dwords per LDS row: byte 4 + c * C + ch holds column c in [-1, 64] of the tile
    __shared__ unsigned tile[(CT_H + 2) * ND];
    const int x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H, b = blockIdx.z;
    const uint8_t* base = img + (int64_t)b * sb;
    const int64_t row_bytes = (int64_t)W * C;
    for (int idx = threadIdx.x; idx < (CT_H + 2) * ND; idx += 256) {
        const int r = idx / ND, d = idx - r * ND;
        const int gy = clampi(y0 - 1 + r, 0, H - 1);                          // replicated rows
        tile[idx] = load4_guarded(base + (int64_t)gy * sr, (int64_t)x0 * C - 4 + 4 * d, row_bytes, vec_in != 0, 0u);
    }
    __syncthreads();
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int y = y0 + ty, x = x0 + 4 * tx;
    if (y >= H || x >= W) return;
    const uint8_t* t8 = (const uint8_t*)tile;
    int bdx[4], bdy[4], bm[4];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        int s[6], d[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int c = clampi(x - 1 + j, 0, W - 1) - x0;                   // replicated columns; in [-1, 64]
            const int o = 4 + c * C + ch;
            const int a0 = t8[(ty + 0) * ND * 4 + o], a1 = t8[(ty + 1) * ND * 4 + o], a2 = t8[(ty + 2) * ND * 4 + o];
            s[j] = a0 + 2 * a1 + a2;
            d[j] = a2 - a0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gx = s[i + 2] - s[i], gy = d[i] + 2 * d[i + 1] + d[i + 2];
            const int m = abs(gx) + abs(gy);
            if (ch == 0 || m > bm[i]) { bdx[i] = gx; bdy[i] = gy; bm[i] = m; }   // strict >: the first channel wins a tie
        }
    }
    const int64_t o = ((int64_t)b * H + y) * W + x;
    if (vec_out && x + 3 < W) {
        *(i16x4*)(dx + o) = (i16x4){(short)bdx[0], (short)bdx[1], (short)bdx[2], (short)bdx[3]};
        *(i16x4*)(dy + o) = (i16x4){(short)bdy[0], (short)bdy[1], (short)bdy[2], (short)bdy[3]};
        *(i32x4*)(mag + o) = (i32x4){bm[0], bm[1], bm[2], bm[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) { dx[o + i] = (int16_t)bdx[i]; dy[o + i] = (int16_t)bdy[i]; mag[o + i] = bm[i]; }
    }
}

// ---- Canny, stage 2: non-maximum suppression + double threshold -> 2 strong, 0 candidate, 1 not an edge -------------------------------------
__global__ __launch_bounds__(256) void canny_nms_kernel(const int16_t* __restrict__ dx, const int16_t* __restrict__ dy, const int32_t* __restrict__ mag,
                                                        int H, int W, int low, int high, uint8_t* __restrict__ map, int vec) {
    constexpr int P = CT_W + 2;
    __shared__ int tile[(CT_H + 2) * P];
    const int x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H;
    const int64_t img0 = (int64_t)blockIdx.z * H * W;
    for (int idx = threadIdx.x; idx < (CT_H + 2) * P; idx += 256) {
        const int r = idx / P, c = idx - r * P;
        const int gy = y0 - 1 + r, gx = x0 - 1 + c;
        tile[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? mag[img0 + (int64_t)gy * W + gx] : 0;      // magnitudes outside the image are 0
    }
    __syncthreads();
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int y = y0 + ty, x = x0 + 4 * tx;
    if (y >= H || x >= W) return;
    const int64_t o = img0 + (int64_t)y * W + x;
    int xs[4], ys[4];
    if (vec && x + 3 < W) {
        const i16x4 a = *(const i16x4*)(dx + o), c = *(const i16x4*)(dy + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) { xs[i] = a[i]; ys[i] = c[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) { xs[i] = x + i < W ? dx[o + i] : 0; ys[i] = x + i < W ? dy[o + i] : 0; }
    }
    unsigned packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int* t = tile + (ty + 1) * P + 4 * tx + 1 + i;
        const int m = t[0];
        unsigned v = 1;
        if (m > low) {
            constexpr int TG22 = 13573;
            const int ax = abs(xs[i]), ay = abs(ys[i]) << 15;
            const int tg22x = ax * TG22;
            bool keep;
            if (ay < tg22x) keep = m > t[-1] && m >= t[1];
            else if (ay > tg22x + (ax << 16)) keep = m > t[-P] && m >= t[P];
            else {
                const int s = (xs[i] ^ ys[i]) < 0 ? -1 : 1;
                keep = m > t[-P - s] && m > t[P + s];
            }
            if (keep) v = m > high ? 2u : 0u;
        }
        packed |= v << (8 * i);
    }
    if (vec && x + 3 < W) *(unsigned*)(map + o) = packed;
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) map[o + i] = (uint8_t)(packed >> (8 * i));
    }
}

// ---- Canny, stage 3: hysteresis ---------------------------------------------------------------------------------------------------------------
// One sweep: every workgroup takes its 64 x 32 tile (plus a one-pixel halo read from the map as it stands) to a LOCAL fixed point in LDS and writes
// the pixels it promoted (0 -> 2) back, in place. No workgroup waits on another. The map only ever changes 0 -> 2, so a halo byte read while its
// owner promotes it is either value and both are sound; a workgroup that promoted a pixel on its tile's rim raises *flag, and the host launches
// another sweep while the flag is raised. A sweep that raises no flag saw stable halos everywhere, so every tile is at its fixed point given its
// neighbours: the global fixed point, which is unique (the set of candidates 8-connected to a strong pixel) whatever the order of promotions.
// Every flagged sweep promotes at least one pixel, so there are at most H * W + 1 sweeps (ug_canny_max_sweeps); the local loop promotes at least
// one of the tile's 2048 pixels per round, so it is bounded by 2049 rounds.
constexpr int HT_W = 64, HT_H = 32, HT_P = 72;      // LDS row: byte 4 + c holds column c in [-1, 64]
__global__ __launch_bounds__(256) void canny_hyst_sweep_kernel(uint8_t* __restrict__ map, int H, int W, int vec, int* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) uint8_t t[(HT_H + 2) * HT_P];
    const int x0 = blockIdx.x * HT_W, y0 = blockIdx.y * HT_H;
    uint8_t* m = map + (int64_t)blockIdx.z * H * W;
    int has0 = 0;
    for (int idx = threadIdx.x; idx < (HT_H + 2) * (HT_W / 4); idx += 256) {
        const int r = idx >> 4, d = idx & 15;
        const int gy = y0 - 1 + r, gx = x0 + 4 * d;
        unsigned v = 0x01010101u;                                                // outside the image: not an edge
        if (gy >= 0 && gy < H && gx < W) v = load4_guarded(m + (int64_t)gy * W, gx, W, vec != 0, 1u);
        *(unsigned*)(t + r * HT_P + 4 + 4 * d) = v;
        has0 |= ((v & 0xffu) == 0) | ((v & 0xff00u) == 0) | ((v & 0xff0000u) == 0) | ((v & 0xff000000u) == 0);
    }
    for (int idx = threadIdx.x; idx < (HT_H + 2) * 2; idx += 256) {
        const int r = idx >> 1, right = idx & 1;
        const int gy = y0 - 1 + r, gx = right ? x0 + HT_W : x0 - 1;
        t[r * HT_P + (right ? 4 + HT_W : 3)] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? m[(int64_t)gy * W + gx] : (uint8_t)1;
    }
    if (!__syncthreads_or(has0)) return;                                         // no candidate in sight: nothing to promote
    const int tr = threadIdx.x >> 3, tc = (threadIdx.x & 7) * 8;                 // this thread owns 8 consecutive pixels of tile row tr
    volatile uint8_t* p = t + (tr + 1) * HT_P + 4 + tc;
    unsigned promoted = 0;
    for (int round = 0; round < HT_W * HT_H + 1; ++round) {
        int changed = 0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {                                   // left to right, then right to left: a run along a row takes one round
#pragma unroll 1
            for (int k = 0; k < 8; ++k) {
                const int c = pass ? 7 - k : k;
                if (p[c] != 0) continue;
                const bool strong = p[c - 1] == 2 || p[c + 1] == 2 || p[c - HT_P - 1] == 2 || p[c - HT_P] == 2 || p[c - HT_P + 1] == 2 ||
                                    p[c + HT_P - 1] == 2 || p[c + HT_P] == 2 || p[c + HT_P + 1] == 2;
                if (strong) { p[c] = 2; promoted |= 1u << c; changed = 1; }
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (promoted) {
        const int gy = y0 + tr;                                                  // promoted pixels are inside the image: outside it the tile holds 1
        bool rim = tr == 0 || tr == HT_H - 1;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (promoted & (1u << c)) {
                m[(int64_t)gy * W + x0 + tc + c] = 2;
                rim |= (tc + c == 0) || (tc + c == HT_W - 1);
            }
        if (rim) *flag = 1;
    }
}

// out = 255 where the map holds 2, else 0; 16 pixels per lane
__global__ __launch_bounds__(256) void canny_final_kernel(const uint8_t* __restrict__ map, int H, int W, uint8_t* __restrict__ out, int64_t ob, int64_t orow,
                                                          int vec_in, int vec_out) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
    if (x >= W) return;
    const uint8_t* s = map + ((int64_t)blockIdx.z * H + blockIdx.y) * W + x;
    uint8_t* d = out + (int64_t)blockIdx.z * ob + (int64_t)blockIdx.y * orow + x;
    if (x + 16 <= W && vec_in && vec_out) {
        const u32x4 v = *(const u32x4*)s;
        u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = ((v[j] >> 1) & 0x01010101u) * 255u;   // bytes are 0, 1 or 2: bit 1 marks an edge
        *(u32x4*)d = r;
    } else {
        for (int j = 0; j < 16 && x + j < W; ++j) d[j] = s[j] == 2 ? 255 : 0;
    }
}

// ---- PIL resampling, horizontal pass: out[y][xo] = clip8((2^21 + sum_k in[y][xmin + k] * coef[xo][k]) >> 22) -------------------------------
// A workgroup makes 256 consecutive output pixels of one row. The input span they read (bounds are monotonic in xo) is staged in LDS with dword
// loads when it fits, and the results leave through LDS as dwords.
constexpr int RS_SPAN = 12288;       // bytes of LDS for the staged input span
template <int C>
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int Win, uint8_t* __restrict__ dst, int64_t db,
                                                       int64_t dr, int Wout, const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef, int K,
                                                       int vec_in, int vec_out) {
    __shared__ __attribute__((aligned(16))) uint8_t span[RS_SPAN];
    __shared__ __attribute__((aligned(16))) uint8_t res[256 * C];
    const int xo0 = blockIdx.x * 256, xo = xo0 + threadIdx.x;
    const uint8_t* row = src + (int64_t)blockIdx.z * sb + (int64_t)blockIdx.y * sr;
    uint8_t* orow = dst + (int64_t)blockIdx.z * db + (int64_t)blockIdx.y * dr;
    const int last = min(xo0 + 255, Wout - 1);
    const int p0 = clampi(bounds[2 * xo0], 0, Win - 1);
    const int p1 = clampi(clampi(bounds[2 * last], 0, Win - 1) + clampi(bounds[2 * last + 1], 0, K), p0, Win);     // one past the last pixel read
    const int64_t row_bytes = (int64_t)Win * C;
    const int a0 = (p0 * C) & ~3;                                            // the staged span starts on a dword of the row
    const int nd = (p1 * C - a0 + 3) >> 2;
    const bool staged = nd * 4 <= RS_SPAN;
    if (staged) {
        for (int d = threadIdx.x; d < nd; d += 256) *(unsigned*)(span + 4 * d) = load4_guarded(row, (int64_t)a0 + 4 * d, row_bytes, vec_in != 0, 0u);
        __syncthreads();
    }
    if (xo < Wout) {
        const int xmin = clampi(bounds[2 * xo], 0, Win - 1), n = clampi(bounds[2 * xo + 1], 0, K);
        const int32_t* k = coef + (int64_t)xo * K;
        int acc[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = 1 << 21;
        for (int i = 0; i < n; ++i) {
            const int w = k[i];
            const int p = min(xmin + i, Win - 1);
            // a window outside [p0, p1) cannot happen with monotonic tables; such a pixel is read from memory, never from outside the staged bytes
            const bool in_span = staged && p >= p0 && p < p1;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] += w * (int)(in_span ? span[p * C + ch - a0] : row[(int64_t)p * C + ch]);
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) res[threadIdx.x * C + ch] = (uint8_t)clampi(acc[ch] >> 22, 0, 255);
    }
    __syncthreads();
    const int nbytes = (last + 1 - xo0) * C;
    const int64_t ob = (int64_t)xo0 * C;                                      // 256 C: a dword boundary of the output row
    for (int d = threadIdx.x; 4 * d < nbytes; d += 256) {
        if (vec_out && 4 * d + 4 <= nbytes) *(unsigned*)(orow + ob + 4 * d) = *(const unsigned*)(res + 4 * d);
        else
            for (int j = 0; j < 4 && 4 * d + j < nbytes; ++j) orow[ob + 4 * d + j] = res[4 * d + j];
    }
}

// vertical pass: a row of W * C bytes is a byte vector; 16 bytes per lane, the window and its coefficients are uniform over the workgroup
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int Hin, int64_t row_bytes,
                                                       uint8_t* __restrict__ dst, int64_t db, int64_t dr, const int32_t* __restrict__ bounds,
                                                       const int32_t* __restrict__ coef, int K, int vec_in, int vec_out) {
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (g >= row_bytes) return;
    const int yo = blockIdx.y;
    const int ymin = clampi(bounds[2 * yo], 0, Hin - 1), n = clampi(bounds[2 * yo + 1], 0, K);
    const int32_t* k = coef + (int64_t)yo * K;
    const uint8_t* s = src + (int64_t)blockIdx.z * sb + g;
    uint8_t* d = dst + (int64_t)blockIdx.z * db + (int64_t)yo * dr + g;
    const bool full = g + 16 <= row_bytes;
    const int nb = full ? 16 : (int)(row_bytes - g);
    int acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 1 << 21;
    for (int i = 0; i < n; ++i) {
        const int w = k[i];
        const uint8_t* r = s + (int64_t)min(ymin + i, Hin - 1) * sr;
        if (full && vec_in) {
            const u32x4 v = *(const u32x4*)r;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += __mul24(w, (int)byte_of(v, j));      // |coefficient| < 2^23: one v_mad_i32_i24
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < nb) acc[j] += __mul24(w, (int)r[j]);
        }
    }
    if (full && vec_out) {
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            unsigned c = (unsigned)clampi(acc[j] >> 22, 0, 255);
            // keeps the compiler from fusing shift + clamp + pack of two neighbours into v_ashr_pk_u8_i32: the instruction writes 16 bits and the
            // upper half of its destination came out of an accumulator register unchanged (bytes 2 and 3 of the first dword were OR-ed with it)
            asm volatile("" : "+v"(c));
            o[j >> 2] |= c << (8 * (j & 3));
        }
        *(u32x4*)d = o;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < nb) d[j] = (uint8_t)clampi(acc[j] >> 22, 0, 255);
    }
}

// ---- PIL convert("L"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16; 16 pixels per lane (48 bytes in, 16 out) -------------------------------
__global__ __launch_bounds__(256) void rgb_to_l_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int W, uint8_t* __restrict__ dst, int64_t db,
                                                       int64_t dr, int vec_in, int vec_out) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
    if (x >= W) return;
    const uint8_t* s = src + (int64_t)blockIdx.z * sb + (int64_t)blockIdx.y * sr + (int64_t)x * 3;
    uint8_t* d = dst + (int64_t)blockIdx.z * db + (int64_t)blockIdx.y * dr + x;
    if (x + 16 <= W && vec_in && vec_out) {
        const u32x4 v[3] = {*(const u32x4*)s, *(const u32x4*)(s + 16), *(const u32x4*)(s + 32)};
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned r = byte_of(v[(3 * j) >> 4], (3 * j) & 15), g = byte_of(v[(3 * j + 1) >> 4], (3 * j + 1) & 15),
                           b = byte_of(v[(3 * j + 2) >> 4], (3 * j + 2) & 15);
            o[j >> 2] |= ((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16) << (8 * (j & 3));
        }
        *(u32x4*)d = o;
    } else {
        for (int j = 0; j < 16 && x + j < W; ++j)
            d[j] = (uint8_t)((19595u * s[3 * j] + 38470u * s[3 * j + 1] + 7471u * s[3 * j + 2] + 0x8000u) >> 16);
    }
}

// ---- uint8 NHWC -> fp32 / bf16 NCHW: v / 255.0f (an IEEE division), then 2.0f * . - 1.0f when normalising; every step rounded in fp32 --------
template <typename T, int C>
__global__ __launch_bounds__(256) void u8_to_chw_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int H, int W, T* __restrict__ dst, int Cout,
                                                        int normalize, int vec_in, int vec_out) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= W) return;
    const int y = blockIdx.y, b = blockIdx.z;
    const uint8_t* s = src + (int64_t)b * sb + (int64_t)y * sr + (int64_t)x * C;
    const bool full = x + 4 <= W;
    unsigned w[C];                                    // 4 pixels = C dwords
#pragma unroll
    for (int i = 0; i < C; ++i) w[i] = load4_guarded(s, 4 * i, (int64_t)(W - x) * C, vec_in != 0, 0u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= Cout) break;
        const int sc = C == 1 ? 0 : c;                // a gray image replicated to Cout channels
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = i * C + sc;
            const float v = (float)((w[o >> 2] >> (8 * (o & 3))) & 255u) / 255.0f;
            f[i] = normalize ? 2.0f * v - 1.0f : v;
        }
        T* d = dst + (((int64_t)b * Cout + c) * H + y) * W + x;
        if (full && vec_out) {
            if constexpr (ElemT<T>::kF32) *(f32x4*)d = (f32x4){f[0], f[1], f[2], f[3]};
            else *(u32x2*)d = (u32x2){pack2bf(f[0], f[1]), pack2bf(f[2], f[3])};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) ElemT<T>::st(d + i, f[i]);
        }
    }
}

// ---- fp32 / bf16 NCHW -> uint8 NHWC: x * 0.5 + 0.5 in the input's dtype (when denormalising), clamp to [0, 1], * 255.0f in fp32, round half to even ---------------
// A workgroup takes 1024 pixels of one row: per channel 16 bytes per lane along W, the bytes interleave in LDS and leave as 16-byte stores.
constexpr int CU_SEG = 1024;
template <typename T> __device__ __forceinline__ uint8_t denorm_u8(float x, int denormalize) {
    float t = x;
    if (denormalize) {
        t = x * 0.5f + 0.5f;                          // -ffp-contract=off: a product and a sum, each rounded (x * 0.5 is exact, so bf16 rounds once)
        t = ElemT<T>::rnd(t);
    }
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return (uint8_t)(int)__builtin_rintf(t * 255.0f);
}
template <typename T>
__global__ __launch_bounds__(256) void chw_to_u8_kernel(const T* __restrict__ src, int C, int H, int W, uint8_t* __restrict__ dst, int64_t db, int64_t dr,
                                                        int denormalize, int vec_in, int vec_out) {
    constexpr int EPL = 16 / (int)sizeof(T);          // elements per 16-byte load
    __shared__ __attribute__((aligned(16))) uint8_t t[CU_SEG * 4];
    const int x0 = blockIdx.x * CU_SEG, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(CU_SEG, W - x0);
    for (int c = 0; c < C; ++c) {
        const T* s = src + (((int64_t)b * C + c) * H + y) * W + x0;
        for (int i = threadIdx.x * EPL; i < npx; i += 256 * EPL) {
            if (vec_in && i + EPL <= npx) {
                float f[8];
                if constexpr (ElemT<T>::kF32) { const f32x4 v = *(const f32x4*)(s + i); f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; }
                else ElemT<T>::load8(s + i, f);
#pragma unroll
                for (int e = 0; e < EPL; ++e) t[(i + e) * C + c] = denorm_u8<T>(f[e], denormalize);
            } else {
                for (int e = 0; e < EPL && i + e < npx; ++e) t[(i + e) * C + c] = denorm_u8<T>(ElemT<T>::ld(s + i + e), denormalize);
            }
        }
    }
    __syncthreads();
    const int nbytes = npx * C;
    uint8_t* d = dst + (int64_t)b * db + (int64_t)y * dr + (int64_t)x0 * C;      // 1024 C: a 16-byte boundary of the output row
    for (int o = threadIdx.x * 16; o < nbytes; o += 256 * 16) {
        if (vec_out && o + 16 <= nbytes) *(u32x4*)(d + o) = *(const u32x4*)(t + o);
        else
            for (int j = 0; j < 16 && o + j < nbytes; ++j) d[o + j] = t[o + j];
    }
}

// ---- PIL BoxBlur / GaussianBlur (BoxBlur.c, 8-bit): passes of an extended box filter along rows, then along columns ------------------------------
// One pass along a line of `size` pixels, per channel, in uint32 (the weights sum to at most 2^24, so nothing overflows):
//   out[x] = (ww * sum_{i=-r..r} in[clamp(x+i)] + fw * (in[clamp(x-r-1)] + in[clamp(x+r+1)]) + 2^23) >> 24,   clamp(p) = min(max(p, 0), size-1)
// r, ww, fw come from the host (unigen_amd/image.py box_blur_constants). PIL slides one accumulator along the line; integer sums are associative, so
// the direct window gives the same bytes. The tile kernels hold a tile plus a halo of passes * (r + 1) pixels per side in LDS and run all `passes`
// of their axis there, ping-pong between two buffers; every pass clamps to the IMAGE, and pass p is computed on the tile widened by the
// (passes - 1 - p) * (r + 1) pixels the later passes still read. Four bytes are summed at a time as two pairs of 16-bit lanes (r <= 127).
constexpr int BL_BUF = 24576;                        // bytes per LDS buffer
constexpr int BL_HALF = 1 << 23;
constexpr int BH_TW = 256, BH_ROWS = 8;              // horizontal tile: 256 pixels of up to 8 rows
constexpr int BH_HALO_MAX = 128;
constexpr int BH_NDS_MAX = ((BH_TW + 2 * BH_HALO_MAX) * 3 + 12) / 4;      // staged dwords of a tile row at the largest halo, C = 3
constexpr int BV_WB = 128;                           // vertical tile: 128 bytes (32 dwords) of a row ...
constexpr int BV_ROWS = BL_BUF / BV_WB;              // ... times 192 rows, halo included
constexpr int BV_HALO_MAX = 48, BV_TH_MAX = 96;

__device__ __forceinline__ void blur_add4(unsigned& lo, unsigned& hi, unsigned v) { lo += v & 0x00ff00ffu; hi += (v >> 8) & 0x00ff00ffu; }
__device__ __forceinline__ unsigned blur_byte(unsigned sum, unsigned edge, unsigned ww, unsigned fw) { return (ww * sum + fw * edge + (unsigned)BL_HALF) >> 24; }
__device__ __forceinline__ unsigned blur_pack4(unsigned lo, unsigned hi, unsigned elo, unsigned ehi, unsigned ww, unsigned fw) {
    return blur_byte(lo & 0xffffu, elo & 0xffffu, ww, fw) | (blur_byte(hi & 0xffffu, ehi & 0xffffu, ww, fw) << 8) | (blur_byte(lo >> 16, elo >> 16, ww, fw) << 16) |
           (blur_byte(hi >> 16, ehi >> 16, ww, fw) << 24);
}
// 4 bytes of an LDS line at any byte offset q >= 0, from the two dwords around it (the line is padded by one dword)
__device__ __forceinline__ unsigned lds_u32_at(const uint8_t* line, int q) {
    const unsigned* p = (const unsigned*)(line + (q & ~3));
    return (unsigned)(((((uint64_t)p[1]) << 32) | p[0]) >> (8 * (q & 3)));
}
__device__ __forceinline__ void store4_guarded(uint8_t* row, int g, int row_bytes, bool vec, unsigned v) {
    if (vec && g + 4 <= row_bytes) *(unsigned*)(row + g) = v;
    else
        for (int k = 0; k < 4; ++k)
            if (g + k < row_bytes) row[g + k] = (uint8_t)(v >> (8 * k));
}

// along rows: LDS offset o of a tile row holds byte a0 + o of the image row, a0 a multiple of 4 at least 3 bytes before the halo; a thread makes one
// dword of a row per step. A dword whose whole window lies inside the image reads unaligned dwords C bytes apart; at the image's ends every byte
// clamps its own pixel index.
template <int C>
__global__ __launch_bounds__(256) void blur_h_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int H, int W, uint8_t* __restrict__ dst, int64_t db,
                                                     int64_t dr, int r, unsigned ww, unsigned fw, int passes, int nds, int vec_in, int vec_out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][BH_ROWS * 4 * (BH_NDS_MAX + 1)];
    const int pitch = 4 * (nds + 1);
    const int x0 = blockIdx.x * BH_TW, y0 = blockIdx.y * BH_ROWS, halo = passes * (r + 1), reach = (r + 1) * C;
    const int row_bytes = W * C, nrow = min(BH_ROWS, H - y0);
    const int a0 = ((x0 - halo) * C - 3) & ~3;
    const uint8_t* base = src + (int64_t)blockIdx.z * sb + (int64_t)y0 * sr;
    for (int idx = threadIdx.x; idx < nrow * nds; idx += 256) {
        const int row = idx / nds, d = idx - row * nds;
        *(unsigned*)(lds[0] + row * pitch + 4 * d) = load4_guarded(base + (int64_t)row * sr, (int64_t)a0 + 4 * d, row_bytes, vec_in != 0, 0u);
    }
    for (int p = 0; p < passes; ++p) {
        __syncthreads();
        const uint8_t* in = lds[p & 1];
        uint8_t* out = lds[(p & 1) ^ 1];
        const int hp = (passes - 1 - p) * (r + 1);
        const int o_lo = (max(x0 - hp, 0) * C - a0) & ~3, o_hi = (min(x0 + BH_TW + hp, W) * C - a0 + 3) & ~3;      // this pass' pixels, widened to dwords
        const int ndw = (o_hi - o_lo) >> 2;
        for (int idx = threadIdx.x; idx < nrow * ndw; idx += 256) {
            const int row = idx / ndw, o = o_lo + 4 * (idx - row * ndw), g = a0 + o;
            const uint8_t* line = in + row * pitch;
            unsigned res = 0;
            if (g - reach >= 0 && g + 3 + reach < row_bytes) {
                unsigned lo = 0, hi = 0, elo = 0, ehi = 0;
                for (int i = -r; i <= r; ++i) blur_add4(lo, hi, lds_u32_at(line, o + i * C));
                blur_add4(elo, ehi, lds_u32_at(line, o - reach));
                blur_add4(elo, ehi, lds_u32_at(line, o + reach));
                res = blur_pack4(lo, hi, elo, ehi, ww, fw);
            } else {
                for (int k = 0; k < 4; ++k) {
                    if (g + k < 0 || g + k >= row_bytes) continue;
                    const int x = (g + k) / C, ch = g + k - x * C - a0;
                    unsigned sum = 0;
                    for (int i = -r; i <= r; ++i) sum += line[clampi(x + i, 0, W - 1) * C + ch];
                    const unsigned edge = (unsigned)line[clampi(x - r - 1, 0, W - 1) * C + ch] + line[clampi(x + r + 1, 0, W - 1) * C + ch];
                    res |= blur_byte(sum, edge, ww, fw) << (8 * k);
                }
            }
            if (p + 1 < passes) *(unsigned*)(out + row * pitch + o) = res;
            else if (g < row_bytes) store4_guarded(dst + (int64_t)blockIdx.z * db + (int64_t)(y0 + row) * dr, g, row_bytes, vec_out != 0, res);
        }
    }
}

// along columns: a row of W * C bytes is a byte vector, the window is the same rows for every lane. LDS row j holds image row y0 - halo + j.
__global__ __launch_bounds__(256) void blur_v_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int H, int row_bytes, uint8_t* __restrict__ dst,
                                                     int64_t db, int64_t dr, int r, unsigned ww, unsigned fw, int passes, int th, int vec_in, int vec_out) {
    __shared__ __attribute__((aligned(16))) unsigned lds[2][BL_BUF / 4];
    constexpr int ND = BV_WB / 4;
    const int gx = blockIdx.x * BV_WB, y0 = blockIdx.y * th, halo = passes * (r + 1), ybase = y0 - halo;
    const int d = threadIdx.x & (ND - 1), g = gx + 4 * d;
    const bool live = g < row_bytes;                                               // a column past the row's end only keeps the barriers company
    const uint8_t* base = src + (int64_t)blockIdx.z * sb;
    const int ya = max(ybase, 0), yb = min(y0 + th + halo, H);
    for (int y = ya + (threadIdx.x >> 5); live && y < yb; y += 256 / ND) lds[0][(y - ybase) * ND + d] = load4_guarded(base + (int64_t)y * sr, g, row_bytes, vec_in != 0, 0u);
    for (int p = 0; p < passes; ++p) {
        __syncthreads();
        const unsigned* in = lds[p & 1];
        unsigned* out = lds[(p & 1) ^ 1];
        const int hp = (passes - 1 - p) * (r + 1);
        const int y_lo = max(y0 - hp, 0), y_hi = min(y0 + th + hp, H);
        for (int y = y_lo + (threadIdx.x >> 5); live && y < y_hi; y += 256 / ND) {
            unsigned lo = 0, hi = 0, elo = 0, ehi = 0;
            for (int i = -r; i <= r; ++i) blur_add4(lo, hi, in[(clampi(y + i, 0, H - 1) - ybase) * ND + d]);
            blur_add4(elo, ehi, in[(clampi(y - r - 1, 0, H - 1) - ybase) * ND + d]);
            blur_add4(elo, ehi, in[(clampi(y + r + 1, 0, H - 1) - ybase) * ND + d]);
            const unsigned res = blur_pack4(lo, hi, elo, ehi, ww, fw);
            if (p + 1 < passes) out[(y - ybase) * ND + d] = res;
            else store4_guarded(dst + (int64_t)blockIdx.z * db + (int64_t)y * dr, g, row_bytes, vec_out != 0, res);
        }
    }
}

// any radius, one pass, one output byte per thread straight from memory: the window is clipped to the line and its clamped ends are counted, so a
// byte costs at most `size` reads however large r is (r + 1 >= size included)
__global__ __launch_bounds__(256) void blur_direct_kernel(const uint8_t* __restrict__ src, int64_t sb, int64_t sr, int H, int W, int C, uint8_t* __restrict__ dst,
                                                          int64_t db, int64_t dr, int vertical, int r, unsigned ww, unsigned fw) {
    const int g = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (g >= W * C) return;
    const uint8_t* line = src + (int64_t)blockIdx.z * sb;
    int64_t step;
    int n, pos;
    if (vertical) { line += g; step = sr; n = H; pos = y; }
    else { pos = g / C; line += (int64_t)y * sr + (g - pos * C); step = C; n = W; }
    const int lo = pos - r, hi = pos + r;                                          // r, pos < 2^24
    unsigned sum = (unsigned)max(-lo, 0) * line[0] + (unsigned)max(hi - (n - 1), 0) * line[(n - 1) * step];
    for (int i = max(lo, 0); i <= min(hi, n - 1); ++i) sum += line[i * step];
    const unsigned edge = (unsigned)line[clampi(lo - 1, 0, n - 1) * step] + line[clampi(hi + 1, 0, n - 1) * step];
    dst[(int64_t)blockIdx.z * db + (int64_t)y * dr + g] = (uint8_t)blur_byte(sum, edge, ww, fw);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
static bool img_args_ok(const void* p, int64_t sb, int64_t sr, int64_t B, int64_t H, int64_t W, int64_t C) {
    return p && B >= 1 && H >= 1 && W >= 1 && B < 65536 && H < 65536 && W < (1 << 24) && sr >= W * C && (B == 1 || sb >= H * sr || sb >= (H - 1) * sr + W * C);
}
static bool strided_aligned(const void* p, int64_t sb, int64_t sr, int a) { return ug_aligned(p, a) && sb % a == 0 && sr % a == 0; }

extern "C" int ug_canny_grad(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int16_t* dx, int16_t* dy,
                             int32_t* mag, ug_stream_t stream) {
    UG_REQUIRE((C == 1 || C == 3) && img_args_ok(img, bstride, rstride, B, H, W, C) && dx && dy && mag, UG_ERR_BAD_SHAPE,
               "ug_canny_grad: bad arguments (B=%lld H=%lld W=%lld C=%d; C is 1 or 3, strides cover a row / a sample)", (long long)B, (long long)H,
               (long long)W, C);
    const dim3 grid((unsigned)ug_cdiv(W, CT_W), (unsigned)ug_cdiv(H, CT_H), (unsigned)B);
    const int vin = strided_aligned(img, bstride, rstride, 4), vout = W % 4 == 0 && ug_aligned(dx, 8) && ug_aligned(dy, 8) && ug_aligned(mag, 16);
    if (C == 1) hipLaunchKernelGGL(canny_grad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, img, bstride, rstride, (int)H, (int)W, dx, dy, mag, vin, vout);
    else hipLaunchKernelGGL(canny_grad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, img, bstride, rstride, (int)H, (int)W, dx, dy, mag, vin, vout);
    UG_CHECK_LAUNCH("ug_canny_grad");
    return UG_OK;
}

extern "C" int ug_canny_nms(const int16_t* dx, const int16_t* dy, const int32_t* mag, int64_t B, int64_t H, int64_t W, int32_t low, int32_t high, uint8_t* map,
                            ug_stream_t stream) {
    UG_REQUIRE(dx && dy && mag && map && B >= 1 && H >= 1 && W >= 1 && B < 65536 && H < 65536 && W < (1 << 24), UG_ERR_BAD_SHAPE,
               "ug_canny_nms: bad arguments (B=%lld H=%lld W=%lld)", (long long)B, (long long)H, (long long)W);
    if (low > high) { const int32_t t = low; low = high; high = t; }
    const dim3 grid((unsigned)ug_cdiv(W, CT_W), (unsigned)ug_cdiv(H, CT_H), (unsigned)B);
    const int vec = W % 4 == 0 && ug_aligned(dx, 8) && ug_aligned(dy, 8) && ug_aligned(map, 4);
    hipLaunchKernelGGL(canny_nms_kernel, grid, dim3(256), 0, (hipStream_t)stream, dx, dy, mag, (int)H, (int)W, low, high, map, vec);
    UG_CHECK_LAUNCH("ug_canny_nms");
    return UG_OK;
}

extern "C" int64_t ug_canny_max_sweeps(int64_t H, int64_t W) { return (H < 1 || W < 1) ? 0 : H * W + 1; }

extern "C" int ug_canny_hysteresis(uint8_t* map, int64_t B, int64_t H, int64_t W, uint8_t* out, int64_t out_bstride, int64_t out_rstride, int32_t* flag,
                                   int32_t* sweeps_host, ug_stream_t stream) {
    UG_REQUIRE(map && flag && img_args_ok(out, out_bstride, out_rstride, B, H, W, 1), UG_ERR_BAD_SHAPE,
               "ug_canny_hysteresis: bad arguments (B=%lld H=%lld W=%lld)", (long long)B, (long long)H, (long long)W);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ug_cdiv(W, HT_W), (unsigned)ug_cdiv(H, HT_H), (unsigned)B);
    const int vec = W % 4 == 0 && ug_aligned(map, 4);
    const int64_t bound = ug_canny_max_sweeps(H, W);
    int64_t n = 0;
    int32_t raised = 1;
    while (raised && n < bound) {          // hard bound: every sweep that raises the flag promoted at least one of the H * W pixels
        hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), s);
        if (e != hipSuccess) UG_FAIL(UG_ERR_HIP, "ug_canny_hysteresis: memset failed: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(canny_hyst_sweep_kernel, grid, dim3(256), 0, s, map, (int)H, (int)W, vec, flag);
        UG_CHECK_LAUNCH("ug_canny_hysteresis");
        e = hipMemcpyAsync(&raised, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) UG_FAIL(UG_ERR_HIP, "ug_canny_hysteresis: reading the sweep flag failed: %s", hipGetErrorString(e));
        ++n;
    }
    UG_REQUIRE(!raised, UG_ERR_HIP, "ug_canny_hysteresis: no fixed point after %lld sweeps", (long long)n);
    const dim3 fgrid((unsigned)ug_cdiv(W, 256 * 16), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(canny_final_kernel, fgrid, dim3(256), 0, s, map, (int)H, (int)W, out, out_bstride, out_rstride, (int)(W % 16 == 0 && ug_aligned(map, 16)),
                       (int)strided_aligned(out, out_bstride, out_rstride, 16));
    UG_CHECK_LAUNCH("ug_canny_hysteresis");
    if (sweeps_host) *sweeps_host = (int32_t)(n > 0x7fffffff ? 0x7fffffff : n);
    return UG_OK;
}

// workspace of ug_canny_u8: dx, dy (int16), mag (int32), map (uint8) per pixel, each 256-byte aligned, and the sweep flag
static int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
extern "C" int64_t ug_canny_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const int64_t n = B * H * W;
    return 2 * up256(2 * n) + up256(4 * n) + up256(n) + 256;
}

extern "C" int ug_canny_u8(const uint8_t* img, int64_t bstride, int64_t rstride, int64_t B, int64_t H, int64_t W, int32_t C, int32_t low, int32_t high,
                           uint8_t* out, int64_t out_bstride, int64_t out_rstride, void* workspace, int64_t workspace_bytes, int32_t* sweeps_host,
                           ug_stream_t stream) {
    UG_REQUIRE(B >= 1 && H >= 1 && W >= 1 && workspace && workspace_bytes >= ug_canny_workspace_bytes(B, H, W) && ug_aligned(workspace, 16), UG_ERR_BAD_SHAPE,
               "ug_canny_u8: bad shape or a workspace smaller than ug_canny_workspace_bytes (B=%lld H=%lld W=%lld)", (long long)B, (long long)H, (long long)W);
    const int64_t n = B * H * W;
    uint8_t* w = (uint8_t*)workspace;
    int16_t* dx = (int16_t*)w;
    int16_t* dy = (int16_t*)(w + up256(2 * n));
    int32_t* mag = (int32_t*)(w + 2 * up256(2 * n));
    uint8_t* map = w + 2 * up256(2 * n) + up256(4 * n);
    int32_t* flag = (int32_t*)(map + up256(n));
    int rc = ug_canny_grad(img, bstride, rstride, B, H, W, C, dx, dy, mag, stream);
    if (rc != UG_OK) return rc;
    rc = ug_canny_nms(dx, dy, mag, B, H, W, low, high, map, stream);          // swaps low > high
    if (rc != UG_OK) return rc;
    return ug_canny_hysteresis(map, B, H, W, out, out_bstride, out_rstride, flag, sweeps_host, stream);
}

extern "C" int ug_img_resize_u8(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t Hin, int64_t Win, int32_t C, uint8_t* dst,
                                int64_t dst_bstride, int64_t dst_rstride, int64_t Hout, int64_t Wout, const int32_t* xbounds, const int32_t* xcoef,
                                int32_t xk, const int32_t* ybounds, const int32_t* ycoef, int32_t yk, uint8_t* tmp, ug_stream_t stream) {
    const bool horiz = Wout != Win, vert = Hout != Hin;
    UG_REQUIRE((C == 1 || C == 3) && img_args_ok(src, src_bstride, src_rstride, B, Hin, Win, C) && img_args_ok(dst, dst_bstride, dst_rstride, B, Hout, Wout, C),
               UG_ERR_BAD_SHAPE, "ug_img_resize_u8: bad arguments (B=%lld %lldx%lld -> %lldx%lld C=%d)", (long long)B, (long long)Hin, (long long)Win,
               (long long)Hout, (long long)Wout, C);
    UG_REQUIRE((!horiz || (xbounds && xcoef && xk >= 1)) && (!vert || (ybounds && ycoef && yk >= 1)) && (!(horiz && vert) || tmp), UG_ERR_BAD_SHAPE,
               "ug_img_resize_u8: a pass that changes a size needs its bounds and coefficient tables, and two passes need the intermediate image");
    hipStream_t s = (hipStream_t)stream;
    if (!horiz && !vert) {                 // nothing to resample: a copy, row by row
        hipError_t e = hipSuccess;
        for (int64_t b = 0; b < B && e == hipSuccess; ++b)
            e = hipMemcpy2DAsync(dst + b * dst_bstride, (size_t)dst_rstride, src + b * src_bstride, (size_t)src_rstride, (size_t)(Win * C), (size_t)Hin,
                                 hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) UG_FAIL(UG_ERR_HIP, "ug_img_resize_u8: copy failed: %s", hipGetErrorString(e));
        return UG_OK;
    }
    // horizontal first, into the uint8 intermediate [B, Hin, Wout, C] (or straight into dst when the height stays)
    const uint8_t* vsrc = src;
    int64_t vsb = src_bstride, vsr = src_rstride;
    if (horiz) {
        uint8_t* hd = vert ? tmp : dst;
        const int64_t hdb = vert ? Hin * Wout * C : dst_bstride, hdr = vert ? Wout * C : dst_rstride;
        const dim3 grid((unsigned)ug_cdiv(Wout, 256), (unsigned)Hin, (unsigned)B);
        const int vin = strided_aligned(src, src_bstride, src_rstride, 4), vout = strided_aligned(hd, hdb, hdr, 4);
        if (C == 1) hipLaunchKernelGGL(resize_h_kernel<1>, grid, dim3(256), 0, s, src, src_bstride, src_rstride, (int)Win, hd, hdb, hdr, (int)Wout, xbounds, xcoef, (int)xk, vin, vout);
        else hipLaunchKernelGGL(resize_h_kernel<3>, grid, dim3(256), 0, s, src, src_bstride, src_rstride, (int)Win, hd, hdb, hdr, (int)Wout, xbounds, xcoef, (int)xk, vin, vout);
        UG_CHECK_LAUNCH("ug_img_resize_u8");
        vsrc = hd; vsb = hdb; vsr = hdr;
    }
    if (vert) {
        const int64_t row_bytes = Wout * C;
        const dim3 grid((unsigned)ug_cdiv(row_bytes, 256 * 16), (unsigned)Hout, (unsigned)B);
        hipLaunchKernelGGL(resize_v_kernel, grid, dim3(256), 0, s, vsrc, vsb, vsr, (int)Hin, row_bytes, dst, dst_bstride, dst_rstride, ybounds, ycoef, (int)yk,
                           (int)strided_aligned(vsrc, vsb, vsr, 16), (int)strided_aligned(dst, dst_bstride, dst_rstride, 16));
        UG_CHECK_LAUNCH("ug_img_resize_u8");
    }
    return UG_OK;
}

extern "C" int ug_img_rgb_to_l(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, uint8_t* dst, int64_t dst_bstride,
                               int64_t dst_rstride, ug_stream_t stream) {
    UG_REQUIRE(img_args_ok(src, src_bstride, src_rstride, B, H, W, 3) && img_args_ok(dst, dst_bstride, dst_rstride, B, H, W, 1), UG_ERR_BAD_SHAPE,
               "ug_img_rgb_to_l: bad arguments (B=%lld H=%lld W=%lld)", (long long)B, (long long)H, (long long)W);
    const dim3 grid((unsigned)ug_cdiv(W, 256 * 16), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(rgb_to_l_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, src_bstride, src_rstride, (int)W, dst, dst_bstride, dst_rstride,
                       (int)strided_aligned(src, src_bstride, src_rstride, 16), (int)strided_aligned(dst, dst_bstride, dst_rstride, 16));
    UG_CHECK_LAUNCH("ug_img_rgb_to_l");
    return UG_OK;
}

template <typename T>
static int u8_to_chw_launch(const uint8_t* src, int64_t sb, int64_t sr, int64_t B, int64_t H, int64_t W, int C, void* dst, int Cout, int normalize, hipStream_t s) {
    const dim3 grid((unsigned)ug_cdiv(W, 256 * 4), (unsigned)H, (unsigned)B);
    const int vin = strided_aligned(src, sb, sr, 4), vout = W % 4 == 0 && ug_aligned(dst, 16);
    if (C == 1) hipLaunchKernelGGL((u8_to_chw_kernel<T, 1>), grid, dim3(256), 0, s, src, sb, sr, (int)H, (int)W, (T*)dst, Cout, normalize, vin, vout);
    else hipLaunchKernelGGL((u8_to_chw_kernel<T, 3>), grid, dim3(256), 0, s, src, sb, sr, (int)H, (int)W, (T*)dst, Cout, normalize, vin, vout);
    UG_CHECK_LAUNCH("ug_img_u8_to_chw");
    return UG_OK;
}
extern "C" int ug_img_u8_to_chw(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, int32_t C, void* dst,
                                int32_t dst_dtype, int32_t Cout, int32_t normalize, ug_stream_t stream) {
    UG_REQUIRE((C == 1 || C == 3) && (Cout == C || (C == 1 && Cout == 3)) && img_args_ok(src, src_bstride, src_rstride, B, H, W, C) && dst &&
               (dst_dtype == UG_DT_BF16 || dst_dtype == UG_DT_F32), UG_ERR_BAD_SHAPE,
               "ug_img_u8_to_chw: bad arguments (B=%lld H=%lld W=%lld C=%d -> %d channels, dtype %d)", (long long)B, (long long)H, (long long)W, C, Cout, dst_dtype);
    return dst_dtype == UG_DT_F32 ? u8_to_chw_launch<float>(src, src_bstride, src_rstride, B, H, W, C, dst, Cout, normalize, (hipStream_t)stream)
                                  : u8_to_chw_launch<bf16_t>(src, src_bstride, src_rstride, B, H, W, C, dst, Cout, normalize, (hipStream_t)stream);
}

extern "C" int ug_img_chw_to_u8(const void* src, int32_t src_dtype, int64_t B, int32_t C, int64_t H, int64_t W, uint8_t* dst, int64_t dst_bstride,
                                int64_t dst_rstride, int32_t denormalize, ug_stream_t stream) {
    UG_REQUIRE(src && C >= 1 && C <= 4 && img_args_ok(dst, dst_bstride, dst_rstride, B, H, W, C) && (src_dtype == UG_DT_BF16 || src_dtype == UG_DT_F32),
               UG_ERR_BAD_SHAPE, "ug_img_chw_to_u8: bad arguments (B=%lld C=%d H=%lld W=%lld, dtype %d; 1 to 4 channels)", (long long)B, C, (long long)H,
               (long long)W, src_dtype);
    const dim3 grid((unsigned)ug_cdiv(W, CU_SEG), (unsigned)H, (unsigned)B);
    const int vout = strided_aligned(dst, dst_bstride, dst_rstride, 16);
    if (src_dtype == UG_DT_F32)
        hipLaunchKernelGGL(chw_to_u8_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, C, (int)H, (int)W, dst, dst_bstride, dst_rstride,
                           (int)denormalize, (int)(W % 4 == 0 && ug_aligned(src, 16)), vout);
    else
        hipLaunchKernelGGL(chw_to_u8_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, C, (int)H, (int)W, dst, dst_bstride, dst_rstride,
                           (int)denormalize, (int)(W % 8 == 0 && ug_aligned(src, 16)), vout);
    UG_CHECK_LAUNCH("ug_img_chw_to_u8");
    return UG_OK;
}

// workspace of ug_img_box_blur_u8: two contiguous images [B, H, W, C], each 256-byte aligned, that the launches alternate between
extern "C" int64_t ug_img_blur_workspace_bytes(int64_t B, int64_t H, int64_t W, int32_t C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return 0;
    return 2 * up256(B * H * W * C);
}

static bool blur_consts_ok(int64_t r, int64_t ww, int64_t fw) {                     // weights that sum to at most 2^24: no pass overflows uint32
    return r >= 0 && r < (1 << 24) && ww >= 0 && fw >= 0 && (2 * r + 1) * ww + 2 * fw <= (1 << 24);
}
static bool blur_identity(int64_t r, int64_t ww, int64_t fw) { return r == 0 && fw == 0 && ww == (1 << 24); }      // the constants of radius 0: PIL skips the axis

extern "C" int ug_img_box_blur_u8(const uint8_t* src, int64_t src_bstride, int64_t src_rstride, int64_t B, int64_t H, int64_t W, int32_t C, uint8_t* dst,
                                  int64_t dst_bstride, int64_t dst_rstride, int32_t rx, int32_t wwx, int32_t fwx, int32_t ry, int32_t wwy, int32_t fwy,
                                  int32_t passes, int32_t fuse, void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    UG_REQUIRE((C == 1 || C == 3) && img_args_ok(src, src_bstride, src_rstride, B, H, W, C) && img_args_ok(dst, dst_bstride, dst_rstride, B, H, W, C),
               UG_ERR_BAD_SHAPE, "ug_img_box_blur_u8: bad arguments (B=%lld H=%lld W=%lld C=%d; C is 1 or 3, strides cover a row / a sample)", (long long)B,
               (long long)H, (long long)W, C);
    UG_REQUIRE(passes >= 1 && (fuse == 0 || fuse == 1), UG_ERR_BAD_SHAPE, "ug_img_box_blur_u8: passes = %d (at least 1), fuse = %d (0 generic, 1 auto)", passes, fuse);
    UG_REQUIRE(blur_consts_ok(rx, wwx, fwx) && blur_consts_ok(ry, wwy, fwy), UG_ERR_BAD_SHAPE,
               "ug_img_box_blur_u8: bad constants (r, ww, fw) = (%d, %d, %d), (%d, %d, %d): 0 <= r < 2^24, weights >= 0 with (2 r + 1) ww + 2 fw <= 2^24", rx, wwx,
               fwx, ry, wwy, fwy);
    const int64_t img_bytes = up256(B * H * W * C);
    UG_REQUIRE(workspace && workspace_bytes >= 2 * img_bytes && ug_aligned(workspace, 16), UG_ERR_BAD_SHAPE,
               "ug_img_box_blur_u8: a 16-byte aligned workspace of ug_img_blur_workspace_bytes = %lld bytes is needed (got %lld)", (long long)(2 * img_bytes),
               (long long)workspace_bytes);
    const uint8_t* src_end = src + (B - 1) * src_bstride + (H - 1) * src_rstride + W * C;
    const uint8_t* dst_end = dst + (B - 1) * dst_bstride + (H - 1) * dst_rstride + W * C;
    UG_REQUIRE(dst_end <= src || src_end <= dst, UG_ERR_BAD_SHAPE, "ug_img_box_blur_u8: dst must not alias src");
    hipStream_t s = (hipStream_t)stream;
    struct Axis { int r, ww, fw, vertical, launches, per; bool tile; } axes[2] = {{rx, wwx, fwx, 0, 0, 0, false}, {ry, wwy, fwy, 1, 0, 0, false}};
    int total = 0;
    for (Axis& a : axes) {
        if (blur_identity(a.r, a.ww, a.fw)) continue;
        const int64_t halo_max = a.vertical ? BV_HALO_MAX : BH_HALO_MAX;
        const bool fused = fuse && (int64_t)passes * (a.r + 1) <= halo_max;        // all passes of the axis in one launch when their halo fits in LDS
        a.tile = a.r + 1 <= halo_max;
        a.per = fused ? passes : 1;
        a.launches = fused ? 1 : passes;
        total += a.launches;
    }
    if (total == 0) {                      // radius 0 on both axes: a copy, row by row
        hipError_t e = hipSuccess;
        for (int64_t b = 0; b < B && e == hipSuccess; ++b)
            e = hipMemcpy2DAsync(dst + b * dst_bstride, (size_t)dst_rstride, src + b * src_bstride, (size_t)src_rstride, (size_t)(W * C), (size_t)H,
                                 hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) UG_FAIL(UG_ERR_HIP, "ug_img_box_blur_u8: copy failed: %s", hipGetErrorString(e));
        return UG_OK;
    }
    uint8_t* ws[2] = {(uint8_t*)workspace, (uint8_t*)workspace + img_bytes};
    const int64_t wsb = H * W * C, wsr = W * C;
    int k = 0;
    for (const Axis& a : axes)
        for (int l = 0; l < a.launches; ++l, ++k) {
            const uint8_t* in = k == 0 ? src : ws[(k - 1) & 1];
            const int64_t ib = k == 0 ? src_bstride : wsb, ir = k == 0 ? src_rstride : wsr;
            uint8_t* out = k == total - 1 ? dst : ws[k & 1];
            const int64_t ob = k == total - 1 ? dst_bstride : wsb, orow = k == total - 1 ? dst_rstride : wsr;
            const int vin = strided_aligned(in, ib, ir, 4), vout = strided_aligned(out, ob, orow, 4);
            const int halo = a.per * (a.r + 1);
            if (!a.tile) {
                const dim3 grid((unsigned)ug_cdiv(W * C, 256), (unsigned)H, (unsigned)B);
                hipLaunchKernelGGL(blur_direct_kernel, grid, dim3(256), 0, s, in, ib, ir, (int)H, (int)W, (int)C, out, ob, orow, a.vertical, a.r, (unsigned)a.ww,
                                   (unsigned)a.fw);
            } else if (a.vertical) {
                const int th = BV_ROWS - 2 * halo < BV_TH_MAX ? BV_ROWS - 2 * halo : BV_TH_MAX;
                const dim3 grid((unsigned)ug_cdiv(W * C, BV_WB), (unsigned)ug_cdiv(H, th), (unsigned)B);
                hipLaunchKernelGGL(blur_v_kernel, grid, dim3(256), 0, s, in, ib, ir, (int)H, (int)(W * C), out, ob, orow, a.r, (unsigned)a.ww, (unsigned)a.fw, a.per, th,
                                   vin, vout);
            } else {
                const int nds = ((BH_TW + 2 * halo) * C + 12) / 4;
                const dim3 grid((unsigned)ug_cdiv(W, BH_TW), (unsigned)ug_cdiv(H, BH_ROWS), (unsigned)B);
                if (C == 1) hipLaunchKernelGGL(blur_h_kernel<1>, grid, dim3(256), 0, s, in, ib, ir, (int)H, (int)W, out, ob, orow, a.r, (unsigned)a.ww, (unsigned)a.fw, a.per, nds, vin, vout);
                else hipLaunchKernelGGL(blur_h_kernel<3>, grid, dim3(256), 0, s, in, ib, ir, (int)H, (int)W, out, ob, orow, a.r, (unsigned)a.ww, (unsigned)a.fw, a.per, nds, vin, vout);
            }
            UG_CHECK_LAUNCH("ug_img_box_blur_u8");
        }
    return UG_OK;
}
