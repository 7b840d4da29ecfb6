// The two kernel classes of diffusers' SanaTransformerBlock that nothing else in this library computes (unigen_amd/sana.py):
//   ug_linear_attn(_f32)     SanaLinearAttnProcessor2_0: softmax-free ReLU linear attention at head width 32
//   ug_glu_dwconv3x3(_f32)   the middle of GLUMBConv: SiLU, depthwise 3x3 convolution, SiLU gate
// By their byte and operation counts both are bound by HBM; as built their instruction counts point at LDS and VALU issue (docs/KERNEL_NOTES.md, "Sana kernels").
// Neither uses the matrix cores.
//
// ---- linear attention ----
// With q' = relu(q), k' = relu(k), per (batch, head):  S[d][j] = sum_n v[n][d] k'[n][j],  z[j] = sum_n k'[n][j]   (1024 + 32 floats, fp32)
//                                                     out[n][d] = sum_j S[d][j] q'[n][j] / (sum_j z[j] q'[n][j] + 1e-15)
// Three launches on the caller's workspace, every word of which is written before it is read in the same call:
//   linattn_state_kernel   one workgroup = LA_CHUNK tokens x up to 4 adjacent heads (128 columns = whole 256-byte lines of bf16, 16 bytes per lane):
//                          k' and v of 32 tokens are staged in LDS as fp32, wave w owns head w of the group, lane (d, half) 16 entries of S. z is summed
//                          by the loading threads (their own 8 columns) and folded over the 16 row groups in a fixed order. -> partial[b][h][chunk]
//   linattn_reduce_kernel  partials summed over the chunks in ascending order -> state[b][h] as S^T[j][d] | z[j]
//   linattn_apply_kernel   one workgroup = LA_ROWS query rows x up to 4 heads: the heads' states in LDS, q' of 16 rows at a time in LDS, thread
//                          (row, octet) computes 8 outputs of its head and the denominator, one rounding at the store.
// No atomics: the sums have one order, so two launches give the same bits.
//
// ---- GLU depthwise convolution ----
// x [B][H][W] rows of 2C (value half | gate half), row stride ldx. One workgroup = 32 image columns x GT_ROWS image rows x OCT channel octets of both
// halves. It walks down its rows: the 34 pixels (one halo pixel either side) of an input row are loaded once, SiLU'd once, rounded (bf16) and put into a
// four-row ring in LDS; an output row is computed when the row below it is in. Pixels outside the image are zeros in the ring (the convolution's zero
// padding acts on the activation). The next input row is in flight in registers while an output row is computed. The taps and the bias are in LDS too.
#include "ug_common.h"

namespace {

constexpr int LA_DH = 32;                        // head width
constexpr int LA_HG = 4;                         // heads per workgroup: 128 columns
constexpr int LA_COLS = LA_HG * LA_DH;
constexpr int LA_TOK = 32;                       // tokens per LDS tile of the state pass
constexpr int LA_CHUNK = 256;                    // tokens per workgroup of the state pass
constexpr int LA_ROWS = 128;                     // query rows per workgroup of the apply pass
constexpr int LA_STATE = LA_DH * LA_DH + LA_DH;  // S | z: 1056 floats
constexpr float LA_EPS = 1e-15f;

__host__ __device__ inline int64_t la_chunks(int64_t N) { return (N + LA_CHUNK - 1) / LA_CHUNK; }

template <typename T>
__global__ __launch_bounds__(256) void linattn_state_kernel(const T* __restrict__ k, int64_t k_rs, int64_t k_bs, const T* __restrict__ v, int64_t v_rs,
                                                            int64_t v_bs, int heads, int64_t N, int nchunk, float* __restrict__ partial) {
    using E = ElemT<T>;
    __shared__ __attribute__((aligned(16))) float ks[LA_TOK][LA_COLS];
    __shared__ __attribute__((aligned(16))) float vs[LA_TOK][LA_COLS];
    __shared__ float zs[16][LA_COLS];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, hg = blockIdx.y, b = blockIdx.z;
    const int h0 = hg * LA_HG;
    const int nh = min(LA_HG, heads - h0);                 // heads of this group
    const int c8 = tid & 15, lr = tid >> 4;                // loader: column octet, row within a pass of 16 rows
    const bool col_ok = c8 * 8 < nh * LA_DH;
    const T* kb = k + (int64_t)b * k_bs + h0 * LA_DH + c8 * 8;
    const T* vb = v + (int64_t)b * v_bs + h0 * LA_DH + c8 * 8;
    const int wave = tid >> 6, lane = tid & 63;
    const int d = lane >> 1, j0 = (lane & 1) * 16;         // compute: S[d][j0 .. j0 + 15] of head h0 + wave
    float acc[16], zp[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) zp[i] = 0.f;
    const int64_t n0 = (int64_t)chunk * LA_CHUNK;
    const int64_t n1 = min(N, n0 + LA_CHUNK);
    for (int64_t t0 = n0; t0 < n1; t0 += LA_TOK) {
#pragma unroll
        for (int p = 0; p < LA_TOK / 16; ++p) {
            const int r = lr + 16 * p;
            const int64_t n = t0 + r;
            float kf[8], vf[8];
            if (col_ok && n < n1) {
                E::load8(kb + n * k_rs, kf);
                E::load8(vb + n * v_rs, vf);
#pragma unroll
                for (int i = 0; i < 8; ++i) kf[i] = fmaxf(kf[i], 0.f);
            } else {                                       // past the chunk or past the group's heads: contributes nothing
#pragma unroll
                for (int i = 0; i < 8; ++i) { kf[i] = 0.f; vf[i] = 0.f; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) zp[i] += kf[i];
            *(f32x4*)&ks[r][c8 * 8] = (f32x4){kf[0], kf[1], kf[2], kf[3]};
            *(f32x4*)&ks[r][c8 * 8 + 4] = (f32x4){kf[4], kf[5], kf[6], kf[7]};
            *(f32x4*)&vs[r][c8 * 8] = (f32x4){vf[0], vf[1], vf[2], vf[3]};
            *(f32x4*)&vs[r][c8 * 8 + 4] = (f32x4){vf[4], vf[5], vf[6], vf[7]};
        }
        __syncthreads();
        if (wave < nh) {
#pragma unroll 4
            for (int t = 0; t < LA_TOK; ++t) {
                const float vv = vs[t][wave * LA_DH + d];
                const float* kr = &ks[t][wave * LA_DH + j0];
#pragma unroll
                for (int i4 = 0; i4 < 4; ++i4) {
                    const f32x4 kk = *(const f32x4*)(kr + 4 * i4);
                    acc[4 * i4 + 0] = fmaf(vv, kk[0], acc[4 * i4 + 0]); acc[4 * i4 + 1] = fmaf(vv, kk[1], acc[4 * i4 + 1]);
                    acc[4 * i4 + 2] = fmaf(vv, kk[2], acc[4 * i4 + 2]); acc[4 * i4 + 3] = fmaf(vv, kk[3], acc[4 * i4 + 3]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) zs[lr][c8 * 8 + i] = zp[i];
    __syncthreads();
    if (wave < nh) {
        float* out = partial + (((int64_t)b * heads + h0 + wave) * nchunk + chunk) * LA_STATE;
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
            *(f32x4*)(out + d * LA_DH + j0 + 4 * i4) = (f32x4){acc[4 * i4], acc[4 * i4 + 1], acc[4 * i4 + 2], acc[4 * i4 + 3]};
        if (lane < LA_DH) {
            float z = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) z += zs[r][wave * LA_DH + lane];
            out[LA_DH * LA_DH + lane] = z;
        }
    }
}

// state[bh] = sum over chunks (ascending) of partial[bh][chunk]; S is written transposed, S^T[j][d], the layout the apply pass reads
__global__ __launch_bounds__(256) void linattn_reduce_kernel(const float* __restrict__ partial, int nchunk, float* __restrict__ state) {
    const int64_t bh = blockIdx.x;
    const float* p = partial + bh * nchunk * LA_STATE;
    float* s = state + bh * LA_STATE;
    for (int e = threadIdx.x; e < LA_STATE; e += 256) {
        float a = 0.f;
        for (int c = 0; c < nchunk; ++c) a += p[(int64_t)c * LA_STATE + e];
        if (e < LA_DH * LA_DH) s[(e & (LA_DH - 1)) * LA_DH + (e >> 5)] = a;
        else s[e] = a;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void linattn_apply_kernel(const T* __restrict__ q, int64_t q_rs, int64_t q_bs, T* __restrict__ o, int64_t o_rs, int64_t o_bs,
                                                            int heads, int64_t N, const float* __restrict__ state) {
    using E = ElemT<T>;
    __shared__ __attribute__((aligned(16))) float st[LA_HG][LA_STATE];
    __shared__ __attribute__((aligned(16))) float qs[16][LA_COLS];
    const int tid = threadIdx.x;
    const int hg = blockIdx.y, b = blockIdx.z;
    const int h0 = hg * LA_HG;
    const int nh = min(LA_HG, heads - h0);
    const float* sb = state + ((int64_t)b * heads + h0) * LA_STATE;
    for (int e = tid; e < nh * LA_STATE; e += 256) (&st[0][0])[e] = sb[e];
    const int c8 = tid & 15, lr = tid >> 4;
    const int hl = c8 >> 2, d0 = (c8 & 3) * 8;             // this thread's head within the group and its 8 output columns
    const bool col_ok = hl < nh;
    const T* qb = q + (int64_t)b * q_bs + h0 * LA_DH + c8 * 8;
    T* ob = o + (int64_t)b * o_bs + h0 * LA_DH + c8 * 8;
    const int64_t r0 = (int64_t)blockIdx.x * LA_ROWS;
    for (int p = 0; p < LA_ROWS / 16; ++p) {
        const int64_t n = r0 + 16 * p + lr;
        if (r0 + 16 * p >= N) break;                       // uniform over the workgroup
        const bool live = col_ok && n < N;
        float qf[8];
        if (live) {
            E::load8(qb + n * q_rs, qf);
#pragma unroll
            for (int i = 0; i < 8; ++i) qf[i] = fmaxf(qf[i], 0.f);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) qf[i] = 0.f;
        }
        __syncthreads();                                   // the previous pass has read qs (first pass: st is complete)
        *(f32x4*)&qs[lr][c8 * 8] = (f32x4){qf[0], qf[1], qf[2], qf[3]};
        *(f32x4*)&qs[lr][c8 * 8 + 4] = (f32x4){qf[4], qf[5], qf[6], qf[7]};
        __syncthreads();
        if (live) {
            float num[8], den = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) num[i] = 0.f;
            const float* sh = st[hl];
#pragma unroll 2
            for (int j4 = 0; j4 < LA_DH / 4; ++j4) {
                const f32x4 qq = *(const f32x4*)&qs[lr][hl * LA_DH + 4 * j4];
                const f32x4 zz = *(const f32x4*)&sh[LA_DH * LA_DH + 4 * j4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float* sr = sh + (4 * j4 + jj) * LA_DH + d0;
                    const f32x4 s0 = *(const f32x4*)sr, s1 = *(const f32x4*)(sr + 4);
                    const float qv = qq[jj];
                    num[0] = fmaf(s0[0], qv, num[0]); num[1] = fmaf(s0[1], qv, num[1]); num[2] = fmaf(s0[2], qv, num[2]); num[3] = fmaf(s0[3], qv, num[3]);
                    num[4] = fmaf(s1[0], qv, num[4]); num[5] = fmaf(s1[1], qv, num[5]); num[6] = fmaf(s1[2], qv, num[6]); num[7] = fmaf(s1[3], qv, num[7]);
                    den = fmaf(zz[jj], qv, den);
                }
            }
            den += LA_EPS;
            float r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = num[i] / den;
            E::store8(ob + n * o_rs, r);
        }
    }
}

template <typename T>
int linear_attn_impl(const char* who, const void* q, int64_t q_rs, int64_t q_bs, const void* k, int64_t k_rs, int64_t k_bs, const void* v, int64_t v_rs,
                     int64_t v_bs, void* o, int64_t o_rs, int64_t o_bs, int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace,
                     ug_stream_t stream) {
    if (batches == 0 || N == 0) return UG_OK;
    UG_REQUIRE(q && k && v && o && workspace && batches > 0 && heads > 0 && N > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(dh == LA_DH, UG_ERR_UNSUPPORTED, "%s: head dim %d is not 32", who, dh);
    constexpr int A = ElemT<T>::kF32 ? 4 : 8;              // elements of 16 bytes
    const ug_view_rule views[] = {{"q", {q, q_rs, q_bs}, A, 16, false}, {"k", {k, k_rs, k_bs}, A, 16, false}, {"v", {v, v_rs, v_bs}, A, 16, false},
                                  {"o", {o, o_rs, o_bs}, A, 16, false}, {"workspace", {workspace, 0, 0}, A, 16, false}};
    if (const int rc = ug_check_views(who, views)) return rc;
    // grid limits: y = head groups and z = batches below 65536; the reduce pass has one workgroup per (batch, head) on x
    UG_REQUIRE(N < (1ll << 30) && batches < 65536 && (heads + LA_HG - 1) / LA_HG < 65536 && batches * (int64_t)heads < (1ll << 31), UG_ERR_UNSUPPORTED,
               "%s: too large", who);
    const int nchunk = (int)la_chunks(N);
    const unsigned ngroups = (unsigned)((heads + LA_HG - 1) / LA_HG);
    float* state = (float*)workspace;
    float* partial = state + batches * heads * LA_STATE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(linattn_state_kernel<T>, dim3((unsigned)nchunk, ngroups, (unsigned)batches), dim3(256), 0, s, (const T*)k, k_rs, k_bs, (const T*)v, v_rs,
                       v_bs, (int)heads, N, nchunk, partial);
    UG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(linattn_reduce_kernel, dim3((unsigned)(batches * heads)), dim3(256), 0, s, (const float*)partial, nchunk, state);
    UG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(linattn_apply_kernel<T>, dim3((unsigned)((N + LA_ROWS - 1) / LA_ROWS), ngroups, (unsigned)batches), dim3(256), 0, s, (const T*)q, q_rs,
                       q_bs, (T*)o, o_rs, o_bs, (int)heads, N, (const float*)state);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

// ---- GLU depthwise 3x3 ----
constexpr int GT_W = 32;                         // image columns per workgroup
constexpr int GT_ROWS = 16;                      // image rows per workgroup
constexpr int GT_PX = GT_W + 2;                  // a ring row: the columns and one halo pixel either side

template <typename T, int OCT>
__global__ __launch_bounds__(GT_W * OCT) void glu_dwconv3x3_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w9, const T* __restrict__ bias,
                                                                 T* __restrict__ out, int64_t ldo, int H, int W, int C, int xtiles) {
    using E = ElemT<T>;
    constexpr int NT = GT_W * OCT;
    constexpr int ITEMS = GT_PX * 2 * OCT;                 // 8-channel items of one ring row: pixel-major, then half, then octet
    constexpr int PER = (ITEMS + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) T ring[4][ITEMS][8];
    __shared__ __attribute__((aligned(16))) T wl[20][OCT][8];     // taps (tap, half) 0..17, then the two bias halves, of this group's channels
    const int tid = threadIdx.x;
    const int oc = tid % OCT, xi = tid / OCT;
    const int xt = blockIdx.x % xtiles, yt = blockIdx.x / xtiles;
    const int b = blockIdx.z;
    const int x0 = xt * GT_W, y0 = yt * GT_ROWS;
    const int yend = min(H, y0 + GT_ROWS);
    const int oct0 = blockIdx.y * OCT;
    const int c0 = (oct0 + oc) * 8;                        // this thread's channels (value half; the gate half is C further)
    const bool chan = c0 < C;                              // else a pad octet of the output row (c0 < ldo), or nothing
    const bool pad = !chan && c0 + 8 <= ldo;
    const T* xb = x + (int64_t)b * H * W * ldx;
    T* ob = out + (int64_t)b * H * W * ldo;

    if (tid < 20 * OCT) {
        const int o_ = tid % OCT, th = tid / OCT;                  // th = 2 tap + half; 18, 19: bias
        const int c = (oct0 + o_) * 8;
        float wv[8];
        if (c < C) E::load8((th < 18 ? w9 + (int64_t)(th >> 1) * 2 * C : bias) + (th & 1) * C + c, wv);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) wv[i] = 0.f;
        }
        E::store8(&wl[th][o_][0], wv);                             // an exact copy: the values are T already
    }
    float stage[PER][8];
    auto fetch = [&](int y) __attribute__((always_inline)) {       // row y of the image -> registers (zeros outside the image / the channels)
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int it = tid + p * NT;
            const int o_ = it % OCT, half = (it / OCT) & 1, px = x0 - 1 + it / (2 * OCT);
            const int c = (oct0 + o_) * 8;
            if (it < ITEMS && y >= 0 && y < H && px >= 0 && px < W && c < C)
                E::load8(xb + ((int64_t)y * W + px) * ldx + half * C + c, stage[p]);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) stage[p][i] = 0.f;
            }
        }
    };
    auto commit = [&](int slot) __attribute__((always_inline)) {   // a = silu(x), rounded as the activation's output; silu(0) = 0 keeps the padding
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int it = tid + p * NT;
            if (it < ITEMS) {
                float a[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = silu<T>(stage[p][i]);
                E::store8(&ring[slot][it][0], a);
            }
        }
    };

    const int px_ok = x0 + xi < W;
    const int nsteps = yend - y0 + 2;                      // input rows y0 - 1 .. yend
    fetch(y0 - 1);
    for (int s = 0; s < nsteps; ++s) {
        commit(s & 3);
        if (s + 1 < nsteps) fetch(y0 + s);
        __syncthreads();                                   // one barrier per row: the slot written next (s + 1) is not among the three read below
        if (s < 2) continue;
        const int yo = y0 + s - 2;
        if (!px_ok) continue;
        T* orow = ob + ((int64_t)yo * W + x0 + xi) * ldo + c0;
        if (chan) {
            float av[8], ag[8];
            E::load8(&wl[18][oc][0], av);
            E::load8(&wl[19][oc][0], ag);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int slot = (s - 2 + ky) & 3;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    float a[8], wv[8];
                    E::load8(&ring[slot][((xi + kx) * 2 + 0) * OCT + oc][0], a);
                    E::load8(&wl[2 * (ky * 3 + kx)][oc][0], wv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) av[i] = fmaf(a[i], wv[i], av[i]);
                    E::load8(&ring[slot][((xi + kx) * 2 + 1) * OCT + oc][0], a);
                    E::load8(&wl[2 * (ky * 3 + kx) + 1][oc][0], wv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) ag[i] = fmaf(a[i], wv[i], ag[i]);
                }
            }
            float r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = E::rnd(av[i]) * E::rnd(silu<T>(E::rnd(ag[i])));
            E::store8(orow, r);
        } else if (pad) {
            E::zero8(orow);
        }
    }
}

template <typename T>
int glu_dwconv3x3_impl(const char* who, const void* x, int64_t ldx, const void* w9, const void* bias, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W,
                       int64_t C, ug_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return UG_OK;
    UG_REQUIRE(x && w9 && bias && out && B > 0 && H > 0 && W > 0 && C > 0 && ldx >= 2 * C && ldo >= C, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(C % 8 == 0, UG_ERR_UNSUPPORTED, "%s: C = %lld is not a multiple of 8", who, (long long)C);
    UG_REQUIRE(ldx % 8 == 0 && ldo % 8 == 0 && ug_aligned(x, 16) && ug_aligned(w9, 16) && ug_aligned(bias, 16) && ug_aligned(out, 16), UG_ERR_BAD_ALIGN,
               "%s: row strides must be multiples of 8 elements and bases 16-byte aligned", who);
    UG_REQUIRE(H < (1 << 20) && W < (1 << 20) && ldx < (1 << 24) && ldo < (1 << 24) && B < 65536, UG_ERR_UNSUPPORTED, "%s: too large", who);
    constexpr int OCT = ElemT<T>::kF32 ? 4 : 8;
    const int xtiles = (int)((W + GT_W - 1) / GT_W);
    const int64_t tiles = (int64_t)xtiles * ((H + GT_ROWS - 1) / GT_ROWS);
    const int64_t ogroups = (ldo / 8 + OCT - 1) / OCT;
    UG_REQUIRE(tiles < (1ll << 31) && ogroups < 65536, UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    hipLaunchKernelGGL((glu_dwconv3x3_kernel<T, OCT>), dim3((unsigned)tiles, (unsigned)ogroups, (unsigned)B), dim3(GT_W * OCT), 0, (hipStream_t)stream,
                       (const T*)x, ldx, (const T*)w9, (const T*)bias, (T*)out, ldo, (int)H, (int)W, (int)C, xtiles);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

}  // namespace

extern "C" int64_t ug_linear_attn_workspace_bytes(int64_t batches, int64_t heads, int64_t N) {
    if (batches <= 0 || heads <= 0 || N <= 0) return 0;
    return batches * heads * (la_chunks(N) + 1) * LA_STATE * (int64_t)sizeof(float);
}

UG_TWINS(ug_linear_attn, linear_attn_impl,
         (const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
          int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride, int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace,
          ug_stream_t stream),
         (__func__, q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride, o_batch_stride, batches, heads,
          N, dh, workspace, stream))
UG_TWINS(ug_glu_dwconv3x3, glu_dwconv3x3_impl,
         (const void* x, int64_t ldx, const void* w9, const void* bias, void* out, int64_t ldo, int64_t B, int64_t H, int64_t W, int64_t C, ug_stream_t stream),
         (__func__, x, ldx, w9, bias, out, ldo, B, H, W, C, stream))
