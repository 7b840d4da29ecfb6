// The backward of the two Sana kernel classes of csrc/sana.hip (unigen_amd/autograd.py: LinearAttention, GluDwConv):
//   ug_linear_attn_bwd(_f32)      dq, dk, dv of the ReLU linear attention from q, k, v, dout and the forward's fp32 state
//   ug_glu_dwconv3x3_bwd(_f32)    dx (and fp32 dw9, dbias) of SiLU -> depthwise 3x3 -> SiLU gate
// Shipped correct and untuned, like the forward kernels (docs/KERNEL_NOTES.md, "Sana kernels"). Neither uses the matrix cores. No atomics: partial
// sums are written to the caller's workspace and added in one fixed order, so two calls give the same bits.
//
// ---- linear attention ----
// With q' = relu(q), k' = relu(k), per (batch, head), all fp32; S, z are the forward's state (S^T[j][d] | z[j], 1056 floats):
//   den[n] = z . q'[n] + 1e-15   o = S q' / den   g[n][d] = dout[n][d] / den[n]   c[n] = -(dout[n] . o[n]) / den[n]
//   dq'[n][j] = sum_d g[n][d] S[d][j] + c[n] z[j]            dS[d][j] = sum_n g[n][d] q'[n][j]      dz[j] = sum_n c[n] q'[n][j]
//   dk'[n][j] = sum_d v[n][d] dS[d][j] + dz[j]               dv[n][d] = sum_j dS[d][j] k'[n][j]     dq = dq' [q > 0], dk = dk' [k > 0]
// Three launches on the caller's workspace, every word of which is written before it is read in the same call:
//   linattn_bwd_q_kernel       one workgroup = LB_ROWS query rows x up to 4 adjacent heads. The heads' states sit in LDS in both orientations
//                              (S^T[j][d] for the output, S[d][j] for dq'). 16 rows at a time: thread (row, octet) recomputes 8 outputs and the
//                              denominator of its head as the forward's apply pass does, folds dout . o over the head's four lanes, leaves g and c in
//                              LDS, and computes its 8 columns of dq' (one rounding at the store). Then wave w adds the 16 rows' g^T q' and c q' of
//                              head w into its registers: lane (d, half) owns 16 entries of dS. -> partial[b][h][chunk] as dS[d][j] | dz[j]
//   linattn_bwd_reduce_kernel  partials summed over the chunks in ascending order -> dstate[b][h]
//   linattn_bwd_kv_kernel      one workgroup = LB_ROWS key rows x up to 4 heads, dS in LDS in both orientations; thread (row, octet): 8 columns of dk'
//                              and of dv, one rounding each at the store.
//
// ---- GLU depthwise convolution ----
// Per pixel p and channel c, recomputed exactly as the forward rounds them: a = rnd(silu(x)), y = rnd(dwconv(a) + bias) (bias first, then the nine
// taps in order, one fma each), s = rnd(silu(y_gate)). The gradient is that of the function as evaluated (roundings straight-through):
//   dy_val = rnd(dout s)   dy_gate = rnd(dout y_val silu'(y_gate))   da[p] = sum_t w9[t] dy[p - t]   dx = rnd(da silu'(x))
//   dw9[t] = sum_p dy[p] a[p + t]   dbias = sum_p dy[p]
// Direct kernels, one thread per (pixel, channel octet), the 3 x 3 window read through the caches (HBM sees every tensor about once):
//   glu_bwd_dy_kernel      both halves of one octet: y, s, dy -> dy [B H W][2C] in the workspace (rounded once, as T)
//   glu_bwd_dx_kernel      the transposed convolution of dy and the factor silu'(x)
//   glu_bwd_dw_kernel      only when dw9 / dbias are asked for: thread = one octet of the 2C channels, walks the GB_SLAB pixels of its slab in order
//                          with 9 x 8 + 8 fp32 accumulators -> partial[slab][10][2C]
//   glu_bwd_reduce_kernel  slabs added in ascending order -> dw9 [9][2C], dbias [2C]
#include "ug_common.h"

namespace {

constexpr int LB_DH = 32;                        // head width
constexpr int LB_HG = 4;                         // heads per workgroup: 128 columns
constexpr int LB_COLS = LB_HG * LB_DH;
constexpr int LB_ROWS = 128;                     // query rows (q pass) / key rows (kv pass) per workgroup; a partial dS per LB_ROWS query rows
constexpr int LB_SS = LB_DH * LB_DH;             // S: 1024 floats
constexpr int LB_STATE = LB_SS + LB_DH;          // S | z: 1056 floats
constexpr float LB_EPS = 1e-15f;

__host__ __device__ inline int64_t lb_chunks(int64_t N) { return (N + LB_ROWS - 1) / LB_ROWS; }

template <typename T>
__global__ __launch_bounds__(256) void linattn_bwd_q_kernel(const T* __restrict__ q, int64_t q_rs, int64_t q_bs, const T* __restrict__ dout, int64_t do_rs,
                                                            int64_t do_bs, T* __restrict__ dq, int64_t dq_rs, int64_t dq_bs, int heads, int64_t N, int nchunk,
                                                            const float* __restrict__ state, float* __restrict__ partial) {
    using E = ElemT<T>;
    __shared__ __attribute__((aligned(16))) float st[LB_HG][LB_STATE];     // S^T[j][d] | z[j]
    __shared__ __attribute__((aligned(16))) float sd[LB_HG][LB_SS];        // S[d][j]
    __shared__ __attribute__((aligned(16))) float qs[16][LB_COLS];
    __shared__ __attribute__((aligned(16))) float gs[16][LB_COLS];
    __shared__ float cs[16][LB_HG];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, hg = blockIdx.y, b = blockIdx.z;
    const int h0 = hg * LB_HG;
    const int nh = min(LB_HG, heads - h0);
    const float* sb = state + ((int64_t)b * heads + h0) * LB_STATE;
    for (int e = tid; e < nh * LB_STATE; e += 256) {
        const float val = sb[e];
        (&st[0][0])[e] = val;
        const int hl_ = e / LB_STATE, r = e - hl_ * LB_STATE;
        if (r < LB_SS) sd[hl_][(r & (LB_DH - 1)) * LB_DH + (r >> 5)] = val;
    }
    const int c8 = tid & 15, lr = tid >> 4;
    const int hl = c8 >> 2, d0 = (c8 & 3) * 8;             // this thread's head within the group and its 8 columns
    const bool col_ok = hl < nh;
    const T* qb = q + (int64_t)b * q_bs + h0 * LB_DH + c8 * 8;
    const T* dob = dout + (int64_t)b * do_bs + h0 * LB_DH + c8 * 8;
    T* dqb = dq + (int64_t)b * dq_bs + h0 * LB_DH + c8 * 8;
    const int wave = tid >> 6, lane = tid & 63;
    const int dd = lane >> 1, j0 = (lane & 1) * 16;        // accumulate: dS[dd][j0 .. j0 + 15] of head h0 + wave
    const int jz = lane & (LB_DH - 1);                     // and dz[jz] (both halves of the wave compute it, the lower one writes it)
    float acc[16], zacc = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int64_t r0 = (int64_t)chunk * LB_ROWS;
    for (int p = 0; p < LB_ROWS / 16; ++p) {
        if (r0 + 16 * p >= N) break;                       // uniform over the workgroup
        const int64_t n = r0 + 16 * p + lr;
        const bool live = col_ok && n < N;
        float qf[8], df[8];
        if (live) {
            E::load8(qb + n * q_rs, qf);
            E::load8(dob + n * do_rs, df);
        } else {                                           // past the rows or the group's heads: contributes nothing
#pragma unroll
            for (int i = 0; i < 8; ++i) { qf[i] = 0.f; df[i] = 0.f; }
        }
        __syncthreads();                                   // the previous pass has read qs, gs, cs
        *(f32x4*)&qs[lr][c8 * 8] = (f32x4){fmaxf(qf[0], 0.f), fmaxf(qf[1], 0.f), fmaxf(qf[2], 0.f), fmaxf(qf[3], 0.f)};
        *(f32x4*)&qs[lr][c8 * 8 + 4] = (f32x4){fmaxf(qf[4], 0.f), fmaxf(qf[5], 0.f), fmaxf(qf[6], 0.f), fmaxf(qf[7], 0.f)};
        __syncthreads();                                   // (first pass: st and sd are complete too)
        float g[8], dot = 0.f, den = 1.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = 0.f;
        if (live) {
            float num[8];
            den = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) num[i] = 0.f;
            const float* sh = st[hl];
#pragma unroll 2
            for (int j4 = 0; j4 < LB_DH / 4; ++j4) {
                const f32x4 qq = *(const f32x4*)&qs[lr][hl * LB_DH + 4 * j4];
                const f32x4 zz = *(const f32x4*)&sh[LB_SS + 4 * j4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float* sr = sh + (4 * j4 + jj) * LB_DH + d0;
                    const f32x4 s0 = *(const f32x4*)sr, s1 = *(const f32x4*)(sr + 4);
                    const float qv = qq[jj];
                    num[0] = fmaf(s0[0], qv, num[0]); num[1] = fmaf(s0[1], qv, num[1]); num[2] = fmaf(s0[2], qv, num[2]); num[3] = fmaf(s0[3], qv, num[3]);
                    num[4] = fmaf(s1[0], qv, num[4]); num[5] = fmaf(s1[1], qv, num[5]); num[6] = fmaf(s1[2], qv, num[6]); num[7] = fmaf(s1[3], qv, num[7]);
                    den = fmaf(zz[jj], qv, den);
                }
            }
            den += LB_EPS;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                g[i] = df[i] / den;
                dot = fmaf(df[i], num[i] / den, dot);
            }
        }
        dot += __shfl_xor(dot, 1, 64);                     // the head's four lanes are adjacent; every lane takes part
        dot += __shfl_xor(dot, 2, 64);
        const float c = live ? -dot / den : 0.f;
        *(f32x4*)&gs[lr][c8 * 8] = (f32x4){g[0], g[1], g[2], g[3]};
        *(f32x4*)&gs[lr][c8 * 8 + 4] = (f32x4){g[4], g[5], g[6], g[7]};
        if ((c8 & 3) == 0) cs[lr][hl] = c;
        __syncthreads();
        if (live) {                                        // dq'[n][d0 + i] = sum_d g[n][d] S[d][d0 + i] + c z[d0 + i]
            float r[8];
            const float* zrow = &st[hl][LB_SS + d0];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = c * zrow[i];
            const float* sh = sd[hl];
#pragma unroll 2
            for (int d4 = 0; d4 < LB_DH / 4; ++d4) {
                const f32x4 gg = *(const f32x4*)&gs[lr][hl * LB_DH + 4 * d4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* sr = sh + (4 * d4 + e) * LB_DH + d0;
                    const f32x4 s0 = *(const f32x4*)sr, s1 = *(const f32x4*)(sr + 4);
                    const float gv = gg[e];
                    r[0] = fmaf(gv, s0[0], r[0]); r[1] = fmaf(gv, s0[1], r[1]); r[2] = fmaf(gv, s0[2], r[2]); r[3] = fmaf(gv, s0[3], r[3]);
                    r[4] = fmaf(gv, s1[0], r[4]); r[5] = fmaf(gv, s1[1], r[5]); r[6] = fmaf(gv, s1[2], r[6]); r[7] = fmaf(gv, s1[3], r[7]);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = qf[i] > 0.f ? r[i] : 0.f;
            E::store8(dqb + n * dq_rs, r);
        }
        if (wave < nh) {                                   // dS += g^T q', dz += c q' over the 16 rows (rows past N hold zeros)
#pragma unroll 4
            for (int t = 0; t < 16; ++t) {
                const float gv = gs[t][wave * LB_DH + dd];
                const float* qr = &qs[t][wave * LB_DH + j0];
#pragma unroll
                for (int i4 = 0; i4 < 4; ++i4) {
                    const f32x4 qq = *(const f32x4*)(qr + 4 * i4);
                    acc[4 * i4 + 0] = fmaf(gv, qq[0], acc[4 * i4 + 0]); acc[4 * i4 + 1] = fmaf(gv, qq[1], acc[4 * i4 + 1]);
                    acc[4 * i4 + 2] = fmaf(gv, qq[2], acc[4 * i4 + 2]); acc[4 * i4 + 3] = fmaf(gv, qq[3], acc[4 * i4 + 3]);
                }
                zacc = fmaf(cs[t][wave], qs[t][wave * LB_DH + jz], zacc);
            }
        }
    }
    if (wave < nh) {
        float* out = partial + (((int64_t)b * heads + h0 + wave) * nchunk + chunk) * LB_STATE;
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
            *(f32x4*)(out + dd * LB_DH + j0 + 4 * i4) = (f32x4){acc[4 * i4], acc[4 * i4 + 1], acc[4 * i4 + 2], acc[4 * i4 + 3]};
        if (lane < LB_DH) out[LB_SS + lane] = zacc;
    }
}

// dstate[bh] = sum over chunks (ascending) of partial[bh][chunk], as dS[d][j] | dz[j]
__global__ __launch_bounds__(256) void linattn_bwd_reduce_kernel(const float* __restrict__ partial, int nchunk, float* __restrict__ dstate) {
    const int64_t bh = blockIdx.x;
    const float* p = partial + bh * nchunk * LB_STATE;
    float* s = dstate + bh * LB_STATE;
    for (int e = threadIdx.x; e < LB_STATE; e += 256) {
        float a = 0.f;
        for (int c = 0; c < nchunk; ++c) a += p[(int64_t)c * LB_STATE + e];
        s[e] = a;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void linattn_bwd_kv_kernel(const T* __restrict__ k, int64_t k_rs, int64_t k_bs, const T* __restrict__ v, int64_t v_rs,
                                                             int64_t v_bs, T* __restrict__ dk, int64_t dk_rs, int64_t dk_bs, T* __restrict__ dv, int64_t dv_rs,
                                                             int64_t dv_bs, int heads, int64_t N, const float* __restrict__ dstate) {
    using E = ElemT<T>;
    __shared__ __attribute__((aligned(16))) float sdj[LB_HG][LB_STATE];    // dS[d][j] | dz[j]
    __shared__ __attribute__((aligned(16))) float sjd[LB_HG][LB_SS];       // dS^T[j][d]
    __shared__ __attribute__((aligned(16))) float ks[16][LB_COLS];
    __shared__ __attribute__((aligned(16))) float vs[16][LB_COLS];
    const int tid = threadIdx.x;
    const int hg = blockIdx.y, b = blockIdx.z;
    const int h0 = hg * LB_HG;
    const int nh = min(LB_HG, heads - h0);
    const float* sb = dstate + ((int64_t)b * heads + h0) * LB_STATE;
    for (int e = tid; e < nh * LB_STATE; e += 256) {
        const float val = sb[e];
        (&sdj[0][0])[e] = val;
        const int hl_ = e / LB_STATE, r = e - hl_ * LB_STATE;
        if (r < LB_SS) sjd[hl_][(r & (LB_DH - 1)) * LB_DH + (r >> 5)] = val;
    }
    const int c8 = tid & 15, lr = tid >> 4;
    const int hl = c8 >> 2, d0 = (c8 & 3) * 8;
    const bool col_ok = hl < nh;
    const int64_t co = h0 * LB_DH + c8 * 8;
    const T* kb = k + (int64_t)b * k_bs + co;
    const T* vb = v + (int64_t)b * v_bs + co;
    T* dkb = dk + (int64_t)b * dk_bs + co;
    T* dvb = dv + (int64_t)b * dv_bs + co;
    const int64_t r0 = (int64_t)blockIdx.x * LB_ROWS;
    for (int p = 0; p < LB_ROWS / 16; ++p) {
        if (r0 + 16 * p >= N) break;                       // uniform over the workgroup
        const int64_t n = r0 + 16 * p + lr;
        const bool live = col_ok && n < N;
        float kf[8], vf[8];
        if (live) {
            E::load8(kb + n * k_rs, kf);
            E::load8(vb + n * v_rs, vf);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) { kf[i] = 0.f; vf[i] = 0.f; }
        }
        __syncthreads();                                   // the previous pass has read ks, vs
        *(f32x4*)&ks[lr][c8 * 8] = (f32x4){fmaxf(kf[0], 0.f), fmaxf(kf[1], 0.f), fmaxf(kf[2], 0.f), fmaxf(kf[3], 0.f)};
        *(f32x4*)&ks[lr][c8 * 8 + 4] = (f32x4){fmaxf(kf[4], 0.f), fmaxf(kf[5], 0.f), fmaxf(kf[6], 0.f), fmaxf(kf[7], 0.f)};
        *(f32x4*)&vs[lr][c8 * 8] = (f32x4){vf[0], vf[1], vf[2], vf[3]};
        *(f32x4*)&vs[lr][c8 * 8 + 4] = (f32x4){vf[4], vf[5], vf[6], vf[7]};
        __syncthreads();                                   // (first pass: sdj and sjd are complete too)
        if (live) {
            float rk[8], rv[8];
            const float* zrow = &sdj[hl][LB_SS + d0];
#pragma unroll
            for (int i = 0; i < 8; ++i) { rk[i] = zrow[i]; rv[i] = 0.f; }
            const float* a = sdj[hl];
            const float* at = sjd[hl];
#pragma unroll 2
            for (int e4 = 0; e4 < LB_DH / 4; ++e4) {
                const f32x4 vv = *(const f32x4*)&vs[lr][hl * LB_DH + 4 * e4];
                const f32x4 kk = *(const f32x4*)&ks[lr][hl * LB_DH + 4 * e4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* ar = a + (4 * e4 + e) * LB_DH + d0;           // dS[d = 4 e4 + e][d0 ..]: dk'[j = d0 + i] += v[d] dS[d][j]
                    const f32x4 s0 = *(const f32x4*)ar, s1 = *(const f32x4*)(ar + 4);
                    const float x = vv[e];
                    rk[0] = fmaf(x, s0[0], rk[0]); rk[1] = fmaf(x, s0[1], rk[1]); rk[2] = fmaf(x, s0[2], rk[2]); rk[3] = fmaf(x, s0[3], rk[3]);
                    rk[4] = fmaf(x, s1[0], rk[4]); rk[5] = fmaf(x, s1[1], rk[5]); rk[6] = fmaf(x, s1[2], rk[6]); rk[7] = fmaf(x, s1[3], rk[7]);
                    const float* tr = at + (4 * e4 + e) * LB_DH + d0;          // dS^T[j = 4 e4 + e][d0 ..]: dv[d = d0 + i] += k'[j] dS[d][j]
                    const f32x4 t0 = *(const f32x4*)tr, t1 = *(const f32x4*)(tr + 4);
                    const float y = kk[e];
                    rv[0] = fmaf(y, t0[0], rv[0]); rv[1] = fmaf(y, t0[1], rv[1]); rv[2] = fmaf(y, t0[2], rv[2]); rv[3] = fmaf(y, t0[3], rv[3]);
                    rv[4] = fmaf(y, t1[0], rv[4]); rv[5] = fmaf(y, t1[1], rv[5]); rv[6] = fmaf(y, t1[2], rv[6]); rv[7] = fmaf(y, t1[3], rv[7]);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) rk[i] = kf[i] > 0.f ? rk[i] : 0.f;
            E::store8(dkb + n * dk_rs, rk);
            E::store8(dvb + n * dv_rs, rv);
        }
    }
}

template <typename T>
int linear_attn_bwd_impl(const char* who, ug_view q, ug_view k, ug_view v, ug_view dout, const float* state, ug_view dq, ug_view dk, ug_view dv, int64_t batches,
                         int32_t heads, int64_t N, int32_t dh, void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    if (batches == 0 || N == 0) return UG_OK;
    UG_REQUIRE(q.p && k.p && v.p && dout.p && dq.p && dk.p && dv.p && workspace && batches > 0 && heads > 0 && N > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(state, UG_ERR_BAD_SHAPE, "%s: state (what ug_linear_attn left at the start of its workspace) is required; there is no recompute path", who);
    UG_REQUIRE(dh == LB_DH, UG_ERR_UNSUPPORTED, "%s: head dim %d is not 32", who, dh);
    constexpr int A = ElemT<T>::kF32 ? 4 : 8;              // elements of 16 bytes
    const ug_view_rule views[] = {{"q", q, A, 16, false},   {"k", k, A, 16, false},   {"v", v, A, 16, false},   {"dout", dout, A, 16, false},
                                  {"dq", dq, A, 16, false}, {"dk", dk, A, 16, false}, {"dv", dv, A, 16, false}, {"state", {state, 0, 0}, A, 16, false},
                                  {"workspace", {workspace, 0, 0}, A, 16, false}};
    if (const int rc = ug_check_views(who, views)) return rc;
    // grid limits: y = head groups and z = batches below 65536; the reduce pass has one workgroup per (batch, head) on x
    UG_REQUIRE(N < (1ll << 30) && batches < 65536 && (heads + LB_HG - 1) / LB_HG < 65536 && batches * (int64_t)heads < (1ll << 31), UG_ERR_UNSUPPORTED,
               "%s: too large", who);
    const int nchunk = (int)lb_chunks(N);
    const int64_t need = batches * heads * ((int64_t)nchunk + 1) * LB_STATE * (int64_t)sizeof(float);
    UG_REQUIRE(workspace_bytes >= need, UG_ERR_BAD_SHAPE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
    const unsigned ngroups = (unsigned)((heads + LB_HG - 1) / LB_HG);
    float* dstate = (float*)workspace;
    float* partial = dstate + batches * heads * LB_STATE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nchunk, ngroups, (unsigned)batches);
    hipLaunchKernelGGL(linattn_bwd_q_kernel<T>, grid, dim3(256), 0, s, (const T*)q.p, q.rs, q.bs, (const T*)dout.p, dout.rs, dout.bs, (T*)dq.p, dq.rs, dq.bs,
                       (int)heads, N, nchunk, state, partial);
    UG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(linattn_bwd_reduce_kernel, dim3((unsigned)(batches * heads)), dim3(256), 0, s, (const float*)partial, nchunk, dstate);
    UG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(linattn_bwd_kv_kernel<T>, grid, dim3(256), 0, s, (const T*)k.p, k.rs, k.bs, (const T*)v.p, v.rs, v.bs, (T*)dk.p, dk.rs, dk.bs, (T*)dv.p,
                       dv.rs, dv.bs, (int)heads, N, (const float*)dstate);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

// ---- GLU depthwise 3x3 ----
constexpr int GB_SLAB = 256;                     // pixels per partial sum of dw9 / dbias

// a, y and s must be the forward's bits: silu<T> (ug_common.h) is the function the forward calls
template <typename T> __device__ __forceinline__ float dsilu_b(float x) {
    const float s = sigmoid<T>(x);
    return s * (1.0f + x * (1.0f - s));
}

__host__ __device__ inline int64_t gb_slabs(int64_t pixels) { return (pixels + GB_SLAB - 1) / GB_SLAB; }
__host__ __device__ inline int64_t gb_dy_bytes(int64_t pixels, int64_t C, int64_t elem) { return (pixels * 2 * C * elem + 15) / 16 * 16; }

template <typename T>
__global__ __launch_bounds__(256) void glu_bwd_dy_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w9, const T* __restrict__ bias,
                                                         const T* __restrict__ dout, int64_t lddo, T* __restrict__ dy, int H, int W, int C, int64_t items) {
    using E = ElemT<T>;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int oc = C / 8;
    const int64_t p = idx / oc;                            // pixel, over [B][H][W]
    const int c = (int)(idx - p * oc) * 8;
    const int xw = (int)(p % W), y = (int)((p / W) % H);
    float av[8], ag[8];
    E::load8(bias + c, av);
    E::load8(bias + C + c, ag);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = xw + kx - 1;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            float a[8], g[8], wv[8];
            if (in) {
                const T* xp = x + (p + (int64_t)(ky - 1) * W + (kx - 1)) * ldx + c;
                E::load8(xp, a);
                E::load8(xp + C, g);
#pragma unroll
                for (int i = 0; i < 8; ++i) { a[i] = E::rnd(silu<T>(a[i])); g[i] = E::rnd(silu<T>(g[i])); }
            } else {                                       // the convolution's zero padding acts on the activation
#pragma unroll
                for (int i = 0; i < 8; ++i) { a[i] = 0.f; g[i] = 0.f; }
            }
            E::load8(w9 + (int64_t)(ky * 3 + kx) * 2 * C + c, wv);
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = fmaf(a[i], wv[i], av[i]);
            E::load8(w9 + (int64_t)(ky * 3 + kx) * 2 * C + C + c, wv);
#pragma unroll
            for (int i = 0; i < 8; ++i) ag[i] = fmaf(g[i], wv[i], ag[i]);
        }
    }
    float gd[8];
    E::load8(dout + p * lddo + c, gd);
    float rv[8], rg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float yv = E::rnd(av[i]), yg = E::rnd(ag[i]);
        const float s = E::rnd(silu<T>(yg));
        rv[i] = gd[i] * s;
        rg[i] = gd[i] * yv * dsilu_b<T>(yg);
    }
    E::store8(dy + p * 2 * C + c, rv);                     // the one rounding of dy
    E::store8(dy + p * 2 * C + C + c, rg);
}

template <typename T>
__global__ __launch_bounds__(256) void glu_bwd_dx_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w9, const T* __restrict__ dy,
                                                         T* __restrict__ dx, int64_t lddx, int H, int W, int C, int64_t items) {
    using E = ElemT<T>;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    const int oc = 2 * C / 8;
    const int64_t p = idx / oc;
    const int c = (int)(idx - p * oc) * 8;                 // over both halves
    const int xw = (int)(p % W), y = (int)((p / W) % H);
    float da[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) da[i] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y - (ky - 1), xx = xw - (kx - 1);          // the output pixel that read this one through tap (ky, kx)
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                float g[8], wv[8];
                E::load8(dy + (p - (int64_t)(ky - 1) * W - (kx - 1)) * 2 * C + c, g);
                E::load8(w9 + (int64_t)(ky * 3 + kx) * 2 * C + c, wv);
#pragma unroll
                for (int i = 0; i < 8; ++i) da[i] = fmaf(g[i], wv[i], da[i]);
            }
        }
    }
    float xv[8], r[8];
    E::load8(x + p * ldx + c, xv);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = da[i] * dsilu_b<T>(xv[i]);
    E::store8(dx + p * lddx + c, r);
}

template <typename T>
__global__ __launch_bounds__(64) void glu_bwd_dw_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ dy, float* __restrict__ partial, int H, int W,
                                                        int C, int64_t pixels) {
    using E = ElemT<T>;
    const int item = blockIdx.y * 64 + threadIdx.x;
    if (item >= 2 * C / 8) return;
    const int c = item * 8;
    const int64_t slab = blockIdx.x;
    const int64_t q0 = slab * GB_SLAB, q1 = min(pixels, q0 + GB_SLAB);
    int xw = (int)(q0 % W), y = (int)((q0 / W) % H);
    float acc[9][8], bacc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        bacc[i] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t][i] = 0.f;
    }
    for (int64_t q = q0; q < q1; ++q) {
        float a[8], gc[8];
        E::load8(x + q * ldx + c, a);
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = E::rnd(silu<T>(a[i]));
        E::load8(dy + q * 2 * C + c, gc);
#pragma unroll
        for (int i = 0; i < 8; ++i) bacc[i] += gc[i];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y - (ky - 1), xx = xw - (kx - 1);      // dw9[t] += dy[p] a[q], p the output pixel that read q through tap t
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    float g[8];
                    if (ky != 1 || kx != 1) E::load8(dy + (q - (int64_t)(ky - 1) * W - (kx - 1)) * 2 * C + c, g);
                    else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) g[i] = gc[i];
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[ky * 3 + kx][i] = fmaf(g[i], a[i], acc[ky * 3 + kx][i]);
                }
            }
        }
        if (++xw == W) { xw = 0; if (++y == H) y = 0; }
    }
    float* out = partial + slab * 10 * 2 * C + c;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        *(f32x4*)(out + (int64_t)t * 2 * C) = (f32x4){acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
        *(f32x4*)(out + (int64_t)t * 2 * C + 4) = (f32x4){acc[t][4], acc[t][5], acc[t][6], acc[t][7]};
    }
    *(f32x4*)(out + (int64_t)9 * 2 * C) = (f32x4){bacc[0], bacc[1], bacc[2], bacc[3]};
    *(f32x4*)(out + (int64_t)9 * 2 * C + 4) = (f32x4){bacc[4], bacc[5], bacc[6], bacc[7]};
}

// dw9[e] (e < n9) / dbias[e - n9] = sum over slabs (ascending) of partial[slab][e]
__global__ __launch_bounds__(256) void glu_bwd_reduce_kernel(const float* __restrict__ partial, int64_t nslab, int64_t n9, int64_t n10, float* __restrict__ dw9,
                                                             float* __restrict__ dbias) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n10) return;
    float a = 0.f;
    for (int64_t s = 0; s < nslab; ++s) a += partial[s * n10 + e];
    if (e < n9) dw9[e] = a;
    else dbias[e - n9] = a;
}

template <typename T>
int glu_dwconv3x3_bwd_impl(const char* who, const void* x, int64_t ldx, const void* w9, const void* bias, const void* dout, int64_t lddo, void* dx, int64_t lddx,
                           float* dw9, float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return UG_OK;
    UG_REQUIRE(x && w9 && bias && dout && dx && workspace && B > 0 && H > 0 && W > 0 && C > 0 && ldx >= 2 * C && lddo >= C && lddx >= 2 * C, UG_ERR_BAD_SHAPE,
               "%s: bad arguments", who);
    UG_REQUIRE((dw9 == nullptr) == (dbias == nullptr), UG_ERR_BAD_SHAPE, "%s: dw9 and dbias are both given or both NULL", who);
    UG_REQUIRE(C % 8 == 0, UG_ERR_UNSUPPORTED, "%s: C = %lld is not a multiple of 8", who, (long long)C);
    UG_REQUIRE(ldx % 8 == 0 && lddo % 8 == 0 && lddx % 8 == 0 && ug_aligned(x, 16) && ug_aligned(w9, 16) && ug_aligned(bias, 16) && ug_aligned(dout, 16) &&
               ug_aligned(dx, 16) && ug_aligned(dw9, 16) && ug_aligned(dbias, 16) && ug_aligned(workspace, 16), UG_ERR_BAD_ALIGN,
               "%s: row strides must be multiples of 8 elements and bases 16-byte aligned", who);
    UG_REQUIRE(H < (1 << 20) && W < (1 << 20) && ldx < (1 << 24) && lddo < (1 << 24) && lddx < (1 << 24) && B < 65536, UG_ERR_UNSUPPORTED, "%s: too large", who);
    const int64_t pixels = B * H * W;
    const int64_t items = pixels * (2 * C / 8);
    const int64_t nslab = gb_slabs(pixels);
    const int64_t cgroups = (2 * C / 8 + 63) / 64;
    UG_REQUIRE((items + 255) / 256 < (1ll << 31) && nslab < (1ll << 31) && cgroups < 65536, UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    const int64_t dy_bytes = gb_dy_bytes(pixels, C, (int64_t)sizeof(T));
    const int64_t need = dy_bytes + nslab * 10 * 2 * C * (int64_t)sizeof(float);
    UG_REQUIRE(workspace_bytes >= need, UG_ERR_BAD_SHAPE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
    T* dy = (T*)workspace;
    float* partial = (float*)((char*)workspace + dy_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int64_t items_dy = pixels * (C / 8);
    hipLaunchKernelGGL(glu_bwd_dy_kernel<T>, dim3((unsigned)((items_dy + 255) / 256)), dim3(256), 0, s, (const T*)x, ldx, (const T*)w9, (const T*)bias,
                       (const T*)dout, lddo, dy, (int)H, (int)W, (int)C, items_dy);
    UG_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(glu_bwd_dx_kernel<T>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const T*)x, ldx, (const T*)w9, (const T*)dy, (T*)dx, lddx,
                       (int)H, (int)W, (int)C, items);
    UG_CHECK_LAUNCH(who);
    if (dw9) {
        hipLaunchKernelGGL(glu_bwd_dw_kernel<T>, dim3((unsigned)nslab, (unsigned)cgroups), dim3(64), 0, s, (const T*)x, ldx, (const T*)dy, partial, (int)H, (int)W,
                           (int)C, pixels);
        UG_CHECK_LAUNCH(who);
        const int64_t n10 = 10 * 2 * C;
        hipLaunchKernelGGL(glu_bwd_reduce_kernel, dim3((unsigned)((n10 + 255) / 256)), dim3(256), 0, s, (const float*)partial, nslab, 9 * 2 * C, n10, dw9, dbias);
        UG_CHECK_LAUNCH(who);
    }
    return UG_OK;
}

}  // namespace

extern "C" int64_t ug_linear_attn_bwd_workspace_bytes(int64_t batches, int64_t heads, int64_t N) {
    if (batches <= 0 || heads <= 0 || N <= 0) return 0;
    return batches * heads * (lb_chunks(N) + 1) * LB_STATE * (int64_t)sizeof(float);
}

#define UG_LAB_PARAMS (const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,              \
                       const void* v, int64_t v_row_stride, int64_t v_batch_stride, const void* dout, int64_t do_row_stride, int64_t do_batch_stride,           \
                       const float* state, void* dq, int64_t dq_row_stride, int64_t dq_batch_stride, void* dk, int64_t dk_row_stride, int64_t dk_batch_stride, \
                       void* dv, int64_t dv_row_stride, int64_t dv_batch_stride, int64_t batches, int32_t heads, int64_t N, int32_t dh, void* workspace,       \
                       int64_t workspace_bytes, ug_stream_t stream)
UG_TWINS(ug_linear_attn_bwd, linear_attn_bwd_impl, UG_LAB_PARAMS,
         (__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), {dout, do_row_stride, do_batch_stride}, state, UG_VIEW(dq), UG_VIEW(dk), UG_VIEW(dv), batches, heads, N, dh,
          workspace, workspace_bytes, stream))
#undef UG_LAB_PARAMS

extern "C" int64_t ug_glu_dwconv3x3_bwd_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int32_t elem_bytes) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (elem_bytes != 2 && elem_bytes != 4)) return 0;
    return gb_dy_bytes(B * H * W, C, elem_bytes) + gb_slabs(B * H * W) * 10 * 2 * C * (int64_t)sizeof(float);
}

#define UG_GB_PARAMS (const void* x, int64_t ldx, const void* w9, const void* bias, const void* dout, int64_t lddo, void* dx, int64_t lddx, float* dw9,    \
                      float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, void* workspace, int64_t workspace_bytes, ug_stream_t stream)
UG_TWINS(ug_glu_dwconv3x3_bwd, glu_dwconv3x3_bwd_impl, UG_GB_PARAMS,
         (__func__, x, ldx, w9, bias, dout, lddo, dx, lddx, dw9, dbias, B, H, W, C, workspace, workspace_bytes, stream))
#undef UG_GB_PARAMS
