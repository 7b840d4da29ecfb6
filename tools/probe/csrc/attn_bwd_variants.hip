// Attention backward: the forms that were built, measured and dropped. PROBE LIBRARY ONLY (python -m unigen_amd.build --probe); the product's
// backward is attn_bwd_kernel<DH, DQ> + attn_bwd_dkv_kernel + attn_bwd_dq_kernel in unigen_amd/csrc/attention.hip, whose dispatcher offers every
// stage (statistics, dQ, dK / dV) to ug_attn_bwd_variants() below in a probe build.
//   attn_bwd_var_kernel   the FROZEN four-mode, two-staging template the product's attn_bwd_kernel was cut from: one kernel on the forward's tiling, a
//                         workgroup OWNS 256 rows of one side and STREAMS 64-row tiles of the other;
//                           LSE : owns queries,  streams K       : S^T = K Q^T                         -> lse2[q] = log2 sum_k 2^(c S)
//                           DQ  : owns queries,  streams K, V    : S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta)  -> dQ^T += K^T dS^T, x scale at the end
//                           DK  : owns keys,     streams Q, dO   : S   = Q K^T, dP   = dO V^T, dS   = P   (dP   - delta)  -> dK^T += Q^T dS,     x scale at the end
//                           DV  : owns keys,     streams Q, dO   : S   = Q K^T, P                                               -> dV^T += dO^T P
//                         lse / delta are per lane when queries are owned and per accumulator row when they are streamed (their 64 values per tile
//                         ride along with the LDS-DMAs into the 512-byte slot behind the two tile images). DMA = false is register staging (HBM ->
//                         registers -> LDS, issue early, write late). Instantiated here: the DK and DV modes in both staging forms (the fused
//                         attn_bwd_dkv_kernel replaced them: dh 128 605 -> 711 TFLOP/s, same bits, profiles/r03y_attn_bwd_fuse_*.log) and the LSE and DQ
//                         modes with register staging (profiles/r02b_attn_dma.log); <LSE | DQ, true> is the product kernel itself.
//                         A change to the shipped kernel is NOT mirrored here: this copy is what the recorded A/B numbers were measured on.
// UG_ATTN_BWD_DMA=0 takes all three stages to the register-staged forms (which also switches the fused and the pair-scheme kernels off);
// UG_ATTN_BWD_FUSE_DKV=0 sends only dK / dV to the two separate modes. Same bits as the product in every combination but the dQ kernel choice.
#include "ug_common.h"
#include "attn_common.h"
#include <type_traits>

namespace {

enum { BWD_LSE = 0, BWD_DQ = 1, BWD_DK = 2, BWD_DV = 3 };

template <int DH, int MODE, bool DMA>
__global__ __launch_bounds__(512, 2) void attn_bwd_var_kernel(
    const bf16_t* __restrict__ own1, int64_t o1_rs, int64_t o1_bs, const bf16_t* __restrict__ own2, int64_t o2_rs, int64_t o2_bs,
    const bf16_t* __restrict__ st1, int64_t s1_rs, int64_t s1_bs, const bf16_t* __restrict__ st2, int64_t s2_rs, int64_t s2_bs,
    float* __restrict__ lse2, const float* __restrict__ delta, int64_t stat_ld /* queries per (b, h) row of lse2 / delta */,
    bf16_t* __restrict__ out, int64_t out_rs, int64_t out_bs, int heads, int Lown, int Lst, int nOwn, float c, float scale) {
    constexpr int RB = 2 * DH, NCH = DH / 8, TILE = KVB * RB, QS = DH / 16, NDB = DH / 32, NT = 512, NST = (KVB * NCH) / NT;
    constexpr bool OWN_Q = MODE == BWD_LSE || MODE == BWD_DQ;          // queries owned (statistics lane-local) or streamed
    constexpr bool TWO = MODE == BWD_DQ || MODE == BWD_DK;             // second score-like product (dP)
    constexpr int BUFSZ = 2 * TILE + (DMA ? 512 : 0);                      // DMA: + lse2[64] | delta[64] of the streamed rows (queries streamed)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][tile of st1 | tile of st2 (| statistics)]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int ot = blockIdx.x % nOwn, bh = blockIdx.x / nOwn;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* O1 = own1 + (int64_t)b * o1_bs + head * DH;
    const bf16_t* O2 = TWO ? own2 + (int64_t)b * o2_bs + head * DH : nullptr;
    const bf16_t* S1 = st1 + (int64_t)b * s1_bs + head * DH;
    const bf16_t* S2 = (MODE != BWD_LSE) ? st2 + (int64_t)b * s2_bs + head * DH : nullptr;
    const int own_row = ot * 256 + wave * 32 + r;
    const int own_ld = own_row < Lown ? own_row : Lown - 1;
    bf16x8 f1[QS], f2[TWO ? QS : 1];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        f1[s] = *(const bf16x8*)(O1 + (int64_t)own_ld * o1_rs + 16 * s + 8 * h);
        if constexpr (TWO) f2[s] = *(const bf16x8*)(O2 + (int64_t)own_ld * o2_rs + 16 * s + 8 * h);
    }
    const float* stat_l = lse2 + (int64_t)bh * stat_ld;
    const float* stat_d = (MODE == BWD_DQ || MODE == BWD_DK) ? delta + (int64_t)bh * stat_ld : nullptr;
    float my_lse = 0.f, my_delta = 0.f;
    if constexpr (MODE == BWD_DQ) { my_lse = stat_l[own_ld]; my_delta = stat_d[own_ld]; }
    // staging: thread -> NST chunks of each streamed tile
    int st_row[NST], st_ch[NST], st_off[NST];
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const int cid = tid + NT * u;
        st_row[u] = cid / NCH; st_ch[u] = cid % NCH;
        st_off[u] = img_off<DH>(st_row[u], st_ch[u]);
    }
    u32x4 r1[DMA ? 1 : NST], r2[DMA ? 1 : NST];
    // LDS-DMA staging (DMA): a tile image is NI runs of 1 KiB (RPI rows each), wave w owns runs w * NIW .. + NIW - 1 of both streamed tiles; the
    // DMAs of tile t + 1 are issued at the top of tile t and waited for (vmcnt(0)) ahead of the barrier that ends it - no staging registers,
    // no ds_write. The swizzle is applied on the source side as in the forward.
    constexpr int RPI = 1024 / RB, NI = TILE / 1024, NIW = NI / 8;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    unsigned d1o[NIW], d2o[NIW];
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int row = (wv * NIW + u) * RPI + lane / NCH;
        const int ch = (lane % NCH) ^ row_swz<DH>(row);
        d1o[u] = (unsigned)(row * (int)s1_rs + ch * 8) * 2u;
        d2o[u] = (unsigned)(row * (int)s2_rs + ch * 8) * 2u;
    }
    auto dma_stream = [&](const bf16_t* base, int64_t rs, const unsigned (&off)[NIW], int row0, unsigned dst) {
        if (row0 + KVB <= Lst) {
            const void* tb = uniform_ptr(base + (int64_t)row0 * rs);
#pragma unroll
            for (int u = 0; u < NIW; ++u) glds16_off(tb, off[u], dst + u * 1024);
        } else {                                       // ragged last tile: rows past the end re-read the last row (masked below)
            int lane_r = lane;
            asm volatile("" : "+v"(lane_r));
#pragma unroll
            for (int u = 0; u < NIW; ++u) {
                const int row = (wv * NIW + u) * RPI + lane_r / NCH;
                const int ch = (lane_r % NCH) ^ row_swz<DH>(row);
                int sr = row0 + row; if (sr > Lst - 1) sr = Lst - 1;
                glds16_ptr(base + (int64_t)sr * rs + ch * 8, dst + u * 1024);
            }
        }
    };
    auto stage_load = [&](int row0, int buf) {
        if constexpr (DMA) {
            const unsigned lb = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + buf * BUFSZ, l0 = lb + wv * NIW * 1024;
            dma_stream(S1, s1_rs, d1o, row0, l0);
            if constexpr (MODE != BWD_LSE) dma_stream(S2, s2_rs, d2o, row0, l0 + TILE);
            if constexpr (!OWN_Q) {                    // the tile's 64 lse2 / delta values ride along (rows padded to a multiple of 64, zeros)
                if (wv == 0) glds4_ptr(stat_l + row0 + lane, lb + 2 * TILE);
                if (MODE == BWD_DK && wv == 1) glds4_ptr(stat_d + row0 + lane, lb + 2 * TILE + 256);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NST; ++u) {
                int row = row0 + st_row[u]; if (row > Lst - 1) row = Lst - 1;
                r1[u] = *(const u32x4*)(S1 + (int64_t)row * s1_rs + st_ch[u] * 8);
                if constexpr (MODE != BWD_LSE) r2[u] = *(const u32x4*)(S2 + (int64_t)row * s2_rs + st_ch[u] * 8);
            }
        }
    };
    auto stage_write = [&](int buf) {
        if constexpr (DMA) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
#pragma unroll
            for (int u = 0; u < NST; ++u) {
                *(u32x4*)(smem + buf * BUFSZ + st_off[u]) = r1[u];
                if constexpr (MODE != BWD_LSE) *(u32x4*)(smem + buf * BUFSZ + TILE + st_off[u]) = r2[u];
            }
        }
    };
    // per-lane LDS read offsets: every swizzled offset is BASE ^ constant, re-derived from opaque copies of three bases (no per-fragment registers)
    const int k_base = RB * r + 16 * (h ^ row_swz<DH>(r));                 // row fragment s of 32-row block kb: kb * 32 * RB + (k_base ^ 32 s)
    const int i16 = lane & 15, g16 = lane >> 4;
    const int t_key = 4 * h + (i16 >> 2), t_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1), t_b8 = 8 * (i16 & 1);
    const int tlo_base = RB * t_key + 16 * (t_lowch ^ row_swz<DH>(t_key)) + t_b8;              // d-block db, k-step ks: ks * 16 * RB + (base ^ 64 db)
    const int thi_base = RB * (t_key + 8) + 16 * (t_lowch ^ row_swz<DH>(t_key + 8)) + t_b8;
    // dh 128: the LDS reads of each matrix phase are software-pipelined by hand - the fragments of step j + PD are requested before the MFMAs
    // of step j (left to hipcc every MFMA pair sits right behind its own ds_read and s_waitcnt): 527 -> 548 TFLOP/s. At dh 64 (half the MFMAs
    // per read burst) the same pipeline measured 6 % slower than hipcc's order, which stays.
    constexpr bool PIPE = DH == 128;
    constexpr int PDS = 3, PDA = 1;
    f32x16 acc[MODE == BWD_LSE ? 1 : NDB];
    if constexpr (MODE != BWD_LSE) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[db][i] = 0.f;
    }
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (Lst + KVB - 1) / KVB;
    stage_load(0, 0);
    stage_write(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage_load((t + 1) * KVB, cur ^ 1);
        const unsigned char* B1 = smem + cur * BUFSZ;
        const unsigned char* B2 = B1 + TILE;
        bf16x8 zf[2][2];
        float tmax = -INFINITY;
        f32x16 x1k[MODE == BWD_LSE ? 2 : 1];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 x1, x2;
#pragma unroll
            for (int i = 0; i < 16; ++i) { x1[i] = 0.f; x2[i] = 0.f; }
            if constexpr (PIPE) {
                int kb0 = k_base;
                asm volatile("" : "+v"(kb0));
                bf16x8 ab[PDS + 1][2];
                auto rd = [&](int s5) {
                    ab[s5 % (PDS + 1)][0] = *(const bf16x8*)(B1 + kb * 32 * RB + (kb0 ^ (32 * s5)));
                    if constexpr (TWO) ab[s5 % (PDS + 1)][1] = *(const bf16x8*)(B2 + kb * 32 * RB + (kb0 ^ (32 * s5)));
                };
#pragma unroll
                for (int j = 0; j < PDS && j < QS; ++j) rd(j);
#pragma unroll
                for (int s5 = 0; s5 < QS; ++s5) {
                    if (s5 + PDS < QS) rd(s5 + PDS);
                    __builtin_amdgcn_sched_barrier(0);
                    x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][0], f1[s5], x1, 0, 0, 0);
                    if constexpr (TWO) x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][1], f2[s5], x2, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int s5 = 0; s5 < QS; ++s5) {
                    const bf16x8 a1 = *(const bf16x8*)(B1 + kb * 32 * RB + (k_base ^ (32 * s5)));
                    x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, f1[s5], x1, 0, 0, 0);
                    if constexpr (TWO) {
                        const bf16x8 a2 = *(const bf16x8*)(B2 + kb * 32 * RB + (k_base ^ (32 * s5)));
                        x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, f2[s5], x2, 0, 0, 0);
                    }
                }
            }
            // streamed row of accumulator element i
            const int srow0 = t * KVB + kb * 32 + 4 * h;
            if constexpr (MODE == BWD_LSE) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (srow0 + (i & 3) + 8 * (i >> 2) >= Lst) x1[i] = -INFINITY;
                    tmax = fmaxf(tmax, x1[i]);
                }
                x1k[kb] = x1;
            } else {
                float z[16];
                float sl[16], sd[16];
                if constexpr (!OWN_Q && DMA) {         // statistics of the streamed rows from the LDS copy (broadcast reads), no global load in the loop
                    const float* st = (const float*)(B1 + 2 * TILE);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 a = *(const f32x4*)(st + kb * 32 + 4 * h + 8 * g);
                        sl[4 * g] = a[0]; sl[4 * g + 1] = a[1]; sl[4 * g + 2] = a[2]; sl[4 * g + 3] = a[3];
                        if constexpr (MODE == BWD_DK) {
                            const f32x4 d4 = *(const f32x4*)(st + 64 + kb * 32 + 4 * h + 8 * g);
                            sd[4 * g] = d4[0]; sd[4 * g + 1] = d4[1]; sd[4 * g + 2] = d4[2]; sd[4 * g + 3] = d4[3];
                        }
                    }
                }
                if constexpr (!OWN_Q && !DMA) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        int q0 = srow0 + 8 * g; if (q0 > (int)stat_ld - 4) q0 = (int)stat_ld - 4;       // stat rows are padded to a multiple of 64
                        const f32x4 a = *(const f32x4*)(stat_l + q0);
                        sl[4 * g] = a[0]; sl[4 * g + 1] = a[1]; sl[4 * g + 2] = a[2]; sl[4 * g + 3] = a[3];
                        if constexpr (MODE == BWD_DK) {
                            const f32x4 d4 = *(const f32x4*)(stat_d + q0);
                            sd[4 * g] = d4[0]; sd[4 * g + 1] = d4[1]; sd[4 * g + 2] = d4[2]; sd[4 * g + 3] = d4[3];
                        }
                    }
                }
                // z = P (DV) or P (dP - delta) (DQ, DK: the softmax scale is applied once, to the accumulator, in the epilogue); rows past the
                // end exist only in the ragged last tile
                if (t * KVB + KVB <= Lst) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -(OWN_Q ? my_lse : sl[i])));
                        z[i] = TWO ? p * (x2[i] - (OWN_Q ? my_delta : sd[i])) : p;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const bool valid = srow0 + (i & 3) + 8 * (i >> 2) < Lst;
                        const float p = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -(OWN_Q ? my_lse : sl[i])));
                        const float v = TWO ? p * (x2[i] - (OWN_Q ? my_delta : sd[i])) : p;
                        z[i] = valid ? v : 0.f;
                    }
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    u32x4 w;
                    w.x = pack2bf(z[8 * s2 + 0], z[8 * s2 + 1]); w.y = pack2bf(z[8 * s2 + 2], z[8 * s2 + 3]);
                    w.z = pack2bf(z[8 * s2 + 4], z[8 * s2 + 5]); w.w = pack2bf(z[8 * s2 + 6], z[8 * s2 + 7]);
                    zf[kb][s2] = __builtin_bit_cast(bf16x8, w);
                }
            }
        }
        if constexpr (MODE == BWD_LSE) {
            tmax = ug_max_halves(tmax);
            const float m_new = fmaxf(m_run, tmax);
            float sum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) sum += __builtin_amdgcn_exp2f((x1k[kb][i] - m_new) * c);
            l_run = l_run * __builtin_amdgcn_exp2f((m_run - m_new) * c) + sum;
            m_run = m_new;
        } else {
            // acc^T[d][own] += T^T[d][streamed] Z[streamed][own], T = st1 (DQ: K, DK: Q) or st2 (DV: dO)
            const unsigned char* Tb = (MODE == BWD_DV) ? B2 : B1;
            if constexpr (PIPE) {
                int lo0 = tlo_base, hi0 = thi_base;
                asm volatile("" : "+v"(lo0), "+v"(hi0));
                bf16x8 tfb[PDA + 1][NDB];
                auto rd = [&](int ks) {
#pragma unroll
                    for (int db = 0; db < NDB; ++db) tfb[ks % (PDA + 1)][db] = tr_read_pair(Tb + ks * 16 * RB + (lo0 ^ (64 * db)), Tb + ks * 16 * RB + (hi0 ^ (64 * db)));
                };
#pragma unroll
                for (int j = 0; j < PDA && j < 4; ++j) rd(j);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks + PDA < 4) rd(ks + PDA);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int db = 0; db < NDB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfb[ks % (PDA + 1)][db], zf[ks >> 1][ks & 1], acc[db], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int db = 0; db < NDB; ++db) {
                        const bf16x8 tf = tr_read_pair(Tb + ks * 16 * RB + (tlo_base ^ (64 * db)), Tb + ks * 16 * RB + (thi_base ^ (64 * db)));
                        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf, zf[ks >> 1][ks & 1], acc[db], 0, 0, 0);
                    }
            }
        }
        if (t + 1 < ntiles) stage_write(cur ^ 1);
        __syncthreads();
    }
    if constexpr (MODE == BWD_LSE) {
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        if (own_row < Lown && h == 0) lse2[(int64_t)bh * stat_ld + own_row] = __builtin_amdgcn_logf(l_tot) + m_run * c;     // v_log_f32 = log2
    } else if (own_row < Lown) {
        bf16_t* Orow = out + (int64_t)b * out_bs + (int64_t)own_row * out_rs + head * DH;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float es = TWO ? scale : 1.f;
                u32x2 w;
                w.x = pack2bf(acc[db][4 * g4 + 0] * es, acc[db][4 * g4 + 1] * es);
                w.y = pack2bf(acc[db][4 * g4 + 2] * es, acc[db][4 * g4 + 3] * es);
                *(u32x2*)(Orow + 32 * db + 8 * g4 + 4 * h) = w;
            }
    }
}

template <int DH, int MODE, bool DMA, typename... Args>
void launch_var(int64_t grid, hipStream_t s, Args... args) {
    constexpr int lds = 2 * (2 * KVB * 2 * DH + (DMA ? 512 : 0));
    static bool attr = false;          // one per instantiation
    if (!attr) { (void)hipFuncSetAttribute((const void*)attn_bwd_var_kernel<DH, MODE, DMA>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
    hipLaunchKernelGGL((attn_bwd_var_kernel<DH, MODE, DMA>), dim3((unsigned)grid), dim3(512), lds, s, args...);
}

template <int DH>
bool variants(int stage, const ug_attn_bwd_args& a) {
    const bool dma = ug_env_int("UG_ATTN_BWD_DMA", 1);     // LDS-DMA staging of the streamed tiles (0: through registers)
    const int nQ = (a.Lq + 255) / 256, nK = (a.Lkv + 255) / 256;
    const int64_t gq = (int64_t)nQ * a.heads * a.batches, gk = (int64_t)nK * a.heads * a.batches;
    const bf16_t* const none = nullptr;
    const int64_t z = 0;
    if (stage == UG_BWD_STAGE_LSE) {
        if (dma) return false;
        launch_var<DH, BWD_LSE, false>(gq, a.s, a.q, a.q_rs, a.q_bs, none, z, z, a.k, a.k_rs, a.k_bs, none, z, z, a.lse2, a.delta, a.stat_ld, (bf16_t*)nullptr, z, z,
                                       a.heads, a.Lq, a.Lkv, nQ, a.c, a.scale);
    } else if (stage == UG_BWD_STAGE_DQ) {
        if (dma) return false;
        launch_var<DH, BWD_DQ, false>(gq, a.s, a.q, a.q_rs, a.q_bs, a.dout, a.do_rs, a.do_bs, a.k, a.k_rs, a.k_bs, a.v, a.v_rs, a.v_bs, a.lse2, a.delta, a.stat_ld,
                                      a.dq, a.dq_rs, a.dq_bs, a.heads, a.Lq, a.Lkv, nQ, a.c, a.scale);
    } else {
        if (dma && ug_env_int("UG_ATTN_BWD_FUSE_DKV", 1)) return false;
        const auto dkv = [&](auto dma_c) {
            constexpr bool DMA = decltype(dma_c)::value;
            launch_var<DH, BWD_DK, DMA>(gk, a.s, a.k, a.k_rs, a.k_bs, a.v, a.v_rs, a.v_bs, a.q, a.q_rs, a.q_bs, a.dout, a.do_rs, a.do_bs, a.lse2, a.delta, a.stat_ld,
                                        a.dk, a.dk_rs, a.dk_bs, a.heads, a.Lkv, a.Lq, nK, a.c, a.scale);
            launch_var<DH, BWD_DV, DMA>(gk, a.s, a.k, a.k_rs, a.k_bs, none, z, z, a.q, a.q_rs, a.q_bs, a.dout, a.do_rs, a.do_bs, a.lse2, a.delta, a.stat_ld,
                                        a.dv, a.dv_rs, a.dv_bs, a.heads, a.Lkv, a.Lq, nK, a.c, a.scale);
        };
        if (dma) dkv(std::true_type{}); else dkv(std::false_type{});
    }
    return true;
}

}  // namespace

// Called by ug_flash_attn_bwd (attention.hip) for each stage, in stream order, with the arguments it has validated.
bool ug_attn_bwd_variants(int stage, int dh, const ug_attn_bwd_args& a) { return dh == 128 ? variants<128>(stage, a) : variants<64>(stage, a); }
