// Attention forward: the forms that were built, measured and dropped. PROBE LIBRARY ONLY (python -m unigen_amd.build --probe); the product's
// forward is flash_attn_kernel<DH, BUFD> in unigen_amd/csrc/attention.hip, which hands every validated call to ug_attn_fwd_variants() below in a
// probe build. Three kernels on the shared device helpers of attn_common.h:
//   flash_attn_var_kernel   the FROZEN general form of the product kernel as of round 6, all ten template parameters: the lock-step loop
//                           (STAGGER = false; PMC: matrix pipe busy 42 %, VALU 45 %, hardly overlapping - 955 vs 989 TFLOP/s at dh 128, L = 4608),
//                           register staging (DMA = false: HBM -> registers -> LDS, issue early, write late), 4-wave workgroups (NW = 4: 800 vs 841
//                           TFLOP/s), 128-key tiles at head width 64 (KV = 128: 906 vs 902 alone, 868 vs 918 inside the SD3.5 forward), PRIO 1 / 2
//                           (prio 0 + wide stores beat the round-1 default prio 1 / narrow everywhere; the static young-half priority 2 loses 1-2 %
//                           at dh 128), 8-byte epilogue stores (WIDE = false). Its header comment and the dispatcher's comments carry the numbers.
//                           A change to the shipped loop is NOT mirrored here: this copy is what the recorded A/B numbers were measured on.
//   flash_attn_m16_kernel   round 4: the stagger on v_mfma_f32_16x16x32_bf16 (+4 % alone, -5.6 % inside the forward)
//   flash_attn_pwg_kernel   one wave per SIMD (4 % behind the 8-wave stagger)
// The default head-width-64 dispatch here is the round-5 form (UG_ATTN_KV64=464: no BUFD / LSUM), bit-identical to the round-5 product, not to today's.
#include "ug_common.h"
#include "attn_common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr bool UG_STAGGER_Q_IN_LDS = false;   // stagger variant: Q fragments from LDS (32 fewer VGPRs) or registers (a third less LDS read traffic in QK^T)

// STAGGER (8 waves, the default): waves 0-3 and 4-7 - the two waves of every SIMD - run one segment apart. A wave alternates a
// matrix-only segment X(t) = P.V(t) then S^T(t+1) = K Q^T (32 MFMAs, an explicit fenced stream) with a VALU-only segment Y(t+1) = the
// online softmax of tile t+1, so a wave's softmax runs under its partner's MFMAs instead of both waves hitting the matrix pipe, then
// the VALU, together (the lock-step loop, STAGGER = false, kept for A/B: both phases then serialise and a tile costs the sum).
// Two barriers per tile; every thread fetches its share of K(t+2), V(t+1) at the start of an even segment and publishes it to LDS at
// the end of the following odd one, into buffers nobody reads in those two segments.
template <int DH, int NW, bool STAGGER, int PRIO = 1, bool WIDE = false, bool DMA = false, int KV = 64, int OCC = 2, bool LSUM = false, bool BUFD = false>   // head dim 128 | 64; waves per workgroup: 8 (256 query rows, 1 / CU) or 4 (128 rows, 2 / CU)
// BUFD (round 6; head width 64 / OCC 4 only): the whole-tile LDS-DMAs in BUFFER form. The stamps put group B's softmax segment 770 cycles above group A's
// (2263 vs 1497), all of it the 4 DMA issues per wave and tile, i.e. the issue sequence itself: per tile ~20 VALU instructions of lane-offset re-derivation
// (kept out of registers in round 3), a 64-bit VALU pointer bump, two v_readfirstlane + s_nop 4 per operand, on a SIMD whose VALU the four waves'
// softmax already saturates. Here the per-lane byte offset is ONE VGPR held through the loop (run 1's is that ^ 16: needs K and V to share a row stride
// that is a multiple of 16 elements - the dispatcher checks), the (batch, head) base is an SGPR resource, the tile / run offset an SGPR: per tile
// 4 x (s_mov m0 + buffer_load ... lds), one v_xor, scalar adds.
// LSUM (round 6, stagger only): the softmax row sums leave the VALU. With the scores' scale / exp2 / max / pack the running sum `l += p` is one of ~5
// VALU instructions per score and the softmax segment Y is what the barriers wait for (tools/attn_stamps.py); here each lane's probabilities are
// summed on the matrix pipe instead, inside X, from the SAME packed bf16 fragments P.V consumes: v_mfma_f32_4x4x4_16b_bf16 (16 blocks of 4x4x4) with
// A = ones makes D[b][i][j] = sum_k B[b][k][j], i.e. every lane gets the sum of the four bf16 values IT passes as B (lane = block b, column j),
// accumulated over the tile's 8 half-fragments: 8 two-pass MFMAs per tile and wave (+12.5 % matrix-pipe cycles) for 32 v_add_f32 (-20 % of the
// softmax segment's issue cycles). The denominator is then the sum of the ROUNDED probabilities - the ones the numerator multiplies - not of their
// fp32 originals (relative difference <= 2^-9 / sqrt(keys), below the output's own bf16 rounding).
// (Round 6 also measured and dropped: five other assignments of the LDS-DMA issue to the wave groups, a 16-wave workgroup, the buffer form at head
// width 128 and a second row-sum chain - stamps in profiles/r06b_*, rates in profiles/r06_attn_variants.log, code in
// tools/probe/patches/attn_r06_variants.diff.)
// KV: keys per tile. 64 everywhere in rounds 1-2; round 3 adds KV = 128 for head dim 64 (UniGenSD3): a 128-key tile of 128-byte rows is the
// same 16 KiB image, the same register budget (S^T 64 + P 32 + O 32 + Q 16 against 32 + 16 + 64 + 32 at dh 128 / 64 keys) and the same 32
// MFMAs per matrix segment as the dh 128 kernel, so the per-segment costs (two barriers, the max exchange, the lazy-rescale test, fences,
// the first-read latency) are paid once per 128 keys instead of once per 64 (at dh 64 the kernel ran at 55-60 %
// of its VALU-issue bound).
// PRIO (stagger only): 0 = no priority games; 1 = s_setprio 1 around the matrix stream of every X segment; 2 = ONE static s_setprio 1 for
// the younger wave group (waves 4-7) before the loop (cdna guide T5, static form); 3 = s_setprio 1 around every softmax segment Y. WIDE: 16-byte
// epilogue stores (T21).
// DMA (stagger only): K / V tiles go HBM -> LDS with global_load_lds_dwordx4 (no staging registers, no ds_write): the swizzled image is
// produced on the SOURCE side (lane l of an instruction lands at byte 16 l of a 1 KiB run = 4 rows at dh 128, so it fetches chunk
// (l % 16) ^ f(row) of its row), and group B (waves 4-7) issues all of it at the start of its softmax segment, two segments ahead of use.
// OCC: waves per SIMD the register allocation must allow. 2 = one 8-wave workgroup per CU (all shipped forms). OCC = 4 (round 3, head dim 64
// only, A/B): <= 128 registers so that TWO workgroups share a CU (64 KiB of LDS each) - four waves per SIMD fill each other's barrier and
// latency bubbles in the VALU-bound dh 64 loop; Q fragments then come from LDS (16 registers fewer).
__global__ __launch_bounds__(64 * NW, OCC) void flash_attn_var_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */, float* __restrict__ lse_out /* nullable */, int64_t lse_ld) {
    constexpr int KVB = KV;                          // shadows the file-level constant (the other kernels keep 64)
    constexpr int NKB = KVB / 32;                    // 32-key blocks of S^T per tile
    constexpr int NKS = KVB / 16;                    // k-steps of O^T += V^T P^T per tile
    constexpr int RB = 2 * DH;                       // row bytes
    constexpr int NCH = DH / 8;                      // 16-byte chunks per row
    constexpr int TILE = KVB * RB;                   // bytes of one K (or V) tile image
    constexpr int QS = DH / 16;                      // k-steps of S^T = K Q^T
    constexpr int NDB = DH / 32;                     // 32-wide d blocks of O^T
    constexpr int QROWS = 32 * NW, NT = 64 * NW, NST = (KVB * NCH) / NT > 0 ? (KVB * NCH) / NT : 1;   // staging chunks of K (and of V) per thread and tile
    static_assert((KVB * NCH) / NT >= 1 || DMA, "tile smaller than the workgroup: register staging cannot cover it (the LDS-DMA form can)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][K tile | V tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    /* -DUG_ATTN_STAMPS (tools/attn_stamps.py, a separate library build; never the product): wave 0 / wave 4 of every workgroup record s_memtime at
     * the kernel's entry, the end of the prologue, the end of the tile loop and the end of the epilogue, s_memrealtime at both ends and the CU they
     * ran on, into the buffer the caller passes as `lse_out` (24 dwords per workgroup and wave group, incl. the four per-segment accumulators of the stagger loop; the log-sum-exp is then not written). */
#ifdef UG_ATTN_STAMPS
    unsigned long long ug_st[4], ug_rt0 = __builtin_amdgcn_s_memrealtime();
#define UG_ASTAMP(I) do { ug_st[I] = __builtin_amdgcn_s_memtime(); } while (0)
    UG_ASTAMP(0);
    // per-segment accumulators of the stagger loop (round 6): cycles a wave spends in Y (softmax, incl. group B's DMA issue), at the barrier behind
    // it, in X (P.V + K.Q^T, incl. group B's DMA wait) and at the barrier behind that, summed over the tiles
    unsigned long long ug_seg[4] = {0, 0, 0, 0}, ug_t = 0;
#define UG_SEG0() do { ug_t = __builtin_amdgcn_s_memtime(); } while (0)
#define UG_SEG(I) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); ug_seg[I] += n_ - ug_t; ug_t = n_; } while (0)
#else
#define UG_ASTAMP(I) do { } while (0)
#define UG_SEG0() do { } while (0)
#define UG_SEG(I) do { } while (0)
#endif

    // XCD-aware block order: all query tiles of one (batch, head) run on one XCD so its K/V stay in that L2.
    const int nwg = gridDim.x;
    const int qd = nwg >> 3, rm = nwg & 7;
    const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
    const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + kk;
    const int qt = logical % nQ;
    const int bh = logical / nQ;
    const int head = bh % heads, b = bh / heads;

    const bf16_t* Qb = q + (int64_t)b * q_bs + head * DH;
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * DH;

    // ---- Q fragments (B operand of S^T = K Q^T): lane (r, h) holds Q[q = r][d = 16 s + 8 h + j] ----
    const int q_row = qt * QROWS + wave * 32 + r;
    const int q_ld = q_row < Lq ? q_row : Lq - 1;
    // Lock-step variant: Q fragments stay in registers. X/Y stagger: they live in LDS (same swizzled row image as K, one
    // ds_read_b128 per k-step) because S^T must survive a barrier next to the P.V operands and 32 fewer VGPRs avoid spills.
    constexpr int QBASE = 2 * 2 * KVB * RB;            // byte offset of the Q image behind the two K|V buffers
    constexpr bool QLDS = STAGGER && (UG_STAGGER_Q_IN_LDS || OCC == 4);
    bf16x8 qf[QLDS ? 1 : QS];
    const int q_lds = QBASE + RB * (wave * 32 + r);
    const int qx = h ^ row_swz<DH>(r);                  // wave * 32 keeps row_swz unchanged (multiple of 16)
    if constexpr (!QLDS) {
#pragma unroll
        for (int s = 0; s < QS; ++s) qf[s] = *(const bf16x8*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);
        // Retire the Q loads HERE: the empty asm takes every fragment as a read-write operand, so hipcc must have the loaded
        // values in hand before it (it waits vmcnt there) and treats them as fresh afterwards. Without it the loads are sunk to
        // the loop header and every iteration re-waits for them with vmcnt(7..0), draining the K/V prefetch issued at its top.
        if constexpr (QS == 8)
            asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]), "+v"(qf[4]), "+v"(qf[5]), "+v"(qf[6]), "+v"(qf[7]));
        else
            asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]));
    } else {
        // each lane copies the 16-byte chunks (16 s + 8 h) of its own query row; only this wave reads them back
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const u32x4 v4 = *(const u32x4*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);
            *(u32x4*)(smem + q_lds + 16 * ((2 * s) ^ qx)) = v4;
        }
    }

    // ---- staging assignment: thread -> 2 chunks of K and 2 of V per tile ----
    int st_row[NST], st_ch[NST], st_off[NST];
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const int cid = tid + NT * u;
        st_row[u] = cid / NCH; st_ch[u] = cid % NCH;
        st_off[u] = img_off<DH>(st_row[u], st_ch[u]);
    }
    u32x4 kreg[NST], vreg[NST];
    auto stage_load = [&](int kv0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            int key = kv0 + st_row[u]; if (key > Lkv - 1) key = Lkv - 1;
            kreg[u] = *(const u32x4*)(Kb + (int64_t)key * k_rs + st_ch[u] * 8);
            vreg[u] = *(const u32x4*)(Vb + (int64_t)key * v_rs + st_ch[u] * 8);
        }
    };
    auto stage_write = [&](int buf) __attribute__((always_inline)) {
        unsigned char* Kbuf = smem + buf * 2 * TILE;
        unsigned char* Vbuf = Kbuf + TILE;
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            *(u32x4*)(Kbuf + st_off[u]) = kreg[u];
            *(u32x4*)(Vbuf + st_off[u]) = vreg[u];
        }
    };

    // ---- per-lane LDS read offsets ----
    // K row read: row = kb*32 + r, chunk = 2s + h  ->  RB*row + 16*((2s) ^ kx),  kx = h ^ f(r)   (f ignores the kb*32 part)
    const int k_rowoff = RB * r;
    const int kx = h ^ row_swz<DH>(r);
    // V transposed read: group g = lane>>4 (16 lanes), i = lane&15. Block rows = keys 16ks + 4h + (i>>2) (+8 for the
    // second half of the k-step), columns d = 32db + 16(g&1) + 4(i&3)..+3. Lane receives column d = 32db + (lane&31).
    const int i16 = lane & 15, g16 = lane >> 4;
    const int v_key = 4 * h + (i16 >> 2);
    const int v_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1);
    const int v_b8 = 8 * (i16 & 1);
    int voff_lo[NDB], voff_hi[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        const int ch = 4 * db + v_lowch;
        voff_lo[db] = RB * v_key + 16 * (ch ^ row_swz<DH>(v_key)) + v_b8;              // f(16 ks + key) == f(key)
        voff_hi[db] = RB * (v_key + 8) + 16 * (ch ^ row_swz<DH>(v_key + 8)) + v_b8;
    }

    f32x16 oacc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    static_assert(!LSUM || STAGGER, "the matrix-pipe row sum lives in the stagger loop's X segment");
    f32x4 lacc = {0.f, 0.f, 0.f, 0.f};                 // LSUM: register 0 = half of this lane's running row sum (rows 1-3 of its 4x4 block: unused copies)
    bf16x4 ones4 = {(short)0x3f80, (short)0x3f80, (short)0x3f80, (short)0x3f80};
    if constexpr (LSUM) asm volatile("" : "+v"(ones4));        // one VGPR pair for the loop, not re-materialised per use

    const int ntiles = (Lkv + KVB - 1) / KVB;
    bf16x8 pf[NKB][2];                                 // P^T fragments of the tile between its S and P stages
    // CUR = buffer parity as a compile-time constant: every LDS address below is then a loop-invariant VGPR + an immediate offset
    // (with a runtime parity hipcc re-materialised ~50 address adds per tile, a quarter of the VALU work of the loop).
    f32x16 sacc[NKB];                                  // S^T of the tile between its QK^T and its softmax
    auto do_QK = [&](int t, auto cur_c) __attribute__((always_inline)) {
        constexpr int CUR = decltype(cur_c)::value;
        const int kv0 = t * KVB;
        const unsigned char* Kbuf = smem + CUR * 2 * TILE;
        // ---- S^T[key][q]: all 8 K fragments of key block 0 first, then block-0 MFMAs with the block-1 reads between them ----
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
        if constexpr (!STAGGER) {
            bf16x8 kf[NKB][QS];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int s = 0; s < QS; ++s) kf[kb][s] = *(const bf16x8*)(Kbuf + kb * 32 * RB + k_rowoff + 16 * ((2 * s) ^ kx));
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int s = 0; s < QS; ++s) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][s], qf[s], sacc[kb], 0, 0, 0);
            if constexpr (NKB == 2) {
                __builtin_amdgcn_sched_group_barrier(0x100, QS, 0);       // ds_reads of key block 0
#pragma unroll
                for (int s = 0; s < QS; ++s) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // 1 MFMA (block 0)
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);    // 1 ds_read (block 1)
                }
                __builtin_amdgcn_sched_group_barrier(0x008, QS, 0);       // MFMAs of block 1
            }
        } else {
            // Q comes from LDS too: per k-step one Q fragment and the two key blocks' K fragments, read two steps ahead of their
            // MFMAs (9 fragments = 36 VGPRs live instead of 24 fragments if hipcc hoisted every read).
            bf16x8 ql[QS], kf[NKB][QS];
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                if constexpr (QLDS) ql[s] = *(const bf16x8*)(smem + q_lds + 16 * ((2 * s) ^ qx)); else ql[s] = qf[s];
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) kf[kb][s] = *(const bf16x8*)(Kbuf + kb * 32 * RB + k_rowoff + 16 * ((2 * s) ^ kx));
            }
#pragma unroll
            for (int s = 0; s < QS; ++s)
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][s], ql[s], sacc[kb], 0, 0, 0);
            if constexpr (NKB == 2) {
                __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);        // fragments of k-steps 0, 1
#pragma unroll
                for (int s = 0; s < QS - 2; ++s) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);    // MFMAs of step s
                    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);    // fragments of step s + 2
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
        }
        if (kv0 + KVB > Lkv) {   // ragged last tile: keys >= Lkv do not exist
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = kv0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (key >= Lkv) sacc[kb][i] = -INFINITY;
                }
        }
    };
    auto do_SM = [&]() __attribute__((always_inline)) {
        // ---- online softmax, all lane-local (this lane: query r, 32 of the tile's 64 keys; lane^32 has the rest) ----
        float tmax = sacc[0][0];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, sacc[kb][i]);
        tmax = ug_max_halves(tmax);
        // Lazy reference point: a row's running max moves only when the tile maximum exceeds it by more than 2^8 in the exponent
        // (softmax is shift-invariant; P and l stay below 2^8 per element: exact in fp32, same relative precision in bf16). With the
        // exact max some row of the wave moves in most tiles and the 64-register rescale below ran nearly every iteration.
        const bool up = (tmax - m_run) * c > 8.0f;
        const float m_new = up ? tmax : m_run;
        if (!__all(!up)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            if constexpr (LSUM) lacc[0] *= alpha; else l_run *= alpha;
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
            m_run = m_new;
        }
        const float mc = m_run * c;
        // (Measured and dropped, round 2, bit-identical: exponentiating key block 1 - or only its last 8 scores per lane - inside X(t), 3-7 VALU
        // instructions behind each of its first 8 P.V MFMAs: -8 % / -4 % at dh 128, -10 % / -7 % at dh 64. Ablations of the same day (tools/attn_ab.py
        // on diagnostic builds): without the K/V DMAs +7-10 %, without this softmax +18 % (+37 % at dh 64), without both +28 % (+53 %): the matrix
        // segments alone take 78 % of the loop's time at dh 128, and VALU work moved into them costs more than it saves here.)
        // (Measured and dropped: the row sum from the packed bf16 probabilities, two per v_dot2c_f32_bf16: -3.5 % at dh 128. Considered and
        // rejected on accuracy: Q pre-multiplied by scale * log2(e) in bf16 with the accumulators initialised to -m (no fma per score): the
        // attention error against fp32 grows from 1.6e-3 to 2.3e-3, 4x on peaked rows.)
        // (Measured and dropped, same box: the scale / shift and the row sums two elements per instruction, v_pk_fma_f32 / v_pk_add_f32 -
        // 5 % SLOWER at dh 128 (1086 vs 1146, 1118 vs 1179 TFLOP/s), +1 % at dh 64: the packed forms buy no issue cycles here.)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            float p[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                p[i] = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], c, -mc));
                if constexpr (!LSUM) l_run += p[i];
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 w;
                w.x = pack2bf(p[8 * s2 + 0], p[8 * s2 + 1]); w.y = pack2bf(p[8 * s2 + 2], p[8 * s2 + 3]);
                w.z = pack2bf(p[8 * s2 + 4], p[8 * s2 + 5]); w.w = pack2bf(p[8 * s2 + 6], p[8 * s2 + 7]);
                pf[kb][s2] = __builtin_bit_cast(bf16x8, w);
            }
        }
    };
    auto do_P = [&](int t, auto cur_c) __attribute__((always_inline)) {
        constexpr int CUR = decltype(cur_c)::value;
        const unsigned char* Vbuf = smem + CUR * 2 * TILE + TILE;
        // ---- O^T[d][q] += V^T[d][key] P^T[key][q]: the V fragments of d-block db+1 are read between the MFMAs of block db ----
        {
            bf16x8 vf[NDB][NKS];
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    vf[db][ks] = tr_read_pair(Vbuf + ks * 16 * RB + voff_lo[db], Vbuf + ks * 16 * RB + voff_hi[db]);
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[db][ks], pf[ks >> 1][ks & 1], oacc[db], 0, 0, 0);
            if constexpr (NKS == 4) {
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);            // 8 tr reads (d-block 0)
#pragma unroll
                for (int i = 0; i < 4 * (NDB - 1); ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);        // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);        // 2 tr reads of the next d-block
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 1);            // last d-block
            }
        }
    };
    // X(t) of the stagger variant as an explicit stream (sched_barrier after every piece): P.V(t) - 16 MFMAs, k-step outer so the 4
    // (8 at dh = 128... NDB) accumulators rotate - then S^T(t+1) = K Q^T - 16 MFMAs. Every LDS fragment is read two or three steps ahead
    // of its MFMA and the first K / Q fragments of the second half are requested under the last P.V MFMAs: this wave is alone on the
    // matrix pipe in this segment (its SIMD partner is in the VALU-only Y), so an exposed ds_read latency is an idle pipe. hipcc's
    // own order (sched_group_barrier hints included) ran the segment at 70-90 cycles per MFMA.
    auto qx_frag = [&](int s) __attribute__((always_inline)) -> bf16x8 { if constexpr (QLDS) return *(const bf16x8*)(smem + q_lds + 16 * ((2 * s) ^ qx)); else return qf[s]; };
    auto do_X = [&](int t, auto cur_c, bool have_qk) __attribute__((always_inline)) {
        constexpr int CUR = decltype(cur_c)::value;
        const unsigned char* Vbuf = smem + CUR * 2 * TILE + TILE;
        const unsigned char* Kbuf = smem + (CUR ^ 1) * 2 * TILE;
        bf16x8 vf[NKS][NDB];
        auto rdv = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) vf[ks][db] = tr_read_pair(Vbuf + ks * 16 * RB + voff_lo[db], Vbuf + ks * 16 * RB + voff_hi[db]);
        };
        bf16x8 kf[NKB][QS];
        auto rdk = [&](int s) __attribute__((always_inline)) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) kf[kb][s] = *(const bf16x8*)(Kbuf + kb * 32 * RB + k_rowoff + 16 * ((2 * s) ^ kx));
        };
        constexpr int QPRE = QS / 4;                   // k-steps of K.Q^T whose fragments are requested under each of the last two P.V steps
        rdv(0); rdv(1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(1);                   // the matrix stream outranks the partner wave's softmax VALU at issue
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks][db], pf[ks >> 1][ks & 1], oacc[db], 0, 0, 0);
            if constexpr (LSUM) {        // this lane's 8 probabilities of the k-step, summed on the matrix pipe (see the template's header)
                const bf16x8 pw = pf[ks >> 1][ks & 1];
                lacc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones4, __builtin_shufflevector(pw, pw, 0, 1, 2, 3), lacc, 0, 0, 0);
                lacc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones4, __builtin_shufflevector(pw, pw, 4, 5, 6, 7), lacc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 2 < NKS) rdv(ks + 2);
            else if (have_qk) {                                                    // the first 2 QPRE k-steps of the second half
#pragma unroll
                for (int j = 0; j < QPRE; ++j) rdk(QPRE * (ks - (NKS - 2)) + j);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!have_qk) { if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(0); return; }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
        for (int s = 0; s < QS; ++s) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][s], qx_frag(s), sacc[kb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 2 * QPRE < QS) { rdk(s + 2 * QPRE); __builtin_amdgcn_sched_barrier(0); }
        }
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(0);
        const int kv0 = (t + 1) * KVB;
        if (kv0 + KVB > Lkv) {   // ragged last tile: keys >= Lkv do not exist
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = kv0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (key >= Lkv) sacc[kb][i] = -INFINITY;
                }
        }
    };
    if constexpr (!STAGGER) {
        stage_load(0);
        stage_write(0);
        __syncthreads();
        auto tile = [&](int t, auto cur_c) __attribute__((always_inline)) {
            constexpr int CUR = decltype(cur_c)::value;
            if (t + 1 < ntiles) stage_load((t + 1) * KVB);
            do_QK(t, cur_c);
            do_SM();
            do_P(t, cur_c);
            if (t + 1 < ntiles) stage_write(CUR ^ 1);
            __syncthreads();
        };
        for (int t = 0; t < ntiles; t += 2) {
            tile(t, std::integral_constant<int, 0>{});
            if (t + 1 < ntiles) tile(t + 1, std::integral_constant<int, 1>{});
        }
    } else {
        static_assert(!STAGGER || NW == 8, "the stagger pairs the waves of one SIMD: w, w + 4");
        // X / Y stagger. A wave alternates a MATRIX-only segment X(t) = P.V of tile t followed by S^T = K.Q^T of tile t+1, and a
        // VALU-only segment Y(t+1) = online softmax of tile t+1. Waves 0-3 (group A) and 4-7 (group B) - the two waves of every
        // SIMD - run one segment apart, so in every segment a SIMD has one wave feeding the matrix pipe and one feeding the VALU
        // (PMC on the lock-step loop: matrix pipe busy 42 %, VALU 45 %, hardly overlapping).
        //   global segment:   0       1       2       3       4
        //   group A:        QK(0)    Y(0)    X(0)    Y(1)    X(1) ...
        //   group B:          -     QK(0)    Y(0)    X(0)    Y(1) ...
        // K(t+1) and V(t) are first needed in segment 2t+2: every thread fetches its share at the START of even segment 2t and
        // publishes it at the END of odd segment 2t+1 (into buffers nobody reads in 2t / 2t+1). Loads cross barriers: raw s_barrier.
        auto seg_barrier = [&]() __attribute__((always_inline)) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        // K(kt), V(vt) -> registers -> LDS. Branch-free on purpose: tiles past the end are clamped re-reads published into buffers whose
        // last readers are done. With a per-load `if (tile < ntiles)` every global_load sat in its own basic block behind an
        // `s_waitcnt vmcnt(0)`: the four loads of a fetch ran one after the other at full memory latency (~4400 cycles per fetch
        // segment, found with s_memtime stamps) - that, not the segment structure, is why this variant first measured 602 TFLOP/s.
        // Addresses: a wave-uniform tile base (SALU) + a per-thread 32-bit element offset computed once - a fetch is then 2 NST loads and
        // no VALU (with `key * stride` in 64 bits per load, a fetch cost the matrix segment ~700 cycles before its first MFMA). The
        // ragged last tile and tiles past the end take the clamped path.
        unsigned koff[NST], voff[NST];
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            koff[u] = (unsigned)(st_row[u] * (int)k_rs + st_ch[u] * 8);
            voff[u] = (unsigned)(st_row[u] * (int)v_rs + st_ch[u] * 8);
        }
        auto fetch = [&](int kt, int vt) __attribute__((always_inline)) {
            if (kt * KVB + KVB <= Lkv && vt * KVB + KVB <= Lkv) {       // wave-uniform: both tiles whole
                const bf16_t* kbase = Kb + (int64_t)kt * KVB * k_rs;
                const bf16_t* vbase = Vb + (int64_t)vt * KVB * v_rs;
#pragma unroll
                for (int u = 0; u < NST; ++u) {
                    kreg[u] = *(const u32x4*)(kbase + koff[u]);
                    vreg[u] = *(const u32x4*)(vbase + voff[u]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < NST; ++u) {
                    int key = kt * KVB + st_row[u]; if (key > Lkv - 1) key = Lkv - 1;
                    kreg[u] = *(const u32x4*)(Kb + (int64_t)key * k_rs + st_ch[u] * 8);
                    key = vt * KVB + st_row[u]; if (key > Lkv - 1) key = Lkv - 1;
                    vreg[u] = *(const u32x4*)(Vb + (int64_t)key * v_rs + st_ch[u] * 8);
                }
            }
        };
        auto publish = [&](int kt, int vt) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < NST; ++u) {
                *(u32x4*)(smem + (kt & 1) * 2 * TILE + st_off[u]) = kreg[u];
                *(u32x4*)(smem + (vt & 1) * 2 * TILE + TILE + st_off[u]) = vreg[u];
            }
        };
        const bool groupA = __builtin_amdgcn_readfirstlane(wave) < NW / 2;
        // LDS-DMA staging: a tile image is NI runs of 1 KiB (RPI rows each); wave wb of group B owns runs wb * NIW .. + NIW - 1
        // (measured and dropped: every wave issuing NI / 8 runs, group A's half at the start of its own softmax segment 2t+1 and waited for
        // at its end - same bits, -0.5 % at dh 128, -12 % at dh 64: group B's issue cost is not what bounds the segment pairs; and group A
        // issuing all of them one at a time behind the MFMAs of the first 2 NIW steps of its matrix segment: -11 % / -4 %, ~46 cycles of
        // matrix-segment time per DMA)
        constexpr int RPI = 1024 / RB, NI = TILE / 1024, NIW = NI / (NW / 2);
        static_assert(NIW >= 1, "fewer 1 KiB runs in a tile than issuing waves");
        const int wb = __builtin_amdgcn_readfirstlane(wave) & (NW / 2 - 1);
        unsigned dko[NIW], dvo[NIW];
#pragma unroll
        for (int u = 0; u < NIW; ++u) {
            const int row = (wb * NIW + u) * RPI + lane / NCH;
            const int ch = (lane % NCH) ^ row_swz<DH>(row);
            dko[u] = (unsigned)(row * (int)k_rs + ch * 8) * 2u;        // bytes
            dvo[u] = (unsigned)(row * (int)v_rs + ch * 8) * 2u;
        }
        static_assert(!BUFD || (DMA && DH == 64 && OCC == 4), "BUFD is the head-width-64, two-workgroups-per-CU form of the LDS-DMA staging");
        static_assert(!BUFD || NIW == 2, "the buffer form derives run 1 from run 0");
        unsigned bvo = 0;                              // BUFD: lane offset of run 0 inside a wave's pair of 1 KiB runs (rows lane / 8, swizzled chunk)
        u32x4 rsK = {0u, 0u, 0u, 0u}, rsV = {0u, 0u, 0u, 0u};
        if constexpr (BUFD) {
            const int sw = (((lane >> 4) & 1) << 2) | ((lane >> 4) & 2);
            bvo = (unsigned)((lane >> 3) * (int)k_rs) * 2u + (unsigned)(((lane & 7) ^ sw) << 4);
            asm volatile("" : "+v"(bvo));
            const unsigned long long ka = (unsigned long long)uniform_ptr(Kb), va = (unsigned long long)uniform_ptr(Vb);
            rsK = (u32x4){(unsigned)ka, (unsigned)(ka >> 32), 0xffffffffu, 0x00020000u};
            rsV = (u32x4){(unsigned)va, (unsigned)(va >> 32), 0xffffffffu, 0x00020000u};
        }
        auto dma_tile = [&](const bf16_t* base, int64_t rs, const unsigned (&off)[NIW], int tile, unsigned dst, auto is_k) {
            if (tile * KVB + KVB <= Lkv) {             // whole tile: wave-uniform base (SGPR pair) + per-lane 32-bit byte offset
                if constexpr (BUFD) {
                    const unsigned so = (unsigned)((tile * KVB + wb * NIW * RPI) * (int)rs) * 2u;          // scalar: tile and run-pair part of the byte offset
                    if constexpr (decltype(is_k)::value) {
                        bufds16(rsK, bvo, so, dst);
                        bufds16(rsK, bvo ^ 16u, so + (unsigned)(RPI * (int)rs) * 2u, dst + 1024);
                    } else {
                        bufds16(rsV, bvo, so, dst);
                        bufds16(rsV, bvo ^ 16u, so + (unsigned)(RPI * (int)rs) * 2u, dst + 1024);
                    }
                } else if constexpr (OCC == 4 && DH == 64 && NIW == 2) {
                    // Lane offsets re-derived at the issue (not kept live through the loop: registers are what this form is short of), cheaply:
                    // run u of wave wb covers rows (2 wb + u) * 8 + lane / 8, so the wave / run part of the row goes into the scalar base and
                    // row_swz<64> reduces to a lane term with bit 0 = u: the second run's chunk is the first one's ^ 1. ~10 VALU per tile
                    // instead of ~48 (round 3: the generic re-derivation was ~12 % of the issuing waves' VALU instructions).
                    int lane_r = lane;
                    asm volatile("" : "+v"(lane_r));
                    const int sw = (((lane_r >> 4) & 1) << 2) | ((lane_r >> 4) & 2);
                    const unsigned c0 = (unsigned)(((lane_r & 7) ^ sw) << 4), rp = (unsigned)((lane_r >> 3) * (int)rs) * 2u;
                    const char* tw = (const char*)uniform_ptr(base + ((int64_t)tile * KVB + wb * NIW * RPI) * rs);
                    glds16_off(tw, rp + c0, dst);
                    glds16_off(tw + (int64_t)RPI * rs * 2, rp + (c0 ^ 16u), dst + 1024);
                } else if constexpr (OCC == 4) {
                    const void* tb = uniform_ptr(base + (int64_t)tile * KVB * rs);
                    int lane_r = lane;
                    asm volatile("" : "+v"(lane_r));
#pragma unroll
                    for (int u = 0; u < NIW; ++u) {
                        const int row = (wb * NIW + u) * RPI + lane_r / NCH;
                        const int ch = (lane_r % NCH) ^ row_swz<DH>(row);
                        glds16_off(tb, (unsigned)(row * (int)rs + ch * 8) * 2u, dst + u * 1024);
                    }
                } else {
                    const void* tb = uniform_ptr(base + (int64_t)tile * KVB * rs);
#pragma unroll
                    for (int u = 0; u < NIW; ++u) glds16_off(tb, off[u], dst + u * 1024);
                }
            } else {                                   // ragged last tile: rows past the end re-read the last key (masked in S^T)
                int lane_r = lane;
                asm volatile("" : "+v"(lane_r));      // row / chunk re-derived here, not kept live through the loop
#pragma unroll
                for (int u = 0; u < NIW; ++u) {
                    const int row = (wb * NIW + u) * RPI + lane_r / NCH;
                    const int ch = (lane_r % NCH) ^ row_swz<DH>(row);
                    int key = tile * KVB + row; if (key > Lkv - 1) key = Lkv - 1;
                    glds16_ptr(base + (int64_t)key * rs + ch * 8, dst + u * 1024);
                }
            }
        };
        auto dma_fetch = [&](int kt, int vt) __attribute__((always_inline)) {         // tiles past the end are simply not fetched
            const unsigned l0 = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wb * NIW * 1024;
            if (kt < ntiles) dma_tile(Kb, k_rs, dko, kt, l0 + (kt & 1) * 2 * TILE, std::true_type{});
            if (vt < ntiles) dma_tile(Vb, v_rs, dvo, vt, l0 + (vt & 1) * 2 * TILE + TILE, std::false_type{});
        };
        auto dma_wait = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
        if constexpr (PRIO == 2) { if (!groupA) __builtin_amdgcn_s_setprio(1); }
        if constexpr (DMA) {
            if (!groupA) { dma_fetch(0, ntiles); dma_wait(); }     // K(0) only
            seg_barrier();
            if (!groupA) dma_fetch(1, 0);
        } else {
            fetch(0, ntiles);                          // K(0) only
            publish(0, ntiles);
            seg_barrier();
            fetch(1, 0);                               // segment 0 (even): K(1), V(0) in flight
        }
        if (!groupA) seg_barrier();                    // B idles through segment 0
        UG_ASTAMP(1);
        do_QK(0, std::integral_constant<int, 0>{});    // A: segment 0 | B: segment 1
        if (!groupA) { if constexpr (DMA) dma_wait(); else publish(1, 0); }    // end of segment 1 (B)
        seg_barrier();
        // one tile = Y(t) | X(t); buffer parity is a compile-time constant (two tiles per trip)
        auto tile = [&](int t, auto cur_c) __attribute__((always_inline)) {
            // Y(t): A in odd segment 2t+1 (publishes K(t+1), V(t) at its end) | B in even segment 2t+2 (fetches K(t+2), V(t+1) at its start)
            if (!groupA) { if constexpr (DMA) dma_fetch(t + 2, t + 1); else fetch(t + 2, t + 1); }
            if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(1);                  // the softmax segment outranks the partner's matrix stream at issue
            do_SM();
            // P^T is "used" here: hipcc otherwise sinks the (pure) scale / exp2 / pack chain across the barrier to its first use, the
            // P.V MFMAs - i.e. out of this VALU-only segment into the matrix-only one, which then ran at ~60 cycles per MFMA
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) { asm volatile("" : "+v"(pf[kb][0])); asm volatile("" : "+v"(pf[kb][1])); }
            if constexpr (LSUM) asm volatile("" : "+v"(m_run)); else asm volatile("" : "+v"(l_run), "+v"(m_run));
            if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(0);
            // group A publishes K(t+1), V(t) and at once re-fills the staging registers with K(t+2), V(t+1): its VALU segment has slack
            // (the partner's matrix segment is longer), whereas a fetch at the head of its own X(t) delayed the first MFMA
            if constexpr (!DMA) { if (groupA) { publish(t + 1, t); fetch(t + 2, t + 1); } }
            UG_SEG(0);
            seg_barrier();
            UG_SEG(1);
            // X(t) = P.V(t) then K.Q^T(t+1): A in even segment 2t+2 | B in odd segment 2t+3 (publish). (Measured and dropped: group B
            // reading its first V^T fragments ahead of the barrier, inside its softmax segment: -4 %, -10 % with two k-steps.)
            do_X(t, cur_c, t + 1 < ntiles);
            if (!groupA) { if constexpr (DMA) dma_wait(); else publish(t + 2, t + 1); }
            UG_SEG(2);
            seg_barrier();
            UG_SEG(3);
        };
        UG_SEG0();
        for (int t = 0; t < ntiles; t += 2) {
            tile(t, std::integral_constant<int, 0>{});
            if (t + 1 < ntiles) tile(t + 1, std::integral_constant<int, 1>{});
        }
        UG_ASTAMP(2);
        if (groupA) seg_barrier();                     // A's trailing (empty) segment pairs with B's last one
    }

    // ---- epilogue: O[q][d] = O^T / l ----
    if constexpr (LSUM) l_run = lacc[0];
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    // training: log2 sum_k 2^(c s) of the row for the backward kernels (m_run is the row's reference point, shared by both lane halves)
#ifndef UG_ATTN_STAMPS
    if (lse_out != nullptr && h == 0 && q_row < Lq) lse_out[(int64_t)bh * lse_ld + q_row] = __builtin_amdgcn_logf(l_tot) + m_run * c;
#endif
    const float inv = 1.0f / l_tot;
    if constexpr (WIDE) {
        // Lane (r, h) holds, per 8-column group g4 of a 32-wide d block, columns 8 g4 + 4 h .. + 3 of its query row (8 bytes). One
        // v_permlane32_swap per dword on the group pair (k, k + 1) moves the upper half-wave's group-k data down and the lower half's
        // group-(k + 1) data up: lanes 0-31 then hold columns 8k .. 8k + 7 and lanes 32-63 columns 8k + 8 .. 8k + 15 of the row: ONE
        // 16-byte store per pair instead of two 8-byte ones (cdna guide T21: the store tail is issue-bound). Rows past Lq only skip the store.
        bf16_t* Orow = o + (int64_t)b * o_bs + (int64_t)(q_row < Lq ? q_row : Lq - 1) * o_rs + head * DH + 8 * h;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int k2 = 0; k2 < 4; k2 += 2) {
                unsigned ax = pack2bf(oacc[db][4 * k2 + 0] * inv, oacc[db][4 * k2 + 1] * inv), ay = pack2bf(oacc[db][4 * k2 + 2] * inv, oacc[db][4 * k2 + 3] * inv);
                unsigned bx = pack2bf(oacc[db][4 * k2 + 4] * inv, oacc[db][4 * k2 + 5] * inv), by = pack2bf(oacc[db][4 * k2 + 6] * inv, oacc[db][4 * k2 + 7] * inv);
                auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
                auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
                u32x4 w; w.x = rx[0]; w.y = ry[0]; w.z = rx[1]; w.w = ry[1];
                if (q_row < Lq) *(u32x4*)(Orow + 32 * db + 8 * k2) = w;
            }
    } else if (q_row < Lq) {
        bf16_t* Orow = o + (int64_t)b * o_bs + (int64_t)q_row * o_rs + head * DH;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                u32x2 w;
                w.x = pack2bf(oacc[db][4 * g4 + 0] * inv, oacc[db][4 * g4 + 1] * inv);
                w.y = pack2bf(oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv);
                *(u32x2*)(Orow + 32 * db + 8 * g4 + 4 * h) = w;
            }
    }
#ifdef UG_ATTN_STAMPS
    UG_ASTAMP(3);
    if (lse_out != nullptr && lane == 0 && (wave & (NW / 2 - 1)) == 0) {
        unsigned long long* d = (unsigned long long*)lse_out + ((int64_t)blockIdx.x * 2 + wave / (NW / 2)) * 12;
        d[8] = ug_seg[0]; d[9] = ug_seg[1]; d[10] = ug_seg[2]; d[11] = ug_seg[3];
        d[0] = ug_st[0]; d[1] = ug_st[1]; d[2] = ug_st[2]; d[3] = ug_st[3]; d[4] = ug_rt0; d[5] = __builtin_amdgcn_s_memrealtime();
        d[6] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // XCC_ID | HW_ID
        d[7] = (unsigned long long)logical;
    }
#endif
#undef UG_ASTAMP
#undef UG_SEG0
#undef UG_SEG
}

// =====================================================================================================================
// Round 4: the X|Y stagger kernel on v_mfma_f32_16x16x32_bf16 - the bf16 shape this chip clocks ~1.12-1.15x higher than 32x32x16 at equal
// cycles per FLOP (MI355X_MICROARCH "DVFS give-back" item 7; tools/probe/coexec4.hip priced this loop's skeleton at +3...+6 %).
// Same workgroup (8 waves x 32 query rows), same 64-key tiles, same swizzled LDS image, same LDS-DMA staging, same segment structure;
// what changes is the operand geometry (lane = (i, g), i = lane & 15, g = lane >> 4):
//   S^T tile (kt, qb) = K[16 keys] Q^T[16 queries], 32 of d per MFMA:  A = K row key(kt, i), chunk 4 s + g (ds_read_b128);  B = Q row 16 qb + i
//     from registers;  D: lane holds S^T[key(kt, 4 g + r)][query 16 qb + i], r = 0..3.
//   O^T tile (db, qb) = V^T[16 d] P^T[32 keys]:  B = this lane's OWN S^T registers of the key-tile pair (2 ks, 2 ks + 1), packed to bf16 - element
//     j of lane group g is key slot (kt = 2 ks + (j >> 2), row 4 g + (j & 3)) - no LDS, no cross-lane traffic for P;  A = V^T, two
//     ds_read_b64_tr_b16 per (ks, db): the 4-key blocks key(2 ks, 4 g ..) and key(2 ks + 1, 4 g ..) of columns 16 db .. + 15.
//   Every LDS fragment feeds TWO MFMAs (qb = 0, 1), so LDS reads, VGPRs and MFMA cycles per tile equal the 32x32x16 kernel's
//   (16 ds_read_b128 + 32 tr reads, 64 x 16 instead of 32 x 32 MFMA cycles per tile and wave).
//   key(kt, rho) = 16 kt + ((rho - 4) & 15): the rotation makes BOTH read kinds conflict-free on the shared image at head width 128 - a
//   ds_read_b128 lane group {i in 0-3, 12-15 of g; i in 4-11 of g + 1} covers all 16 slots of the bank row iff the rows read by lanes 4-11 are
//   closed under row ^ 4 (f(row) ^ 1 = f(row ^ 4) for the image's f), and a transposed read's 32-lane half takes rows {12-15, 0-3} or
//   {4-7, 8-11}, whose slot pairs f(row) >> 1 are distinct. (With key = 16 kt + rho the row reads are 2-way, cdna guide T10.)
//   Softmax: a query's scores are spread over the 4 lane groups - row max and final row sum take one v_permlane16_swap + one v_permlane32_swap.
// =====================================================================================================================
__device__ __forceinline__ float ug_max_groups(float x) {      // max over lanes l, l ^ 16, l ^ 32, l ^ 48, in every lane
    unsigned u = __float_as_uint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    x = __builtin_fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    u = __float_as_uint(x);
    const auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float ug_sum_groups(float x) {
    unsigned u = __float_as_uint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    u = __float_as_uint(x);
    const auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

template <int DH, int PRIO>
__global__ __launch_bounds__(512, 2) void flash_attn_m16_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */, float* __restrict__ lse_out /* nullable */, int64_t lse_ld) {
    constexpr int KVB = 64, RB = 2 * DH, NCH = DH / 8, TILE = KVB * RB;
    constexpr int NS = DH / 32;                      // k-steps (32 of d) of S^T = K Q^T
    constexpr int NDB = DH / 16;                     // 16-wide d blocks of O^T
    constexpr int NKT = KVB / 16;                    // 16-key tiles of S^T per K/V tile
    constexpr int NKS = KVB / 32;                    // k-steps (32 keys) of O^T += V^T P^T
    constexpr int NU = NKS * (NDB / 4);              // P.V steps of 8 MFMAs (4 d blocks x 2 query blocks)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][K tile | V tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;

    const int nwg = gridDim.x;
    const int qd = nwg >> 3, rm = nwg & 7;
    const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
    const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + kk;
    const int qt = logical % nQ;
    const int bh = logical / nQ;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* Qb = q + (int64_t)b * q_bs + head * DH;
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * DH;

    // ---- Q fragments (B operand of S^T): lane (i, g) holds Q[16 qb + i][32 s + 8 g + j] ----
    bf16x8 qf[2][NS];
    int q_row[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        q_row[qb] = qt * 256 + wave * 32 + 16 * qb + i;
        const int q_ld = q_row[qb] < Lq ? q_row[qb] : Lq - 1;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[qb][s] = *(const bf16x8*)(Qb + (int64_t)q_ld * q_rs + 32 * s + 8 * g);
    }
    // retire the Q loads here (see flash_attn_kernel): otherwise every loop iteration re-waits for them and drains the K/V prefetch
    if constexpr (NS == 4)
        asm volatile("" : "+v"(qf[0][0]), "+v"(qf[0][1]), "+v"(qf[0][2]), "+v"(qf[0][3]), "+v"(qf[1][0]), "+v"(qf[1][1]), "+v"(qf[1][2]), "+v"(qf[1][3]));
    else
        asm volatile("" : "+v"(qf[0][0]), "+v"(qf[0][1]), "+v"(qf[1][0]), "+v"(qf[1][1]));

    // ---- per-lane LDS read offsets ----
    const int pi_i = (i - 4) & 15;                   // S^T-tile row i of this lane <-> image row 16 kt + pi_i
    const int k_rowoff = RB * pi_i;
    const int fk = row_swz<DH>(pi_i);
    // transposed V read: lane 4 qq + pp of group g supplies row rho = (4 g + qq - 4) & 15 (+ 16 kt), columns 16 db + 4 pp .. + 3
    const int qq = i >> 2, pp = i & 3;
    const int rho = (4 * g + qq - 4) & 15;
    int voff[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) voff[db] = RB * rho + 16 * ((2 * db + (pp >> 1)) ^ row_swz<DH>(rho)) + 8 * (pp & 1);

    f32x4 oacc[NDB][2];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) oacc[db][qb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    const int ntiles = (Lkv + KVB - 1) / KVB;
    bf16x8 pf[NKS][2];                                 // P^T fragments of the tile between its softmax and its P.V
    f32x4 sacc[NKT][2];                                // S^T of the tile between its K Q^T and its softmax

    auto mask_ragged = [&](int kv0) __attribute__((always_inline)) {
        if (kv0 + KVB > Lkv) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + 16 * kt + ((4 * g + r - 4) & 15);
                    if (key >= Lkv) { sacc[kt][0][r] = -INFINITY; sacc[kt][1][r] = -INFINITY; }
                }
        }
    };
    auto do_QK0 = [&]() __attribute__((always_inline)) {     // tile 0 (buffer 0): no P.V before it
        const unsigned char* Kbuf = smem;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) { sacc[kt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; sacc[kt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const bf16x8 kf = *(const bf16x8*)(Kbuf + kt * 16 * RB + k_rowoff + 16 * ((4 * s + g) ^ fk));
                sacc[kt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][s], sacc[kt][0], 0, 0, 0);
                sacc[kt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][s], sacc[kt][1], 0, 0, 0);
            }
        mask_ragged(0);
    };
    auto do_SM = [&]() __attribute__((always_inline)) {
        float tmax[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float t = sacc[0][qb][0];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                t = ug_max3(t, sacc[kt][qb][0], sacc[kt][qb][1]);
                t = ug_max3(t, sacc[kt][qb][2], sacc[kt][qb][3]);
            }
            tmax[qb] = ug_max_groups(t);
        }
        // lazy reference point, as in flash_attn_kernel: a row's running max moves only when the tile max exceeds it by more than 2^8
        const bool up0 = (tmax[0] - m_run[0]) * c > 8.0f, up1 = (tmax[1] - m_run[1]) * c > 8.0f;
        if (!__all(!(up0 || up1))) {
            const float mn0 = up0 ? tmax[0] : m_run[0], mn1 = up1 ? tmax[1] : m_run[1];
            const float a0 = __builtin_amdgcn_exp2f((m_run[0] - mn0) * c), a1 = __builtin_amdgcn_exp2f((m_run[1] - mn1) * c);
            l_run[0] *= a0; l_run[1] *= a1;
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int r = 0; r < 4; ++r) { oacc[db][0][r] *= a0; oacc[db][1][r] *= a1; }
            m_run[0] = mn0; m_run[1] = mn1;
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const float mc = m_run[qb] * c;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                float p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    p[j] = __builtin_amdgcn_exp2f(fmaf(sacc[2 * ks + (j >> 2)][qb][j & 3], c, -mc));
                    l_run[qb] += p[j];
                }
                u32x4 w;
                w.x = pack2bf(p[0], p[1]); w.y = pack2bf(p[2], p[3]); w.z = pack2bf(p[4], p[5]); w.w = pack2bf(p[6], p[7]);
                pf[ks][qb] = __builtin_bit_cast(bf16x8, w);
            }
        }
    };
    // X(t) = P.V(t) then S^T(t + 1) = K Q^T as an explicit, fenced stream: NU steps of 8 P.V MFMAs, then NS steps of 8 K Q^T MFMAs; every LDS
    // fragment is requested two steps (256 MFMA cycles) ahead of its MFMAs
    auto do_X = [&](int t, auto cur_c, bool have_qk) __attribute__((always_inline)) {
        constexpr int CUR = decltype(cur_c)::value;
        const unsigned char* Vbuf = smem + CUR * 2 * TILE + TILE;
        const unsigned char* Kbuf = smem + (CUR ^ 1) * 2 * TILE;
        bf16x8 vf[NU][4], kf[NS][NKT];
        auto rdv = [&](int u) __attribute__((always_inline)) {
            const int ks = u / (NDB / 4), db0 = 4 * (u % (NDB / 4));
#pragma unroll
            for (int d = 0; d < 4; ++d)
                vf[u][d] = tr_read_pair(Vbuf + (2 * ks) * 16 * RB + voff[db0 + d], Vbuf + (2 * ks + 1) * 16 * RB + voff[db0 + d]);
        };
        auto rdk = [&](int s) __attribute__((always_inline)) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) kf[s][kt] = *(const bf16x8*)(Kbuf + kt * 16 * RB + k_rowoff + 16 * ((4 * s + g) ^ fk));
        };
        rdv(0);
        if constexpr (NU > 1) rdv(1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int ks = u / (NDB / 4), db0 = 4 * (u % (NDB / 4));
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                oacc[db0 + d][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][d], pf[ks][0], oacc[db0 + d][0], 0, 0, 0);
                oacc[db0 + d][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][d], pf[ks][1], oacc[db0 + d][1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (u + 2 < NU) rdv(u + 2);
            else if (have_qk && u + 2 - NU < NS) rdk(u + 2 - NU);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!have_qk) { if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(0); return; }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) { sacc[kt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; sacc[kt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                sacc[kt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s][kt], qf[0][s], sacc[kt][0], 0, 0, 0);
                sacc[kt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s][kt], qf[1][s], sacc[kt][1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (s + 2 < NS) { rdk(s + 2); __builtin_amdgcn_sched_barrier(0); }
        }
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(0);
        mask_ragged((t + 1) * KVB);
    };

    // ---- X | Y stagger with LDS-DMA staging: identical orchestration to flash_attn_kernel<.., STAGGER, .., DMA> ----
    auto seg_barrier = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    const bool groupA = __builtin_amdgcn_readfirstlane(wave) < 4;
    constexpr int RPI = 1024 / RB, NI = TILE / 1024, NIW = NI / 4;
    const int wb = __builtin_amdgcn_readfirstlane(wave) & 3;
    unsigned dko[NIW], dvo[NIW];
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int row = (wb * NIW + u) * RPI + lane / NCH;
        const int ch = (lane % NCH) ^ row_swz<DH>(row);
        dko[u] = (unsigned)(row * (int)k_rs + ch * 8) * 2u;        // bytes
        dvo[u] = (unsigned)(row * (int)v_rs + ch * 8) * 2u;
    }
    auto dma_tile = [&](const bf16_t* base, int64_t rs, const unsigned (&off)[NIW], int tile, unsigned dst) {
        if (tile * KVB + KVB <= Lkv) {
            const void* tb = uniform_ptr(base + (int64_t)tile * KVB * rs);
#pragma unroll
            for (int u = 0; u < NIW; ++u) glds16_off(tb, off[u], dst + u * 1024);
        } else {                                   // ragged last tile: rows past the end re-read the last key (masked in S^T)
            int lane_r = lane;
            asm volatile("" : "+v"(lane_r));
#pragma unroll
            for (int u = 0; u < NIW; ++u) {
                const int row = (wb * NIW + u) * RPI + lane_r / NCH;
                const int ch = (lane_r % NCH) ^ row_swz<DH>(row);
                int key = tile * KVB + row; if (key > Lkv - 1) key = Lkv - 1;
                glds16_ptr(base + (int64_t)key * rs + ch * 8, dst + u * 1024);
            }
        }
    };
    auto dma_fetch = [&](int kt, int vt) __attribute__((always_inline)) {
        const unsigned l0 = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wb * NIW * 1024;
        if (kt < ntiles) dma_tile(Kb, k_rs, dko, kt, l0 + (kt & 1) * 2 * TILE);
        if (vt < ntiles) dma_tile(Vb, v_rs, dvo, vt, l0 + (vt & 1) * 2 * TILE + TILE);
    };
    auto dma_wait = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    if (!groupA) { dma_fetch(0, ntiles); dma_wait(); }     // K(0) only
    seg_barrier();
    if (!groupA) dma_fetch(1, 0);
    if (!groupA) seg_barrier();                    // B idles through segment 0
    do_QK0();                                      // A: segment 0 | B: segment 1
    if (!groupA) dma_wait();
    seg_barrier();
    auto tile = [&](int t, auto cur_c) __attribute__((always_inline)) {
        if (!groupA) dma_fetch(t + 2, t + 1);
        if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(1);
        do_SM();
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) { asm volatile("" : "+v"(pf[ks][0])); asm volatile("" : "+v"(pf[ks][1])); }
        asm volatile("" : "+v"(l_run[0]), "+v"(l_run[1]), "+v"(m_run[0]), "+v"(m_run[1]));
        if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(0);
        seg_barrier();
        do_X(t, cur_c, t + 1 < ntiles);
        if (!groupA) dma_wait();
        seg_barrier();
    };
    for (int t = 0; t < ntiles; t += 2) {
        tile(t, std::integral_constant<int, 0>{});
        if (t + 1 < ntiles) tile(t + 1, std::integral_constant<int, 1>{});
    }
    if (groupA) seg_barrier();                     // A's trailing (empty) segment pairs with B's last one

    // ---- epilogue: O[q][d] = O^T / l. Lane (i, g) holds, per (db, qb), columns 16 db + 4 g .. + 3 of row 16 qb + i ----
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float l_tot = ug_sum_groups(l_run[qb]);
        if (lse_out != nullptr && g == 0 && q_row[qb] < Lq) lse_out[(int64_t)bh * lse_ld + q_row[qb]] = __builtin_amdgcn_logf(l_tot) + m_run[qb] * c;
        const float inv = 1.0f / l_tot;
        // v_permlane16_swap on the d-block pair (db, db + 1): afterwards an even lane group holds columns 16 db + 4 g .. + 7 (its own block-db
        // data and group g + 1's), an odd one columns 16 (db + 1) + 4 (g - 1) .. + 7: ONE 16-byte store per pair (cdna guide T21)
        bf16_t* Orow = o + (int64_t)b * o_bs + (int64_t)(q_row[qb] < Lq ? q_row[qb] : Lq - 1) * o_rs + head * DH + ((g & 1) ? 16 + 4 * (g - 1) : 4 * g);
#pragma unroll
        for (int db = 0; db < NDB; db += 2) {
            unsigned ax = pack2bf(oacc[db][qb][0] * inv, oacc[db][qb][1] * inv), ay = pack2bf(oacc[db][qb][2] * inv, oacc[db][qb][3] * inv);
            unsigned bx = pack2bf(oacc[db + 1][qb][0] * inv, oacc[db + 1][qb][1] * inv), by = pack2bf(oacc[db + 1][qb][2] * inv, oacc[db + 1][qb][3] * inv);
            const auto rx = __builtin_amdgcn_permlane16_swap(ax, bx, false, false);
            const auto ry = __builtin_amdgcn_permlane16_swap(ay, by, false, false);
            u32x4 w; w.x = rx[0]; w.y = ry[0]; w.z = rx[1]; w.w = ry[1];
            if (q_row[qb] < Lq) *(u32x4*)(Orow + 16 * db) = w;
        }
    }
}

// =====================================================================================================================
// One wave per SIMD ("pwg"): 4 waves x 64 query rows, up to 512 registers per lane, software-pipelined inside the wave.
//
// The 8-wave loop above keeps the matrix pipe ~42 % busy: its two waves per SIMD reach the MFMA segments and the softmax
// segments together. Here a single in-order wave per SIMD overlaps the two itself:
//     iteration t:   S1 = [ online softmax of S(t) (VALU)  interleaved with  O^T += V^T P^T of tile t-1 (32 MFMAs) ]
//                    S2 = [ S^T(t+1) = K Q^T (32 MFMAs) ]
// Per 64-key tile a wave issues 64 MFMAs for 64 query rows (every K / V fragment read from LDS feeds two MFMAs - half the LDS
// traffic per FLOP of the 32-row waves) against ~260 VALU instructions placed in the MFMA gaps of S1.
// LDS: 2 K slots + 2 V slots (64 KB), one barrier per tile: iteration t writes K(t+2) and V(t) (fetched to registers one
// iteration earlier) into the slots whose last readers finished before the barrier at its top, and fetches K(t+3), V(t+1).
// =====================================================================================================================
template <int DH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void flash_attn_pwg_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */) {
    constexpr int RB = 2 * DH, NCH = DH / 8, TILE = KVB * RB, QS = DH / 16, NDB = DH / 32;
    constexpr int NT = 256, NST = (KVB * NCH) / NT;
    static_assert(NST >= 1, "tile smaller than the workgroup");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // K slot 0 | K slot 1 | V slot 0 | V slot 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    const int nwg = gridDim.x;
    const int qd = nwg >> 3, rm = nwg & 7;
    const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
    const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + kk;
    const int qt = logical % nQ;
    const int bh = logical / nQ;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* Qb = q + (int64_t)b * q_bs + head * DH;
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * DH;

    // ---- Q fragments of the wave's two 32-row blocks (B operand of S^T = K Q^T): lane (r, h) holds Q[r][16 s + 8 h + j]. They are parked
    // in AGPRs (hipcc does not feed MFMA B operands from AGPRs) and copied to VGPRs one k-step ahead of their MFMAs, 8 v_accvgpr_read per
    // step in the MFMA shadow. Re-reading them from LDS instead doubled the QK^T segment's LDS traffic to ~75 % of the LDS array. ----
    bf16x8 qf[2][QS];
    int q_row[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        q_row[qb] = qt * 256 + wave * 64 + qb * 32 + r;
        const int q_ld = q_row[qb] < Lq ? q_row[qb] : Lq - 1;
#pragma unroll
        for (int s = 0; s < QS; ++s) qf[qb][s] = *(const bf16x8*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)      // retire the loads here (see the 8-wave kernel) and pin the class
#pragma unroll
        for (int s = 0; s < QS; ++s) asm volatile("" : "+a"(qf[qb][s]));
    // ---- staging: thread -> NST chunks of K and of V per tile ----
    int st_off[NST], st_row[NST], st_col[NST];
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const int cid = tid + NT * u;
        st_row[u] = cid / NCH;
        st_col[u] = (cid % NCH) * 8;
        st_off[u] = img_off<DH>(st_row[u], cid % NCH);
    }
    u32x4 kreg[NST], vreg[NST];
    auto fetch_k = [&](int kv0) {
#pragma unroll
        for (int u = 0; u < NST; ++u) { int key = kv0 + st_row[u]; if (key > Lkv - 1) key = Lkv - 1; kreg[u] = *(const u32x4*)(Kb + (int64_t)key * k_rs + st_col[u]); }
    };
    auto fetch_v = [&](int kv0) {
#pragma unroll
        for (int u = 0; u < NST; ++u) { int key = kv0 + st_row[u]; if (key > Lkv - 1) key = Lkv - 1; vreg[u] = *(const u32x4*)(Vb + (int64_t)key * v_rs + st_col[u]); }
    };
    auto write_k = [&](int slot) {
#pragma unroll
        for (int u = 0; u < NST; ++u) *(u32x4*)(smem + slot * TILE + st_off[u]) = kreg[u];
    };
    auto write_v = [&](int slot) {
#pragma unroll
        for (int u = 0; u < NST; ++u) *(u32x4*)(smem + (2 + slot) * TILE + st_off[u]) = vreg[u];
    };

    // ---- per-lane LDS read offsets (same images as the 8-wave kernel). Every swizzled offset is BASE ^ constant: the XOR only touches
    // bits 4-7, which the row term (multiple of 256) and the 8-byte term leave free. The segments re-derive their 8-16 addresses from
    // an opaque copy of the base (one v_xor each) - kept as loop invariants, hipcc held ~40 address registers and spilled them. ----
    static_assert(DH == 128, "XOR-folded offsets assume 256-byte rows");
    const int kx = h ^ row_swz<DH>(r);
    const int k_base = RB * r + 16 * kx;                                   // K fragment s, key block kb: kb * 32 * RB + (k_base ^ 32 s)
    const int i16 = lane & 15, g16 = lane >> 4;
    const int v_key = 4 * h + (i16 >> 2);
    const int v_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1);
    const int v_b8 = 8 * (i16 & 1);
    const int vlo_base = RB * v_key + 16 * (v_lowch ^ row_swz<DH>(v_key)) + v_b8;          // d-block db, k-step ks: ks * 16 * RB + (base ^ 64 db)
    const int vhi_base = RB * (v_key + 8) + 16 * (v_lowch ^ row_swz<DH>(v_key + 8)) + v_b8;

    f32x16 oacc[2][NDB];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[qb][db][i] = 0.f;
    // Register classes are pinned through empty asm operands: O^T accumulators, Q fragments and the staging registers are touched
    // only by MFMA / memory instructions and live in AGPRs; S^T and P^T are read and written by VALU and stay in VGPRs. Left to
    // itself hipcc accumulated S^T in AGPRs and moved ~500 registers per tile through v_accvgpr_read / _write.
    auto pin_o = [&]() {
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int db = 0; db < NDB; ++db) asm("" : "+a"(oacc[qb][db]));
    };
    pin_o();
    f32x16 sacc[2][2];                                   // [query block][key block] of the tile between its QK^T and its softmax
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f}, alpha[2] = {1.f, 1.f};
    bf16x8 pf[2][2][2][2];                               // P^T fragments [tile parity][query block][key block][half]
    const int ntiles = (Lkv + KVB - 1) / KVB;

    // The segments below are written as explicit instruction streams: sched_barrier(0) after every piece keeps hipcc from
    // re-clumping them (left to the scheduler - with or without sched_group_barrier - the softmax VALU work ended up in runs of 60-70
    // instructions between MFMAs, and a lone wave per SIMD has nobody to cover a stalled pipe). Measured with s_memtime stamps: a
    // segment that is VALU-bound costs its VALU cycles + ~16 per MFMA, one that is MFMA-bound 32 per MFMA. Hence three segments:
    //   A: P.V(t-1), 32 MFMAs  | row maxima of both query blocks, then the 32 exp elements of query block 0
    //   B: S^T(t+1) of query block 0, 16 MFMAs into the S registers block 0 just released | the 32 exp elements of query block 1
    //   C: S^T(t+1) of query block 1, 16 MFMAs | the staging pieces (8 LDS writes, 8 global loads)
#define UG_FENCE() __builtin_amdgcn_sched_barrier(0)
    float mc[2], lsum[2];
    // one exp element of the lane: query block qb = e / 32, key block (e / 16) % 2; packs a finished group of 8 into pf[PP]
    auto sm_elems = [&](int e0, int e1, auto pp_c, float (&p)[2][32]) __attribute__((always_inline)) {
        constexpr int PP = decltype(pp_c)::value;
#pragma unroll
        for (int e = e0; e < e1; ++e) {
            const int qb = e >> 5, kb = (e >> 4) & 1, x = e & 15;
            const float pe = __builtin_amdgcn_exp2f(fmaf(sacc[qb][kb][x], c, -mc[qb]));
            p[qb][e & 31] = pe;
            lsum[qb] += pe;
            if ((e & 7) == 7) {
                const int g = e >> 3, s2 = g & 1;
                const float* pg = &p[qb][(g & 3) * 8];
                u32x4 w;
                w.x = pack2bf(pg[0], pg[1]); w.y = pack2bf(pg[2], pg[3]); w.z = pack2bf(pg[4], pg[5]); w.w = pack2bf(pg[6], pg[7]);
                pf[PP][qb][kb][s2] = __builtin_bit_cast(bf16x8, w);
            }
            if ((e & 31) == 31) l_run[qb] = l_run[qb] * alpha[qb] + lsum[qb];
        }
    };
    float pbuf[2][32];
    // Segment A. Returns whether any lane's reference point moved (then O is rescaled by alpha after this segment).
    auto do_A = [&](auto slot_c, auto pp_c, auto pv_c) __attribute__((always_inline)) -> int {
        constexpr int SLOT = decltype(slot_c)::value, PP = decltype(pp_c)::value;
        constexpr bool HAVE_PV = decltype(pv_c)::value;
        const unsigned char* Vbuf = smem + (2 + SLOT) * TILE;
        int vl0 = vlo_base, vh0 = vhi_base;
        asm volatile("" : "+v"(vl0), "+v"(vh0));
        // P.V order: k-step outer, then d-block, then query block: the 8 accumulators rotate
        bf16x8 vf[4][NDB];
        auto rdv = [&](int ks) {
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                vf[ks][db] = tr_read_pair(Vbuf + ks * 16 * RB + (vl0 ^ (64 * db)), Vbuf + ks * 16 * RB + (vh0 ^ (64 * db)));
        };
        if constexpr (HAVE_PV) { rdv(0); UG_FENCE(); }
        int moved = 0;
        float tmax[2];
        lsum[0] = 0.f; lsum[1] = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if constexpr (HAVE_PV) {
                const int ks = i >> 3, db = (i >> 1) & 3, qb = i & 1;
                oacc[qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks][db], pf[PP ^ 1][qb][ks >> 1][ks & 1], oacc[qb][db], 0, 0, 0);
                UG_FENCE();
                if ((i & 7) == 1 && ks + 1 < 4) { rdv(ks + 1); UG_FENCE(); }
            }
            if (i < 8) {
                // maxima: piece i covers 8 of the 32 values of query block i / 4
                const int qb = i >> 2, part = i & 3, kb = part >> 1, o8 = 8 * (part & 1);
                const f32x16& sv = sacc[qb][kb];
                float m8 = ug_max3(sv[o8], sv[o8 + 1], sv[o8 + 2]);
                m8 = ug_max3(m8, sv[o8 + 3], sv[o8 + 4]);
                m8 = ug_max3(m8, sv[o8 + 5], sv[o8 + 6]);
                tmax[qb] = part == 0 ? ug_max3(m8, sv[o8 + 7], sv[o8 + 7]) : ug_max3(tmax[qb], m8, sv[o8 + 7]);
                if (part == 3) {
                    // Lazy running max: the reference point of a row moves only when the tile maximum exceeds it by more than 2^8 in
                    // the exponent (softmax is shift-invariant; P and l then stay below 2^8 per element, exact in fp32 / same relative
                    // precision in bf16). With an exact max some row of the 64 moves in nearly every tile and the O^T rescale - a
                    // round trip of 128 accumulators through VGPRs, ~2500 cycles - ran every iteration.
                    const float tm = ug_max_halves(tmax[qb]);
                    const bool up = (tm - m_run[qb]) * c > 8.0f;
                    const float m_new = up ? tm : m_run[qb];
                    moved |= !__all(!up);
                    alpha[qb] = __builtin_amdgcn_exp2f((m_run[qb] - m_new) * c);     // 1 where the point stayed, 0 on the first tile
                    m_run[qb] = m_new;
                    mc[qb] = m_new * c;
                }
            } else {
                const int j = i - 8;                     // 24 pieces x 4/3 elements: query block 0
                sm_elems((j * 4) / 3, ((j + 1) * 4) / 3, pp_c, pbuf);
            }
            UG_FENCE();
        }
        if constexpr (HAVE_PV) pin_o();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) { asm volatile("" : "+v"(pf[PP][0][kb][0])); asm volatile("" : "+v"(pf[PP][0][kb][1])); }
        return moved;
    };
    // S^T(t)[query block QB] = K Q^T from K slot SLOT (16 MFMAs, k-step outer, the 2 key-block accumulators alternate). These MFMAs are
    // inline asm: S^T accumulates in VGPRs (where the softmax reads it) and the Q fragment comes straight from its AGPRs. As a builtin,
    // hipcc accumulates in AGPRs in a 512-register kernel and copies Q to VGPRs: +128 v_accvgpr_read and 64 more live registers per
    // tile. hipcc does not see an MFMA here, so the hazards are ours: operands come from ds_read / AGPRs (waitcnt is tracked through
    // the asm operands) and the results are first read by VALU behind the s_nops that close segment C or behind the next barrier.
    // FILL(ks) is called after the MFMAs of k-step ks: the VALU / memory work this segment shadows.
    auto do_QK = [&](int t, auto slot_c, auto qb_c, auto&& fill) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_c)::value, QB = decltype(qb_c)::value;
        const unsigned char* Kbuf = smem + SLOT * TILE;
        int kb0 = k_base;
        asm volatile("" : "+v"(kb0));
        constexpr int AHEAD = 3;
        bf16x8 kf[QS][2];
        auto rd = [&](int ks) {
            kf[ks][0] = *(const bf16x8*)(Kbuf + (kb0 ^ (32 * ks)));
            kf[ks][1] = *(const bf16x8*)(Kbuf + 32 * RB + (kb0 ^ (32 * ks)));
        };
#pragma unroll
        for (int ks = 0; ks < AHEAD; ++ks) rd(ks);
        UG_FENCE();
#pragma unroll
        for (int ks = 0; ks < QS; ++ks) {
            if (ks + AHEAD < QS) rd(ks + AHEAD);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (ks == 0) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(sacc[QB][kb]) : "v"(kf[ks][kb]), "a"(qf[QB][ks]));
                else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(sacc[QB][kb]) : "v"(kf[ks][kb]), "a"(qf[QB][ks]));
            }
            UG_FENCE();
            fill(ks);
            UG_FENCE();
        }
    };
    auto mask_tail = [&](int t) __attribute__((always_inline)) {        // ragged last tile: keys >= Lkv do not exist
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 7" ::: "memory");   // the last MFMAs' results (8 passes) before any VALU read
        if (t * KVB + KVB > Lkv) {
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = t * KVB + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (key >= Lkv) sacc[qb][kb][i] = -INFINITY;
                    }
        }
    };
    // one staging piece of segment C of iteration t_it (computing S^T(t_it + 1)): pieces 0-7 publish K(t_it+2) / V(t_it) into the
    // slots of parity t_it & 1, pieces 8-15 fetch K(t_it+3) / V(t_it+1). Tiles past the end are clamped re-reads nobody consumes.
    auto stage_piece = [&](int pc, int t_it, int wslot) __attribute__((always_inline)) {
        constexpr int W = 2 * NST;
        if (pc < NST) *(u32x4*)(smem + wslot * TILE + st_off[pc]) = kreg[pc];
        else if (pc < W) *(u32x4*)(smem + (2 + wslot) * TILE + st_off[pc - NST]) = vreg[pc - NST];
        else if (pc < 2 * W) {
            const bool isk = pc < W + NST;
            const int u = isk ? pc - W : pc - W - NST;
            int tile = isk ? t_it + 3 : t_it + 1; if (tile > ntiles - 1) tile = ntiles - 1;              // wave-uniform
            const int rmax = Lkv - 1 - tile * KVB;
            const int row = st_row[u] < rmax ? st_row[u] : rmax;
            if (isk) kreg[u] = *(const u32x4*)(Kb + (int64_t)tile * KVB * k_rs + (unsigned)(row * (int)k_rs + st_col[u]));
            else vreg[u] = *(const u32x4*)(Vb + (int64_t)tile * KVB * v_rs + (unsigned)(row * (int)v_rs + st_col[u]));
        }
    };

    // ---- prologue: K(0), K(1) in LDS, S(0) computed, K(2) and V(0) in registers ----
    fetch_k(0);
    write_k(0);
    fetch_k(KVB);                                        // clamped re-read when there is a single tile
    write_k(1);
    __syncthreads();
    auto nofill = [&](int) {};
    do_QK(0, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, nofill);
    do_QK(0, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, nofill);
    mask_tail(0);
    fetch_k(2 * KVB);
    fetch_v(0);

    auto rescale_o = [&]() __attribute__((always_inline)) {   // rare (a row's reference point moved): one accumulator at a time through VGPRs
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                f32x16 x = oacc[qb][db];
                asm volatile("" : "+v"(x));
#pragma unroll
                for (int i = 0; i < 16; ++i) x[i] *= alpha[qb];
                asm volatile("" : "+a"(x));
                oacc[qb][db] = x;
            }
    };
    // Iteration t: barrier | A | (rescale) | B | C. C also publishes K(t+2) -> K slot t & 1 and V(t) -> V slot t & 1 (their last
    // readers, QK(t) and P.V(t-2), finished before the barrier) and fetches K(t+3), V(t+1).
    auto iter = [&](int t, auto par_c, auto pv_c) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value;     // t & 1
        using CUR = std::integral_constant<int, PAR>;
        using OTH = std::integral_constant<int, PAR ^ 1>;
        __syncthreads();
        // S^T is "redefined" here so that its softmax cannot be hoisted above the barrier, away from the P.V MFMAs it must shadow
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) asm volatile("" : "+v"(sacc[qb][kb]));
        const int moved = do_A(OTH{}, CUR{}, pv_c);
        if (decltype(pv_c)::value && moved) rescale_o();
        if (t + 1 < ntiles) {
            // B: 2 exp elements of query block 1 per MFMA (hipcc hoists most of this pure chain up into segment A; pinning it here
            // measured 3 % slower)
            do_QK(t + 1, OTH{}, std::integral_constant<int, 0>{}, [&](int ks) __attribute__((always_inline)) { sm_elems(32 + 4 * ks, 36 + 4 * ks, CUR{}, pbuf); });
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) { asm volatile("" : "+v"(pf[PAR][1][kb][0])); asm volatile("" : "+v"(pf[PAR][1][kb][1])); }
            // C: 2 staging pieces per k-step
            do_QK(t + 1, OTH{}, std::integral_constant<int, 1>{}, [&](int ks) __attribute__((always_inline)) { stage_piece(2 * ks, t, PAR); stage_piece(2 * ks + 1, t, PAR); });
            mask_tail(t + 1);
        } else {
            sm_elems(32, 64, CUR{}, pbuf);               // last tile: the rest of its softmax, and V(t) is still to be published
            write_v(PAR);
        }
    };
    iter(0, std::integral_constant<int, 0>{}, std::false_type{});       // no P.V yet (O is zero: nothing to rescale)
    for (int t = 1; t < ntiles; t += 2) {
        iter(t, std::integral_constant<int, 1>{}, std::true_type{});
        if (t + 1 < ntiles) iter(t + 1, std::integral_constant<int, 0>{}, std::true_type{});
    }
#undef UG_FENCE
    __syncthreads();                                     // V(ntiles-1) visible
    auto tail_PV = [&](auto par_c) {                     // O^T += V^T P^T of the last tile
        constexpr int PAR = decltype(par_c)::value;
        const unsigned char* Vbuf = smem + (2 + PAR) * TILE;
        int vl0 = vlo_base, vh0 = vhi_base;
        asm volatile("" : "+v"(vl0), "+v"(vh0));
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 vfr = tr_read_pair(Vbuf + ks * 16 * RB + (vl0 ^ (64 * db)), Vbuf + ks * 16 * RB + (vh0 ^ (64 * db)));
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
                    oacc[qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr, pf[PAR][qb][ks >> 1][ks & 1], oacc[qb][db], 0, 0, 0);
            }
    };
    if ((ntiles - 1) & 1) tail_PV(std::integral_constant<int, 1>{}); else tail_PV(std::integral_constant<int, 0>{});

    // ---- epilogue: O[q][d] = O^T / l ----
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float l_tot = l_run[qb] + __shfl_xor(l_run[qb], 32, 64);
        const float inv = 1.0f / l_tot;
        if (q_row[qb] < Lq) {
            bf16_t* Orow = o + (int64_t)b * o_bs + (int64_t)q_row[qb] * o_rs + head * DH;
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    u32x2 w;
                    w.x = pack2bf(oacc[qb][db][4 * g4 + 0] * inv, oacc[qb][db][4 * g4 + 1] * inv);
                    w.y = pack2bf(oacc[qb][db][4 * g4 + 2] * inv, oacc[qb][db][4 * g4 + 3] * inv);
                    *(u32x2*)(Orow + 32 * db + 8 * g4 + 4 * h) = w;
                }
        }
    }
}

}  // namespace

// Called by flash_attn_fwd_impl (attention.hip) with the arguments it has validated.
int ug_attn_fwd_variants(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride, int64_t k_batch_stride,
                         const void* v, int64_t v_row_stride, int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                         int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale, float* lse_out, int64_t lse_ld,
                         ug_stream_t stream) {
#define UG_ATTN_LAUNCH_KV(KVV, OCCV, LS, BUF, DHV, NWV, STG, ...)                                                                                  \
    hipLaunchKernelGGL((flash_attn_var_kernel<DHV, NWV, STG, __VA_ARGS__, KVV, OCCV, LS, BUF>), dim3((unsigned)nwg), dim3(64 * NWV), 2 * 2 * KVV * 2 * DHV + (STG ? 32 * NWV * 2 * DHV : 0), (hipStream_t)stream, \
                       (const bf16_t*)q, q_row_stride, q_batch_stride, (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, \
                       v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride, (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld)
    static int nw = -1;
    if (nw < 0) { const char* e = getenv("UG_ATTN_WAVES"); nw = (e && atoi(e) == 4) ? 4 : 8; }   // 8 measured faster (841 vs 800 TFLOP/s at L = 4608)
    const int qrows = 32 * nw;
    const int nQ = (int)((Lq + qrows - 1) / qrows);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd: grid too large");
    const float c = softmax_scale * 1.4426950408889634f;
#define UG_ATTN_LAUNCH(DHV, NWV, STG, ...)                                                                                           \
    hipLaunchKernelGGL((flash_attn_var_kernel<DHV, NWV, STG, ##__VA_ARGS__>), dim3((unsigned)nwg), dim3(64 * NWV), 2 * 2 * KVB * 2 * DHV + (STG ? 32 * NWV * 2 * DHV : 0), (hipStream_t)stream, \
                       (const bf16_t*)q, q_row_stride, q_batch_stride, (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, \
                       v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride, (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld)
    const int m16 = ug_env_int("UG_ATTN_M16", 0);                     // 1: always, -1: head width 128 from 2048 keys on (what round 4 tried in the product), 0: never
    if (dh == 128 && nw == 8 && (m16 == 1 || (m16 < 0 && Lkv >= 2048))) {       // round 4: the stagger kernel on v_mfma_f32_16x16x32_bf16
        const int pr16 = ug_env_int("UG_ATTN_PRIO", 0);
        if (pr16 == 1)
            hipLaunchKernelGGL((flash_attn_m16_kernel<128, 1>), dim3((unsigned)nwg), dim3(512), 4 * 64 * 2 * 128, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride,
                               (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride,
                               (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld);
        else if (pr16 == 3)
            hipLaunchKernelGGL((flash_attn_m16_kernel<128, 3>), dim3((unsigned)nwg), dim3(512), 4 * 64 * 2 * 128, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride,
                               (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride,
                               (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld);
        else
            hipLaunchKernelGGL((flash_attn_m16_kernel<128, 0>), dim3((unsigned)nwg), dim3(512), 4 * 64 * 2 * 128, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride,
                               (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride,
                               (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld);
        UG_CHECK_LAUNCH("ug_flash_attn_fwd");
        return UG_OK;
    }
    if (dh == 64 && nw == 8 && m16 == 1) {        // head width 64 on the same kernel (one workgroup per CU): A/B only
        hipLaunchKernelGGL((flash_attn_m16_kernel<64, 0>), dim3((unsigned)nwg), dim3(512), 4 * 64 * 2 * 64, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride,
                           (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride,
                           (int)heads, (int)Lq, (int)Lkv, nQ, c, lse_out, lse_ld);
        UG_CHECK_LAUNCH("ug_flash_attn_fwd");
        return UG_OK;
    }
    static int pwg = -1;
    if (pwg < 0) { const char* e = getenv("UG_ATTN_PWG"); pwg = e ? atoi(e) : 0; }
    if (pwg && dh == 128 && !lse_out) {
        const int nQp = (int)((Lq + 255) / 256);
        const int64_t nwgp = (int64_t)nQp * heads * batches;
        static bool attr = false;
        if (!attr) { (void)hipFuncSetAttribute((const void*)flash_attn_pwg_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * KVB * 2 * 128); attr = true; }
        hipLaunchKernelGGL((flash_attn_pwg_kernel<128>), dim3((unsigned)nwgp), dim3(256), 4 * KVB * 2 * 128, (hipStream_t)stream,
                           (const bf16_t*)q, q_row_stride, q_batch_stride, (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v,
                           v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride, (int)heads, (int)Lq, (int)Lkv, nQp, c);
        UG_CHECK_LAUNCH("ug_flash_attn_fwd");
        return UG_OK;
    }
    static int stagger = -1;
    // UG_ATTN_STAGGER=0 selects the lock-step loop; default: the X|Y stagger. Same-box A/B after the branch-free fetch and the softmax pin
    // (before them the stagger variant measured 602 vs 842): dh = 128: 989 vs 955 TFLOP/s at L = 4608, 1027 vs 1007 (4096 x 4608),
    // 1068 vs 1044 (8192), 956 vs 933 (B16, 2048); dh = 64 inside the SD3.5 forward: 795 vs 775.
    if (stagger < 0) { const char* e = getenv("UG_ATTN_STAGGER"); stagger = (e && atoi(e) == 0) ? 0 : 1; }
    const bool stg = stagger == 1;
    // UG_ATTN_PRIO = 0 | 1 | 2 | 3, UG_ATTN_WIDE = 0 | 1: A/B switches of the stagger kernel (re-read per call when UG_ENV_DYNAMIC=1)
    // Interleaved A/B, round 2 (tools/attn_ab.py, same process): prio 0 + wide stores is the fastest form everywhere - dh 128: 1137 / 1147 / 1178
    // vs 1124 / 1133 / 1172 TFLOP/s for the round-1 default (prio 1, narrow) at 4608^2 / 4096x4608 / 8192x8704; dh 64: 880-885 vs 856-871; the
    // static young-half priority (2) loses 1-2 % at dh 128.
    // UG_ATTN_PRIO = 3 (DMA variant): s_setprio 1 around the softmax segment - it is the longer one of each segment pair (loop ablations,
    // profiles/r02f_attn_bwd.log). Interleaved A/B, 12 of 12 pairs: +0.3-0.5 % at dh 128 (1137 -> 1141, 1153 -> 1158, 1185 -> 1191 TFLOP/s);
    // dh 64: -0.5 % (within noise) -> default 3 at dh 128, 0 at dh 64.
    const int prio = ug_env_int("UG_ATTN_PRIO", dh == 128 ? 3 : 0), wide = ug_env_int("UG_ATTN_WIDE", 1), dma = ug_env_int("UG_ATTN_DMA", 1);
#define UG_ATTN_STG(DHV)                                                                          \
    do {                                                                                          \
        if (dma && prio == 3) { UG_ATTN_LAUNCH(DHV, 8, true, 3, true, true); break; }             \
        if (dma) { UG_ATTN_LAUNCH(DHV, 8, true, 0, true, true); break; }                          \
        if (wide) { if (prio == 0 || prio == 3) UG_ATTN_LAUNCH(DHV, 8, true, 0, true); else if (prio == 2) UG_ATTN_LAUNCH(DHV, 8, true, 2, true); else UG_ATTN_LAUNCH(DHV, 8, true, 1, true); } \
        else { if (prio == 0 || prio == 3) UG_ATTN_LAUNCH(DHV, 8, true, 0, false); else if (prio == 2) UG_ATTN_LAUNCH(DHV, 8, true, 2, false); else UG_ATTN_LAUNCH(DHV, 8, true, 1, false); } \
    } while (0)
    // Head dim 64 (round 3, UG_ATTN_KV64): 464 (default) = 64-key tiles at <= 128 registers so that TWO workgroups share a CU; 128 = 128-key
    // tiles, one workgroup per CU; 64 = the round-2 kernel. Interleaved A/B (tools/attn_ab.py, profiles/r03e_attn_ab64.log): alone
    // 872 / 906 / 902 TFLOP/s (64 / 128 / 464) at 4096 x 4429, 886 / 920 / 912 at 4096^2; inside the SD3.5 forward, where other kernels'
    // tails and launches leave more bubbles to fill, 834 / 868 / 918 (0.4214 / 0.4144 / 0.4043 s per forward). 464 is bit-identical to 64.
    const int kv64 = ug_env_int("UG_ATTN_KV64", 464);
    if (dh == 128) { if (nw == 4) UG_ATTN_LAUNCH(128, 4, false); else if (stg) UG_ATTN_STG(128); else UG_ATTN_LAUNCH(128, 8, false); }
    else if (nw == 8 && stg && dma && kv64 == 128) {
        static bool attr = false;
        if (!attr) { (void)hipFuncSetAttribute((const void*)flash_attn_var_kernel<64, 8, true, 0, true, true, 128, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 2 * 128 * 2 * 64 + 32 * 8 * 2 * 64); attr = true; }
        UG_ATTN_LAUNCH_KV(128, 2, false, false, 64, 8, true, 0, true, true);
    }
    else if (nw == 8 && stg && dma && kv64 == 464) {        // UG_ATTN_KV64=464: 64-key tiles, <= 128 registers, two workgroups per CU
        UG_ATTN_LAUNCH_KV(64, 4, false, false, 64, 8, true, 0, true, true);
    }
    else           { if (nw == 4) UG_ATTN_LAUNCH(64, 4, false); else if (stg) UG_ATTN_STG(64); else UG_ATTN_LAUNCH(64, 8, false); }
#undef UG_ATTN_STG
#undef UG_ATTN_LAUNCH
#undef UG_ATTN_LAUNCH_KV
    UG_CHECK_LAUNCH("ug_flash_attn_fwd");
    return UG_OK;
}
