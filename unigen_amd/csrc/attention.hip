// Flash-style fused attention for the joint text|image|condition sequences of the UniGen MM-DiT blocks: the forward kernel that ships and the
// backward kernels.
//   O = softmax(Q K^T * scale) V, non-causal, no mask, bf16 in/out, fp32 scores / statistics / accumulators.
// Replaces F.scaled_dot_product_attention at src/UniGenUtils.py:601 (JointAttnRopeProcessor) and inside diffusers
// FluxAttnProcessor2_0 (base blocks, src/UniGenTransformer.py:1129,1151). L = 4608 / 8192 / 8704 at 1024^2.
//
// Forward structure (gfx950, wave64): one workgroup = 8 waves = 256 query rows of one (batch, head); each wave owns 32 query rows. K/V tiles
// of 64 keys go HBM -> LDS by LDS-DMA (no staging registers), double buffered, in an XOR-swizzled 256-byte-row image that is conflict-free
// for both the row reads (K, ds_read_b128) and the transposed reads (V, ds_read_b64_tr_b16); the two wave groups run one segment apart (X|Y stagger).
//   S^T = K Q^T   with v_mfma_f32_32x32x16_bf16: the query index lands on the LANE, so the softmax row statistics are
//                 lane-local (one exchange with lane^32 per tile for the max).
//   O^T = V^T P^T : the S^T accumulator registers 8s..8s+7, packed to bf16, ARE the B operand of k-step s (permuted k
//                 order, matched by the key order of the transposed V reads) - P never touches LDS or other lanes.
// This file holds only what the product dispatches. The device helpers shared with the probe kernels are in attn_common.h; every forward form that
// was measured and dropped (and the general ten-parameter template this kernel was cut from) is tools/probe/csrc/attn_fwd_variants.hip.
#include "ug_common.h"
#include "attn_common.h"
#include <type_traits>

namespace {


// The forward kernel: the X|Y stagger. Waves 0-3 (group A) and 4-7 (group B) - the two waves of every SIMD - run one segment apart. A wave
// alternates a matrix-only segment X(t) = P.V(t) then S^T(t+1) = K Q^T (32 MFMAs, an explicit fenced stream) with a VALU-only segment
// Y(t+1) = the online softmax of tile t+1, so a wave's softmax runs under its partner's MFMAs instead of both waves hitting the matrix pipe,
// then the VALU, together. Two barriers per tile. Everything but the head width and the DMA form is fixed; what follows from the head width:
//   DH = 128: one workgroup per CU (<= 256 registers), Q fragments in registers, row sums on the VALU, s_setprio 1 around every softmax segment
//             (PRIO 3: it is the longer one of each segment pair - +0.3-0.5 % in 12 of 12 interleaved pairs; -0.5 %, within noise, at DH 64).
//   DH =  64: <= 128 registers so that TWO workgroups share a CU (64 KiB of LDS each) - four waves per SIMD fill each other's barrier and latency
//             bubbles in the VALU-bound loop; Q fragments then come from LDS (QLDS: 16 registers fewer); row sums on the matrix pipe (LSUM).
// Staging: K / V tiles go HBM -> LDS with global_load_lds_dwordx4 (no staging registers, no ds_write): the swizzled image is produced on the
// SOURCE side (lane l of an instruction lands at byte 16 l of a 1 KiB run = 4 rows at dh 128, so it fetches chunk (l % 16) ^ f(row) of its
// row), and group B issues all of it at the start of its softmax segment, two segments ahead of use.
// BUFD (round 6; head width 64 only): the whole-tile LDS-DMAs in BUFFER form. The stamps put group B's softmax segment 770 cycles above group A's
// (2263 vs 1497), all of it the 4 DMA issues per wave and tile, i.e. the issue sequence itself: per tile ~20 VALU instructions of lane-offset re-derivation
// (kept out of registers in round 3), a 64-bit VALU pointer bump, two v_readfirstlane + s_nop 4 per operand, on a SIMD whose VALU the four waves'
// softmax already saturates. Here the per-lane byte offset is ONE VGPR held through the loop (run 1's is that ^ 16: needs K and V to share a row stride
// that is a multiple of 16 elements - the dispatcher checks), the (batch, head) base is an SGPR resource, the tile / run offset an SGPR: per tile
// 4 x (s_mov m0 + buffer_load ... lds), one v_xor, scalar adds.
// LSUM (round 6): the softmax row sums leave the VALU. With the scores' scale / exp2 / max / pack the running sum `l += p` is one of ~5
// VALU instructions per score and the softmax segment Y is what the barriers wait for (tools/attn_stamps.py); here each lane's probabilities are
// summed on the matrix pipe instead, inside X, from the SAME packed bf16 fragments P.V consumes: v_mfma_f32_4x4x4_16b_bf16 (16 blocks of 4x4x4) with
// A = ones makes D[b][i][j] = sum_k B[b][k][j], i.e. every lane gets the sum of the four bf16 values IT passes as B (lane = block b, column j),
// accumulated over the tile's 8 half-fragments: 8 two-pass MFMAs per tile and wave (+12.5 % matrix-pipe cycles) for 32 v_add_f32 (-20 % of the
// softmax segment's issue cycles). The denominator is then the sum of the ROUNDED probabilities - the ones the numerator multiplies - not of their
// fp32 originals (relative difference <= 2^-9 / sqrt(keys), below the output's own bf16 rounding). At head width 128 LSUM lost 4 % (X is its longer segment).
// (Round 6 also measured and dropped: five other assignments of the LDS-DMA issue to the wave groups, the buffer form at head width 128 and a
// second row-sum chain - stamps in profiles/r06b_*, rates in profiles/r06_attn_variants.log, code in tools/probe/patches/attn_r06_variants.diff.
// Every older form - lock-step loop, register staging, 4-wave workgroups, 128-key tiles, PRIO 1 / 2, 8-byte stores - is the frozen ten-parameter
// copy of this kernel in tools/probe/csrc/attn_fwd_variants.hip, with its numbers.)
template <int DH, bool BUFD>   // head dim 128 | 64; BUFD: buffer-form DMAs
__global__ __launch_bounds__(512, DH == 128 ? 2 : 4) void flash_attn_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */, float* __restrict__ lse_out /* nullable */, int64_t lse_ld) {
    constexpr int NW = 8;                            // waves per workgroup: 256 query rows
    constexpr int PRIO = DH == 128 ? 3 : 0;          // 3 = s_setprio 1 around every softmax segment Y; 0 = no priority games
    constexpr bool LSUM = DH == 64;                  // row sums on the matrix pipe
    constexpr bool QLDS = DH == 64;                  // Q fragments from LDS (the two-workgroups-per-CU register budget) or from registers
    constexpr int NKB = KVB / 32;                    // 32-key blocks of S^T per tile
    constexpr int NKS = KVB / 16;                    // k-steps of O^T += V^T P^T per tile
    constexpr int RB = 2 * DH;                       // row bytes
    constexpr int NCH = DH / 8;                      // 16-byte chunks per row
    constexpr int TILE = KVB * RB;                   // bytes of one K (or V) tile image
    constexpr int QS = DH / 16;                      // k-steps of S^T = K Q^T
    constexpr int NDB = DH / 32;                     // 32-wide d blocks of O^T
    constexpr int QROWS = 32 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][K tile | V tile] | Q image
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
    // The divisions run on the VALU, so hipcc takes their (wave-uniform) results for per-lane values: at head width 64 the (batch, head) base pointers
    // derived from them were 64-bit VGPR pairs, live through the loop, that the 128-register budget pushed to scratch (10-12 VGPRs, one reload per tile).
    const int qt = DH == 64 ? __builtin_amdgcn_readfirstlane(logical % nQ) : logical % nQ;
    const int bh = DH == 64 ? __builtin_amdgcn_readfirstlane(logical / nQ) : logical / nQ;
    const int head = DH == 64 ? __builtin_amdgcn_readfirstlane(bh % heads) : bh % heads, b = DH == 64 ? __builtin_amdgcn_readfirstlane(bh / heads) : bh / heads;

    const bf16_t* Qb = q + (int64_t)b * q_bs + head * DH;
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * DH;

    // ---- Q fragments (B operand of S^T = K Q^T): lane (r, h) holds Q[q = r][d = 16 s + 8 h + j] ----
    const int q_row = qt * QROWS + wave * 32 + r;
    const int q_ld = q_row < Lq ? q_row : Lq - 1;
    // QLDS: the fragments live in LDS (same swizzled row image as K, one ds_read_b128 per k-step) - S^T must survive a barrier next to
    // the P.V operands, and at head width 64 the registers are what the two-workgroups-per-CU form is short of.
    constexpr int QBASE = 2 * 2 * KVB * RB;            // byte offset of the Q image behind the two K|V buffers
    bf16x8 qf[QLDS ? 1 : QS];
    const int q_lds = QBASE + RB * (wave * 32 + r);
    const int qx = h ^ row_swz<DH>(r);                  // wave * 32 keeps row_swz unchanged (multiple of 16)
    if constexpr (!QLDS) {
#pragma unroll
        for (int s = 0; s < QS; ++s) qf[s] = *(const bf16x8*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);
        // Retire the Q loads HERE: the empty asm takes every fragment as a read-write operand, so hipcc must have the loaded
        // values in hand before it (it waits vmcnt there) and treats them as fresh afterwards. Without it the loads are sunk to
        // the loop header and every iteration re-waits for them with vmcnt(7..0), draining the K/V prefetch issued at its top.
        asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]), "+v"(qf[4]), "+v"(qf[5]), "+v"(qf[6]), "+v"(qf[7]));
    } else {
        // each lane copies the 16-byte chunks (16 s + 8 h) of its own query row; only this wave reads them back
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const u32x4 v4 = *(const u32x4*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);
            *(u32x4*)(smem + q_lds + 16 * ((2 * s) ^ qx)) = v4;
        }
    }

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
    f32x4 lacc = {0.f, 0.f, 0.f, 0.f};                 // LSUM: register 0 = half of this lane's running row sum (rows 1-3 of its 4x4 block: unused copies)
    bf16x4 ones4 = {(short)0x3f80, (short)0x3f80, (short)0x3f80, (short)0x3f80};
    if constexpr (LSUM) asm volatile("" : "+v"(ones4));        // one VGPR pair for the loop, not re-materialised per use

    const int ntiles = (Lkv + KVB - 1) / KVB;
    bf16x8 pf[NKB][2];                                 // P^T fragments of the tile between its S and P stages
    // CUR = buffer parity as a compile-time constant: every LDS address below is then a loop-invariant VGPR + an immediate offset
    // (with a runtime parity hipcc re-materialised ~50 address adds per tile, a quarter of the VALU work of the loop).
    f32x16 sacc[NKB];                                  // S^T of the tile between its QK^T and its softmax
    auto do_QK = [&](int t, auto cur_c) __attribute__((always_inline)) {      // the prologue's S^T(0); every later one is the second half of do_X
        constexpr int CUR = decltype(cur_c)::value;
        const int kv0 = t * KVB;
        const unsigned char* Kbuf = smem + CUR * 2 * TILE;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
        // per k-step one Q fragment (from LDS under QLDS) and the two key blocks' K fragments, read two steps ahead of their
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
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);        // fragments of k-steps 0, 1
#pragma unroll
        for (int s = 0; s < QS - 2; ++s) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);    // MFMAs of step s
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);    // fragments of step s + 2
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
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
        // (softmax is shift-invariant; P and l stay below 2^8 per element: exact in fp32, same relative precision in bf16 - a dominant
        // probability then carries a bf16 rounding of its own, up to 2x the worst-row error of the exact maximum on such rows: measured in
        // docs/PARITY_TOLERANCES.md, "Attention regimes sweep"). With the exact max some row of the wave moves in most tiles and the
        // 64-register rescale below ran nearly every iteration.
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
    // X(t) as an explicit stream (sched_barrier after every piece): P.V(t) - 16 MFMAs, k-step outer so the 4
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
        if (!have_qk) return;
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
    // The segments (PMC on the lock-step loop this replaced: matrix pipe busy 42 %, VALU 45 %, hardly overlapping):
    //   global segment:   0       1       2       3       4
    //   group A:        QK(0)    Y(0)    X(0)    Y(1)    X(1) ...
    //   group B:          -     QK(0)    Y(0)    X(0)    Y(1) ...
    // K(t+1) and V(t) are first needed in segment 2t+2: group B issues their DMAs at the START of its softmax segment Y(t-1) (global segment 2t)
    // and waits for them at the END of its X(t-1) (segment 2t+1), into buffers nobody reads in 2t / 2t+1. DMAs cross barriers: raw s_barrier.
    auto seg_barrier = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    const bool groupA = __builtin_amdgcn_readfirstlane(wave) < NW / 2;
    // LDS-DMA staging: a tile image is NI runs of 1 KiB (RPI rows each); wave wb of group B owns runs wb * NIW .. + NIW - 1
    // (measured and dropped: every wave issuing NI / 8 runs, group A's half at the start of its own softmax segment 2t+1 and waited for
    // at its end - same bits, -0.5 % at dh 128, -12 % at dh 64: group B's issue cost is not what bounds the segment pairs; and group A
    // issuing all of them one at a time behind the MFMAs of the first 2 NIW steps of its matrix segment: -11 % / -4 %, ~46 cycles of
    // matrix-segment time per DMA)
    constexpr int RPI = 1024 / RB, NI = TILE / 1024, NIW = NI / (NW / 2);
    const int wb = __builtin_amdgcn_readfirstlane(wave) & (NW / 2 - 1);
    unsigned dko[NIW], dvo[NIW];
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int row = (wb * NIW + u) * RPI + lane / NCH;
        const int ch = (lane % NCH) ^ row_swz<DH>(row);
        dko[u] = (unsigned)(row * (int)k_rs + ch * 8) * 2u;        // bytes
        dvo[u] = (unsigned)(row * (int)v_rs + ch * 8) * 2u;
    }
    static_assert(!BUFD || DH == 64, "BUFD is the head-width-64, two-workgroups-per-CU form of the LDS-DMA staging (it derives run 1 of a wave's two from run 0)");
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
            } else if constexpr (DH == 64) {
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
    if (!groupA) { dma_fetch(0, ntiles); dma_wait(); }     // K(0) only
    seg_barrier();
    if (!groupA) dma_fetch(1, 0);
    if (!groupA) seg_barrier();                    // B idles through segment 0
    UG_ASTAMP(1);
    do_QK(0, std::integral_constant<int, 0>{});    // A: segment 0 | B: segment 1
    if (!groupA) dma_wait();                       // end of segment 1 (B)
    seg_barrier();
    // one tile = Y(t) | X(t); buffer parity is a compile-time constant (two tiles per trip)
    auto tile = [&](int t, auto cur_c) __attribute__((always_inline)) {
        // Y(t): A in odd segment 2t+1 | B in even segment 2t+2 (issues the DMAs of K(t+2), V(t+1) at its start)
        if (!groupA) dma_fetch(t + 2, t + 1);
        if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(1);                  // the softmax segment outranks the partner's matrix stream at issue
        do_SM();
        // P^T is "used" here: hipcc otherwise sinks the (pure) scale / exp2 / pack chain across the barrier to its first use, the
        // P.V MFMAs - i.e. out of this VALU-only segment into the matrix-only one, which then ran at ~60 cycles per MFMA
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) { asm volatile("" : "+v"(pf[kb][0])); asm volatile("" : "+v"(pf[kb][1])); }
        if constexpr (LSUM) asm volatile("" : "+v"(m_run)); else asm volatile("" : "+v"(l_run), "+v"(m_run));
        if constexpr (PRIO == 3) __builtin_amdgcn_s_setprio(0);
        UG_SEG(0);
        seg_barrier();
        UG_SEG(1);
        // X(t) = P.V(t) then K.Q^T(t+1): A in even segment 2t+2 | B in odd segment 2t+3 (waits for its DMAs). (Measured and dropped: group B
        // reading its first V^T fragments ahead of the barrier, inside its softmax segment: -4 %, -10 % with two k-steps.)
        do_X(t, cur_c, t + 1 < ntiles);
        if (!groupA) dma_wait();
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

    // ---- epilogue: O[q][d] = O^T / l ----
    if constexpr (LSUM) l_run = lacc[0];
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    // training: log2 sum_k 2^(c s) of the row for the backward kernels (m_run is the row's reference point, shared by both lane halves)
#ifndef UG_ATTN_STAMPS
    if (lse_out != nullptr && h == 0 && q_row < Lq) lse_out[(int64_t)bh * lse_ld + q_row] = __builtin_amdgcn_logf(l_tot) + m_run * c;
#endif
    const float inv = 1.0f / l_tot;
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
// Attention BACKWARD (the autograd of F.scaled_dot_product_attention, src/UniGenUtils.py:601) on the forward kernel's
// tiling. This file holds the kernels the product dispatches: attn_bwd_kernel in its two query-owning modes (below), the fused dK / dV kernel
// attn_bwd_dkv_kernel, the pair-scheme dQ kernel attn_bwd_dq_kernel and attn_delta_kernel. In attn_bwd_kernel a workgroup OWNS 256 queries (each
// wave 32, their fragments in registers as the B operand, the query index on the LANE) and STREAMS 64-key tiles through the forward's swizzled
// LDS image (row reads for the score-like products, transposed reads for the accumulating product):
//   LSE : owns queries,  streams K       : S^T = K Q^T                         -> lse2[q] = log2 sum_k 2^(c S)          (lane-local statistics)
//   DQ  : owns queries,  streams K, V    : S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta)  -> dQ^T += K^T dS^T, x scale at the end
// with P = 2^(c S - lse2[q]), c = scale log2(e), delta[q] = sum_d dO[q][d] O[q][d]. The 32x32 accumulator of a score-like product has the
// streamed index on its rows and the owned index on its lanes, so its registers, packed to bf16, ARE the B operand of the accumulating
// product (the forward's P^T trick); lse / delta are per lane. The kernel was cut from a template of four modes and two staging forms: its
// key-owning modes DK and DV (they stream Q, dO and the queries' statistics; the fused kernel below replaced them) and register staging of the
// streamed tiles (HBM -> registers -> LDS instead of LDS-DMA) are the frozen copy attn_bwd_var_kernel in tools/probe/csrc/attn_bwd_variants.hip,
// probe library only (UG_ATTN_BWD_FUSE_DKV=0, UG_ATTN_BWD_DMA=0). S is recomputed per kernel - still ~4x less time than moving fp32 score
// matrices through HBM. Streamed tiles reach LDS by LDS-DMA one tile ahead; at dh 128 the LDS reads of every matrix phase are
// software-pipelined by hand. Measured (tools/attn_bwd_ab.py, profiles/r02f_attn_bwd.log): 501 -> 595 TFLOP/s of the algorithmic
// 10 B H Lq Lkv dh at dh 128 (4608^2), 395-420 -> 511-551 at dh 64.
// Tried and removed (commit "Attention backward: hand-pipelined LDS reads ...", same log): an X|Y staggered variant as in the forward (wave
// groups one segment apart, S of the whole tile and Z crossing the barriers in registers, three LDS-DMA buffers). Same bits, but at dh 128 it
// needs ~300 registers (hipcc spilled 100: 211 TFLOP/s) and at dh 64 it measured 431-465 against the lock-step kernel's 453-492 of that day:
// stamps showed each group's segment stretching by 450-900 cycles beside its partner's although a VALU-only and an MFMA-only wave co-execute
// perfectly in isolation (tools/probe/coexec*.hip) - unexplained, left for a later round. Starting waves 4-7 one matrix phase late per tile
// inside the lock-step kernel: +3 % / -6 % (dh 128 / 64) before the pipelining, -3 % after it.

// =====================================================================================================================
// What the three streaming kernels below share. A streamed tile image is NI runs of 1 KiB (RPI rows each); wave w owns runs w * NIW .. + NIW - 1 of
// both streamed tiles and issues their LDS-DMAs itself - no staging registers, no ds_write. The swizzle is applied on the source side as in the forward.
template <int DH> constexpr int BWD_NIW = KVB * 2 * DH / 1024 / 8;
// per-lane byte offsets of a wave's runs inside a whole tile of each of the two streamed operands (row strides rs1, rs2)
template <int DH>
__device__ __forceinline__ void bwd_dma_offsets(int wave, int lane, int64_t rs1, int64_t rs2, unsigned (&d1o)[BWD_NIW<DH>], unsigned (&d2o)[BWD_NIW<DH>]) {
    constexpr int RB = 2 * DH, NCH = DH / 8, RPI = 1024 / RB, NIW = BWD_NIW<DH>;
#pragma unroll
    for (int u = 0; u < NIW; ++u) {
        const int row = (wave * NIW + u) * RPI + lane / NCH;
        const int ch = (lane % NCH) ^ row_swz<DH>(row);
        d1o[u] = (unsigned)(row * (int)rs1 + ch * 8) * 2u;
        d2o[u] = (unsigned)(row * (int)rs2 + ch * 8) * 2u;
    }
}
// this wave's share of the tile of rows row0 .. row0 + 63 of `base` (L rows) -> LDS at dst
template <int DH>
__device__ __forceinline__ void bwd_dma_stream(const bf16_t* base, int64_t rs, const unsigned (&off)[BWD_NIW<DH>], int row0, int L, int wave, int lane, unsigned dst) {
    constexpr int RB = 2 * DH, NCH = DH / 8, RPI = 1024 / RB, NIW = BWD_NIW<DH>;
    if (row0 + KVB <= L) {
        const void* tb = uniform_ptr(base + (int64_t)row0 * rs);
#pragma unroll
        for (int u = 0; u < NIW; ++u) glds16_off(tb, off[u], dst + u * 1024);
    } else {                                           // ragged last tile: rows past the end re-read the last row (masked by the caller)
        int lane_r = lane;
        asm volatile("" : "+v"(lane_r));
#pragma unroll
        for (int u = 0; u < NIW; ++u) {
            const int row = (wave * NIW + u) * RPI + lane_r / NCH;
            const int ch = (lane_r % NCH) ^ row_swz<DH>(row);
            int sr = row0 + row; if (sr > L - 1) sr = L - 1;
            glds16_ptr(base + (int64_t)sr * rs + ch * 8, dst + u * 1024);
        }
    }
}
// per-lane LDS read offsets: every swizzled offset is BASE ^ constant, re-derived from opaque copies of three bases (no per-fragment registers)
template <int DH>
__device__ __forceinline__ void bwd_read_bases(int lane, int& k_base, int& tlo_base, int& thi_base) {
    constexpr int RB = 2 * DH;
    const int r = lane & 31, h = lane >> 5;
    k_base = RB * r + 16 * (h ^ row_swz<DH>(r));                           // row fragment s of 32-row block kb: kb * 32 * RB + (k_base ^ 32 s)
    const int i16 = lane & 15, g16 = lane >> 4;
    const int t_key = 4 * h + (i16 >> 2), t_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1), t_b8 = 8 * (i16 & 1);
    tlo_base = RB * t_key + 16 * (t_lowch ^ row_swz<DH>(t_key)) + t_b8;              // d-block db, k-step ks: ks * 16 * RB + (base ^ 64 db)
    thi_base = RB * (t_key + 8) + 16 * (t_lowch ^ row_swz<DH>(t_key + 8)) + t_b8;
}
template <int NDB>
__device__ __forceinline__ void bwd_zero(f32x16 (&acc)[NDB]) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[db][i] = 0.f;
}
// one gradient row, acc^T[d][own row] x es -> bf16: lane (r, h) holds columns 32 db + 8 g4 + 4 h .. + 3 of its row (Orow: the row's head slice)
template <int NDB>
__device__ __forceinline__ void bwd_store_row(bf16_t* Orow, const f32x16 (&acc)[NDB], float es, int h) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            u32x2 w;
            w.x = pack2bf(acc[db][4 * g4 + 0] * es, acc[db][4 * g4 + 1] * es);
            w.y = pack2bf(acc[db][4 * g4 + 2] * es, acc[db][4 * g4 + 3] * es);
            *(u32x2*)(Orow + 32 * db + 8 * g4 + 4 * h) = w;
        }
}

template <int DH, bool DQ>       // head dim 128 | 64; DQ: the dQ mode (own2 = dO, st2 = V, out = dQ), else the LSE mode (those three unused)
__global__ __launch_bounds__(512, 2) void attn_bwd_kernel(
    const bf16_t* __restrict__ own1, int64_t o1_rs, int64_t o1_bs, const bf16_t* __restrict__ own2, int64_t o2_rs, int64_t o2_bs,
    const bf16_t* __restrict__ st1, int64_t s1_rs, int64_t s1_bs, const bf16_t* __restrict__ st2, int64_t s2_rs, int64_t s2_bs,
    float* __restrict__ lse2, const float* __restrict__ delta, int64_t stat_ld /* queries per (b, h) row of lse2 / delta */,
    bf16_t* __restrict__ out, int64_t out_rs, int64_t out_bs, int heads, int Lown, int Lst, int nOwn, float c, float scale) {
    constexpr int RB = 2 * DH, TILE = KVB * RB, QS = DH / 16, NDB = DH / 32, NIW = BWD_NIW<DH>;
    constexpr int BUFSZ = 2 * TILE + 512;      // the 512 bytes were the statistics slot (lse2[64] | delta[64]) of the streamed queries of the DK / DV modes: unused here, kept for the addresses
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][tile of st1 | tile of st2 | 512 unused bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int ot = blockIdx.x % nOwn, bh = blockIdx.x / nOwn;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* O1 = own1 + (int64_t)b * o1_bs + head * DH;
    const bf16_t* O2 = DQ ? own2 + (int64_t)b * o2_bs + head * DH : nullptr;
    const bf16_t* S1 = st1 + (int64_t)b * s1_bs + head * DH;
    const bf16_t* S2 = DQ ? st2 + (int64_t)b * s2_bs + head * DH : nullptr;
    const int own_row = ot * 256 + wave * 32 + r;
    const int own_ld = own_row < Lown ? own_row : Lown - 1;
    bf16x8 f1[QS], f2[DQ ? QS : 1];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        f1[s] = *(const bf16x8*)(O1 + (int64_t)own_ld * o1_rs + 16 * s + 8 * h);
        if constexpr (DQ) f2[s] = *(const bf16x8*)(O2 + (int64_t)own_ld * o2_rs + 16 * s + 8 * h);
    }
    const float* stat_l = lse2 + (int64_t)bh * stat_ld;
    const float* stat_d = DQ ? delta + (int64_t)bh * stat_ld : nullptr;
    float my_lse = 0.f, my_delta = 0.f;
    if constexpr (DQ) { my_lse = stat_l[own_ld]; my_delta = stat_d[own_ld]; }
    // LDS-DMA staging: the DMAs of tile t + 1 are issued at the top of tile t and waited for (vmcnt(0)) ahead of the barrier that ends it
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    unsigned d1o[NIW], d2o[NIW];
    bwd_dma_offsets<DH>(wv, lane, s1_rs, s2_rs, d1o, d2o);
    auto stage_load = [&](int row0, int buf) {
        const unsigned l0 = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + buf * BUFSZ + wv * NIW * 1024;
        bwd_dma_stream<DH>(S1, s1_rs, d1o, row0, Lst, wv, lane, l0);
        if constexpr (DQ) bwd_dma_stream<DH>(S2, s2_rs, d2o, row0, Lst, wv, lane, l0 + TILE);
    };
    auto stage_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    // bwd_read_bases, spelled out: through the helper hipcc gives the LSE mode 112 / 110 registers (dh 128 / 64) instead of 97 / 82
    const int k_base = RB * r + 16 * (h ^ row_swz<DH>(r));
    const int i16 = lane & 15, g16 = lane >> 4;
    const int t_key = 4 * h + (i16 >> 2), t_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1), t_b8 = 8 * (i16 & 1);
    const int tlo_base = RB * t_key + 16 * (t_lowch ^ row_swz<DH>(t_key)) + t_b8;
    const int thi_base = RB * (t_key + 8) + 16 * (t_lowch ^ row_swz<DH>(t_key + 8)) + t_b8;
    // dh 128: the LDS reads of each matrix phase are software-pipelined by hand - the fragments of step j + PD are requested before the MFMAs
    // of step j (left to hipcc every MFMA pair sits right behind its own ds_read and s_waitcnt): 527 -> 548 TFLOP/s. At dh 64 (half the MFMAs
    // per read burst) the same pipeline measured 6 % slower than hipcc's order, which stays.
    constexpr bool PIPE = DH == 128;
    constexpr int PDS = 3, PDA = 1;
    f32x16 acc[DQ ? NDB : 1];
    if constexpr (DQ) bwd_zero(acc);
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (Lst + KVB - 1) / KVB;
    stage_load(0, 0);
    stage_wait();
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage_load((t + 1) * KVB, cur ^ 1);
        const unsigned char* B1 = smem + cur * BUFSZ;
        const unsigned char* B2 = B1 + TILE;
        bf16x8 zf[2][2];
        float tmax = -INFINITY;
        f32x16 x1k[DQ ? 1 : 2];
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
                    if constexpr (DQ) ab[s5 % (PDS + 1)][1] = *(const bf16x8*)(B2 + kb * 32 * RB + (kb0 ^ (32 * s5)));
                };
#pragma unroll
                for (int j = 0; j < PDS && j < QS; ++j) rd(j);
#pragma unroll
                for (int s5 = 0; s5 < QS; ++s5) {
                    if (s5 + PDS < QS) rd(s5 + PDS);
                    __builtin_amdgcn_sched_barrier(0);
                    x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][0], f1[s5], x1, 0, 0, 0);
                    if constexpr (DQ) x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][1], f2[s5], x2, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int s5 = 0; s5 < QS; ++s5) {
                    const bf16x8 a1 = *(const bf16x8*)(B1 + kb * 32 * RB + (k_base ^ (32 * s5)));
                    x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, f1[s5], x1, 0, 0, 0);
                    if constexpr (DQ) {
                        const bf16x8 a2 = *(const bf16x8*)(B2 + kb * 32 * RB + (k_base ^ (32 * s5)));
                        x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, f2[s5], x2, 0, 0, 0);
                    }
                }
            }
            // streamed row of accumulator element i
            const int srow0 = t * KVB + kb * 32 + 4 * h;
            if constexpr (!DQ) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (srow0 + (i & 3) + 8 * (i >> 2) >= Lst) x1[i] = -INFINITY;
                    tmax = fmaxf(tmax, x1[i]);
                }
                x1k[kb] = x1;
            } else {
                float z[16];
                // z = P (dP - delta) (the softmax scale is applied once, to the accumulator, in the epilogue); keys past the end exist only in the
                // ragged last tile
                if (t * KVB + KVB <= Lst) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -my_lse));
                        z[i] = p * (x2[i] - my_delta);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const bool valid = srow0 + (i & 3) + 8 * (i >> 2) < Lst;
                        const float p = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -my_lse));
                        const float v = p * (x2[i] - my_delta);
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
        if constexpr (!DQ) {
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
            // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
            const unsigned char* Tb = B1;
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
        if (t + 1 < ntiles) stage_wait();
        __syncthreads();
    }
    if constexpr (!DQ) {
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        if (own_row < Lown && h == 0) lse2[(int64_t)bh * stat_ld + own_row] = __builtin_amdgcn_logf(l_tot) + m_run * c;     // v_log_f32 = log2
    } else if (own_row < Lown) {
        bwd_store_row(out + (int64_t)b * out_bs + (int64_t)own_row * out_rs + head * DH, acc, scale, h);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused dK / dV (round 3): the key-owning DK and DV modes (tools/probe/csrc/attn_bwd_variants.hip) both recompute S = Q K^T over the same (keys, queries) - 8 product units per attention
// against the minimum of 5. Fusing them on the 256-key ownership needs 128 accumulator + 64 owned-operand registers beside the score tiles:
// over the 256 a two-wave-per-SIMD kernel has. This kernel splits the work of a 32-key block between the TWO waves of a pair instead:
//   a workgroup owns 128 keys; waves p and p + 4 (p = 0..3) own the same 32 keys (K and V fragments in registers, key on the lane);
//   score phase : wave half h = wave >> 2 takes the 32 streamed queries kb = h of the 64-row tile: S, dP -> P and dS = P (dP - delta), packed to bf16 -
//                 the B operands of the accumulating products. Half 0 accumulates dK, half 1 accumulates dV: a wave keeps the operand of ITS gradient
//                 and publishes the other one lane-linear in LDS (2 KiB per wave, double-buffered);
//   accumulation: after ONE barrier per tile a wave has its partner's operand too and accumulates its gradient over all 64 queries, all head dims:
//                 dK^T += Q^T dS (half 0) or dV^T += dO^T P (half 1) (transposed reads of the streamed tile, fragments one k-step ahead).
// Per 32 keys x 64 queries: 16 + 16 (scores) + 16 + 16 (accumulation) MFMAs = the five product units, no duplicated product, 64 accumulator
// registers per wave. The streamed tiles (image and statistics of the DK mode) sit in a ring of THREE stages: tile t + 2 is requested right after the
// barrier of tile t and waited for ahead of the barrier of tile t + 1, so that single barrier certifies the exchange, the landing and the free stage.
// Measured (tools/attn_bwd_ab.py, profiles/r03y_attn_bwd_fuse_*.log; whole backward incl. the DQ mode): dh 128 605 -> 711 TFLOP/s of the algorithmic
// 10 B H Lq Lkv dh at 4608^2 (+17.6 %; 8704^2 +17 %, 1000^2 +8 %), dh 64 531 -> 578 / 574 -> 612; same bits as the two modes (same products, same order).
// Steps on the way: the first form (both gradients per wave on half the head dims, 4 KiB exchange, two barriers) +0.8 %; its transposed reads one step
// ahead +2 %; the per-element row masks out of the whole-tile path (32 v_cndmask per tile: the score phase is VALU-bound) +13.6 %; this form +17.6 %.
// Tried and dropped: the dV waves scoring tile t + 1 BEFORE accumulating tile t while the dK waves do the opposite (the two waves of a SIMD then
// alternate VALU-heavy and MFMA-only phases): 37 spilled registers at dh 128 (421 TFLOP/s), and 522 vs 578 at dh 64 without a single spill.
// Also dropped: scalar branches instead of the wave-uniform `half ? a : b` selects of the operands (24 v_cndmask per tile): the duplicated
// accumulation block costs 46 spilled registers at dh 128 (476 TFLOP/s).
// ---------------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(512, 2) void attn_bwd_dkv_kernel(
    const bf16_t* __restrict__ kk, int64_t k_rs, int64_t k_bs, const bf16_t* __restrict__ vv, int64_t v_rs, int64_t v_bs,
    const bf16_t* __restrict__ qq, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ dd, int64_t d_rs, int64_t d_bs,
    const float* __restrict__ lse2, const float* __restrict__ delta, int64_t stat_ld, bf16_t* __restrict__ dk, int64_t dk_rs, int64_t dk_bs,
    bf16_t* __restrict__ dv, int64_t dv_rs, int64_t dv_bs, int heads, int Lkv, int Lq, int nOwn, float c, float scale) {
    constexpr int RB = 2 * DH, TILE = KVB * RB, QS = DH / 16, NDB = DH / 32, NIW = BWD_NIW<DH>;
    constexpr int BUFSZ = 2 * TILE + 512, NSTG = 3, ZOFF = NSTG * BUFSZ;   // [3][Q tile | dO tile | lse2[64] | delta[64]] then [2][8 waves] x 2 KiB of exchanged operands
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = wave & 3, half = wave >> 2;           // half 0: queries kb = 0 of a tile, accumulates dK; half 1: queries kb = 1, accumulates dV
    const int r = lane & 31, h = lane >> 5;
    const int ot = blockIdx.x % nOwn, bh = blockIdx.x / nOwn;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* Kb = kk + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = vv + (int64_t)b * v_bs + head * DH;
    const bf16_t* Qb = qq + (int64_t)b * q_bs + head * DH;
    const bf16_t* Db = dd + (int64_t)b * d_bs + head * DH;
    const int own_row = ot * 128 + pair * 32 + r;
    const int own_ld = own_row < Lkv ? own_row : Lkv - 1;
    bf16x8 fk[QS], fv[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        fk[s] = *(const bf16x8*)(Kb + (int64_t)own_ld * k_rs + 16 * s + 8 * h);
        fv[s] = *(const bf16x8*)(Vb + (int64_t)own_ld * v_rs + 16 * s + 8 * h);
    }
    const float* stat_l = lse2 + (int64_t)bh * stat_ld;
    const float* stat_d = delta + (int64_t)bh * stat_ld;
    // LDS-DMA staging as in attn_bwd_kernel (wave w owns runs w * NIW .. + NIW - 1 of both streamed tiles), but a ring of three stages: tile t + 2 is
    // requested right after the barrier of tile t (its stage was last read by the accumulation of tile t - 1, which every wave has left by then) and is
    // waited for ahead of the barrier of tile t + 1 - one barrier per tile certifies both the exchange and the landing.
    unsigned d1o[NIW], d2o[NIW];
    bwd_dma_offsets<DH>(wave, lane, q_rs, d_rs, d1o, d2o);
    auto stage_load = [&](int row0, int stg) __attribute__((always_inline)) {
        const unsigned lb = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + stg * BUFSZ, l0 = lb + wave * NIW * 1024;
        bwd_dma_stream<DH>(Qb, q_rs, d1o, row0, Lq, wave, lane, l0);
        bwd_dma_stream<DH>(Db, d_rs, d2o, row0, Lq, wave, lane, l0 + TILE);
        if (wave == 0) glds4_ptr(stat_l + row0 + lane, lb + 2 * TILE);          // the tile's 64 lse2 / delta values (rows padded to a multiple of 64, zeros)
        if (wave == 1) glds4_ptr(stat_d + row0 + lane, lb + 2 * TILE + 256);
    };
    int k_base, tlo_base, thi_base;
    bwd_read_bases<DH>(lane, k_base, tlo_base, thi_base);
    f32x16 acc[NDB];                                   // dK^T (half 0) or dV^T (half 1): [d][own key]
    bwd_zero(acc);
    const int ntiles = (Lq + KVB - 1) / KVB;
    stage_load(0, 0);
    if (ntiles > 1) stage_load(KVB, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int stg = 0;                                       // stage of tile t
    for (int t = 0; t < ntiles; ++t) {
        const unsigned char* B1 = smem + stg * BUFSZ;
        const unsigned char* B2 = B1 + TILE;
        unsigned char* const zmine = smem + ZOFF + (t & 1) * 16384 + wave * 2048 + lane * 16;
        const unsigned char* const zpart = smem + ZOFF + (t & 1) * 16384 + (wave ^ 4) * 2048 + lane * 16;
        // ---- score phase: the 32 streamed queries kb = half; this wave keeps the operand of ITS gradient and publishes the other one ----
        bf16x8 zown[2];
        {
            f32x16 x1, x2;
#pragma unroll
            for (int i = 0; i < 16; ++i) { x1[i] = 0.f; x2[i] = 0.f; }
            int kb0 = k_base;
            asm volatile("" : "+v"(kb0));
            constexpr int PDS = 2;
            bf16x8 ab[PDS + 1][2];
            auto rd = [&](int s5) __attribute__((always_inline)) {
                ab[s5 % (PDS + 1)][0] = *(const bf16x8*)(B1 + half * 32 * RB + (kb0 ^ (32 * s5)));
                ab[s5 % (PDS + 1)][1] = *(const bf16x8*)(B2 + half * 32 * RB + (kb0 ^ (32 * s5)));
            };
#pragma unroll
            for (int j = 0; j < PDS && j < QS; ++j) rd(j);
#pragma unroll
            for (int s5 = 0; s5 < QS; ++s5) {
                if (s5 + PDS < QS) rd(s5 + PDS);
                __builtin_amdgcn_sched_barrier(0);
                x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][0], fk[s5], x1, 0, 0, 0);
                x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][1], fv[s5], x2, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            const float* st = (const float*)(B1 + 2 * TILE);
            float sl[16], sd[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 a = *(const f32x4*)(st + half * 32 + 4 * h + 8 * g);
                const f32x4 d4 = *(const f32x4*)(st + 64 + half * 32 + 4 * h + 8 * g);
                sl[4 * g] = a[0]; sl[4 * g + 1] = a[1]; sl[4 * g + 2] = a[2]; sl[4 * g + 3] = a[3];
                sd[4 * g] = d4[0]; sd[4 * g + 1] = d4[1]; sd[4 * g + 2] = d4[2]; sd[4 * g + 3] = d4[3];
            }
            float pk[16], pv[16];
            if (t * KVB + KVB <= Lq) {                 // rows past the end exist only in the ragged last tile
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    pv[i] = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -sl[i]));
                    pk[i] = pv[i] * (x2[i] - sd[i]);
                }
            } else {
                const int srow0 = t * KVB + half * 32 + 4 * h;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -sl[i]));
                    const bool valid = srow0 + (i & 3) + 8 * (i >> 2) < Lq;
                    pv[i] = valid ? p : 0.f;
                    pk[i] = valid ? p * (x2[i] - sd[i]) : 0.f;
                }
            }
            bf16x8 zk[2], zv[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                u32x4 w;
                w.x = pack2bf(pk[8 * s2 + 0], pk[8 * s2 + 1]); w.y = pack2bf(pk[8 * s2 + 2], pk[8 * s2 + 3]);
                w.z = pack2bf(pk[8 * s2 + 4], pk[8 * s2 + 5]); w.w = pack2bf(pk[8 * s2 + 6], pk[8 * s2 + 7]);
                zk[s2] = __builtin_bit_cast(bf16x8, w);
                w.x = pack2bf(pv[8 * s2 + 0], pv[8 * s2 + 1]); w.y = pack2bf(pv[8 * s2 + 2], pv[8 * s2 + 3]);
                w.z = pack2bf(pv[8 * s2 + 4], pv[8 * s2 + 5]); w.w = pack2bf(pv[8 * s2 + 6], pv[8 * s2 + 7]);
                zv[s2] = __builtin_bit_cast(bf16x8, w);
            }
            zown[0] = half ? zv[0] : zk[0]; zown[1] = half ? zv[1] : zk[1];        // wave-uniform selects
            *(bf16x8*)(zmine) = half ? zk[0] : zv[0];
            *(bf16x8*)(zmine + 1024) = half ? zk[1] : zv[1];
        }
        // ---- accumulation over all 64 queries: dK^T += Q^T dS (half 0) or dV^T += dO^T P (half 1); the transposed fragments of k-step ks + 1 are
        //      requested before the MFMAs of step ks, those of step 0 ahead of the barrier (they do not depend on the partner) ----
        {
            const unsigned char* Tb = half ? B2 : B1;
            int lo0 = tlo_base, hi0 = thi_base;
            asm volatile("" : "+v"(lo0), "+v"(hi0));
            bf16x8 tf[2][NDB];
            auto rdT = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
                for (int db = 0; db < NDB; ++db) tf[ks & 1][db] = tr_read_pair(Tb + ks * 16 * RB + (lo0 ^ (64 * db)), Tb + ks * 16 * RB + (hi0 ^ (64 * db)));
            };
            rdT(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's share of tile t + 1 has landed (requested a whole tile ago)
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                           // the partner's operand is in LDS; tile t + 1 is complete; nobody reads the stage of tile t - 1 any more
            if (t + 2 < ntiles) stage_load((t + 2) * KVB, stg == 0 ? 2 : stg - 1);
            const bf16x8 zp0 = *(const bf16x8*)(zpart), zp1 = *(const bf16x8*)(zpart + 1024);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bool mine = (ks >> 1) == half;               // wave-uniform
                const bf16x8 bz = mine ? zown[ks & 1] : ((ks & 1) ? zp1 : zp0);
                if (ks + 1 < 4) rdT(ks + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int db = 0; db < NDB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[ks & 1][db], bz, acc[db], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        stg = stg == 2 ? 0 : stg + 1;
    }
    if (own_row < Lkv) {
        bf16_t* Orow = (half ? dv + (int64_t)b * dv_bs + (int64_t)own_row * dv_rs : dk + (int64_t)b * dk_bs + (int64_t)own_row * dk_rs) + head * DH;
        bwd_store_row(Orow, acc, half ? 1.f : scale, h);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dQ on the pair scheme (round 3): the DQ mode above owns 256 queries per workgroup - 18 x 24 x B = 864 workgroups at L = 4608, B = 2: 3.4 rounds of
// the 256 CUs, the last one 37 % full. Here a workgroup owns 128 queries; waves p and p + 4 own the same 32 (Q and dO fragments in registers, query on
// the lane), wave half h takes the 32 streamed KEYS kb = h of each 64-key tile: S^T, dP^T -> dS^T -> dQ^T += K^T dS^T over its own keys only - no
// exchange per tile, 24 MFMAs per wave and tile - and the two partial sums of a pair meet once, in LDS, after the last tile. Twice the workgroups
// (6.75 rounds: 4 % idle in the last instead of 16 %), half the accumulator-side registers, the three-stage stream ring and one barrier per tile of
// the fused dK / dV kernel. The sum over keys associates differently from the DQ mode (two partial sums): same value to fp32 rounding, not the same bits.
// ---------------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(512, 2) void attn_bwd_dq_kernel(
    const bf16_t* __restrict__ qq, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ dd, int64_t d_rs, int64_t d_bs,
    const bf16_t* __restrict__ kk, int64_t k_rs, int64_t k_bs, const bf16_t* __restrict__ vv, int64_t v_rs, int64_t v_bs,
    const float* __restrict__ lse2, const float* __restrict__ delta, int64_t stat_ld, bf16_t* __restrict__ dq, int64_t dq_rs, int64_t dq_bs,
    int heads, int Lq, int Lkv, int nOwn, float c, float scale) {
    constexpr int RB = 2 * DH, TILE = KVB * RB, QS = DH / 16, NDB = DH / 32, NIW = BWD_NIW<DH>;
    constexpr int BUFSZ = 2 * TILE;                    // [3][K tile | V tile]
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = wave & 3, half = wave >> 2;
    const int r = lane & 31, h = lane >> 5;
    const int ot = blockIdx.x % nOwn, bh = blockIdx.x / nOwn;
    const int head = bh % heads, b = bh / heads;
    const bf16_t* Qb = qq + (int64_t)b * q_bs + head * DH;
    const bf16_t* Db = dd + (int64_t)b * d_bs + head * DH;
    const bf16_t* Kb = kk + (int64_t)b * k_bs + head * DH;
    const bf16_t* Vb = vv + (int64_t)b * v_bs + head * DH;
    const int own_row = ot * 128 + pair * 32 + r;
    const int own_ld = own_row < Lq ? own_row : Lq - 1;
    bf16x8 fq[QS], fo[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        fq[s] = *(const bf16x8*)(Qb + (int64_t)own_ld * q_rs + 16 * s + 8 * h);
        fo[s] = *(const bf16x8*)(Db + (int64_t)own_ld * d_rs + 16 * s + 8 * h);
    }
    const float my_lse = lse2[(int64_t)bh * stat_ld + own_ld], my_delta = delta[(int64_t)bh * stat_ld + own_ld];
    unsigned d1o[NIW], d2o[NIW];
    bwd_dma_offsets<DH>(wave, lane, k_rs, v_rs, d1o, d2o);
    auto stage_load = [&](int row0, int stg) __attribute__((always_inline)) {
        const unsigned l0 = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + stg * BUFSZ + wave * NIW * 1024;
        bwd_dma_stream<DH>(Kb, k_rs, d1o, row0, Lkv, wave, lane, l0);
        bwd_dma_stream<DH>(Vb, v_rs, d2o, row0, Lkv, wave, lane, l0 + TILE);
    };
    int k_base, tlo_base, thi_base;
    bwd_read_bases<DH>(lane, k_base, tlo_base, thi_base);
    f32x16 acc[NDB];                                   // partial dQ^T [d][own query] over this wave's key blocks
    bwd_zero(acc);
    const int ntiles = (Lkv + KVB - 1) / KVB;
    stage_load(0, 0);
    if (ntiles > 1) stage_load(KVB, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int stg = 0;
    for (int t = 0; t < ntiles; ++t) {
        const unsigned char* B1 = smem + stg * BUFSZ;
        const unsigned char* B2 = B1 + TILE;
        if (t + 2 < ntiles) stage_load((t + 2) * KVB, stg == 0 ? 2 : stg - 1);      // the stage of tile t - 1: every wave left it before the barrier behind us
        f32x16 x1, x2;
#pragma unroll
        for (int i = 0; i < 16; ++i) { x1[i] = 0.f; x2[i] = 0.f; }
        {
            int kb0 = k_base;
            asm volatile("" : "+v"(kb0));
            constexpr int PDS = 3;
            bf16x8 ab[PDS + 1][2];
            auto rd = [&](int s5) __attribute__((always_inline)) {
                ab[s5 % (PDS + 1)][0] = *(const bf16x8*)(B1 + half * 32 * RB + (kb0 ^ (32 * s5)));
                ab[s5 % (PDS + 1)][1] = *(const bf16x8*)(B2 + half * 32 * RB + (kb0 ^ (32 * s5)));
            };
#pragma unroll
            for (int j = 0; j < PDS && j < QS; ++j) rd(j);
#pragma unroll
            for (int s5 = 0; s5 < QS; ++s5) {
                if (s5 + PDS < QS) rd(s5 + PDS);
                __builtin_amdgcn_sched_barrier(0);
                x1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][0], fq[s5], x1, 0, 0, 0);
                x2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab[s5 % (PDS + 1)][1], fo[s5], x2, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the transposed K fragments of this wave's two k-steps (keys 32 half + 16 ks ..): requested now, used after the softmax arithmetic
        bf16x8 tf[2][NDB];
        {
            int lo0 = tlo_base, hi0 = thi_base;
            asm volatile("" : "+v"(lo0), "+v"(hi0));
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int db = 0; db < NDB; ++db)
                    tf[ks][db] = tr_read_pair(B1 + (2 * half + ks) * 16 * RB + (lo0 ^ (64 * db)), B1 + (2 * half + ks) * 16 * RB + (hi0 ^ (64 * db)));
        }
        float z[16];
        if (t * KVB + KVB <= Lkv) {                    // keys past the end exist only in the ragged last tile
#pragma unroll
            for (int i = 0; i < 16; ++i) z[i] = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -my_lse)) * (x2[i] - my_delta);
        } else {
            const int srow0 = t * KVB + half * 32 + 4 * h;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = __builtin_amdgcn_exp2f(fmaf(x1[i], c, -my_lse)) * (x2[i] - my_delta);
                z[i] = srow0 + (i & 3) + 8 * (i >> 2) < Lkv ? v : 0.f;
            }
        }
        bf16x8 zf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            u32x4 w;
            w.x = pack2bf(z[8 * s2 + 0], z[8 * s2 + 1]); w.y = pack2bf(z[8 * s2 + 2], z[8 * s2 + 3]);
            w.z = pack2bf(z[8 * s2 + 4], z[8 * s2 + 5]); w.w = pack2bf(z[8 * s2 + 6], z[8 * s2 + 7]);
            zf[s2] = __builtin_bit_cast(bf16x8, w);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int db = 0; db < NDB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[ks][db], zf[ks], acc[db], 0, 0, 0);
        // this wave's share of tile t + 1 (requested two tiles ago) has landed; the requests of tile t + 2, issued above, stay in flight
        if (t + 2 < ntiles) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NIW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        stg = stg == 2 ? 0 : stg + 1;
    }
    // the pair's two partial sums: half 1 parks its accumulators in LDS (lane-linear, NDB x 4 KiB per wave; the stream stages are free now), half 0 adds them
    float* park = (float*)smem + pair * (NDB * 4 * 256) + lane * 4;     // 4 x NDB x 4 KiB <= the three stream stages at either head width
    if (half == 1) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(f32x4*)(park + (db * 4 + g4) * 256) = (f32x4){acc[db][4 * g4 + 0], acc[db][4 * g4 + 1], acc[db][4 * g4 + 2], acc[db][4 * g4 + 3]};
    }
    __syncthreads();
    if (half == 0 && own_row < Lq) {
        bf16_t* Orow = dq + (int64_t)b * dq_bs + (int64_t)own_row * dq_rs + head * DH;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 o = *(const f32x4*)(park + (db * 4 + g4) * 256);
                u32x2 w;
                w.x = pack2bf((acc[db][4 * g4 + 0] + o[0]) * scale, (acc[db][4 * g4 + 1] + o[1]) * scale);
                w.y = pack2bf((acc[db][4 * g4 + 2] + o[2]) * scale, (acc[db][4 * g4 + 3] + o[3]) * scale);
                *(u32x2*)(Orow + 32 * db + 8 * g4 + 4 * h) = w;
            }
    }
}

// delta[bh][q] = sum_d dO[b][q][h*DH + d] * O[b][q][h*DH + d]: DH / 8 lanes per (b, q, h), 16-byte loads, the sum over those lanes by xor shuffles
template <int DH>
__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs, const bf16_t* __restrict__ dout, int64_t d_rs,
                                                         int64_t d_bs, float* __restrict__ delta, int64_t stat_ld, int64_t total, int heads, int Lq) {
    constexpr int LPV = DH / 8, VPW = 64 / LPV;
    const int lane = threadIdx.x & 63, sub = lane % LPV;
    const int64_t id = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * VPW + lane / LPV;
    const int64_t idc = id < total ? id : total - 1;
    const int hd = (int)(idc % heads); const int64_t t = idc / heads; const int q = (int)(t % Lq); const int64_t b = t / Lq;
    const bf16x8 a = *(const bf16x8*)(o + b * o_bs + (int64_t)q * o_rs + hd * DH + 8 * sub);
    const bf16x8 g = *(const bf16x8*)(dout + b * d_bs + (int64_t)q * d_rs + hd * DH + 8 * sub);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += bf2f((bf16_t)a[k]) * bf2f((bf16_t)g[k]);
#pragma unroll
    for (int m = 1; m < LPV; m <<= 1) acc += __shfl_xor(acc, m, 64);
    if (sub == 0 && id < total) delta[(b * heads + hd) * stat_ld + q] = acc;
}

}  // namespace

static int flash_attn_fwd_impl(const char* who, const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k,
                               int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
                               int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                               int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                               float* lse_out, int64_t lse_ld, ug_stream_t stream) {
    if (batches == 0 || Lq == 0) return UG_OK;
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && Lq > 0 && Lkv > 0, UG_ERR_BAD_SHAPE, "%s: bad arguments", who);
    UG_REQUIRE(dh == 128 || dh == 64, UG_ERR_UNSUPPORTED, "%s: head dim %d not in {64, 128}", who, dh);
    UG_REQUIRE(Lq < (1 << 30) && Lkv < (1 << 30), UG_ERR_UNSUPPORTED, "%s: sequence too long", who);
    // the row-stride bound: the LDS-DMAs of K and V form 32-bit byte offsets over a 64-row tile from the row stride cut to int (63 rs + 120 < 2^31
    // is what they can hold); one rule for every row stride of the family, the one of ug_flash_attn_fwd_wide
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, true}, {"k", UG_VIEW(k), 8, 16, true}, {"v", UG_VIEW(v), 8, 16, true}, {"o", UG_VIEW(o), 4, 8, true}};
    if (const int rc = ug_check_views(who, views)) return rc;
#ifdef UG_PROBE_BUILD     // probe library: every forward form, the UG_ATTN_* environment switches select (tools/probe/csrc/attn_fwd_variants.hip)
    return ug_attn_fwd_variants(q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                                o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, lse_out, lse_ld, stream);
#endif
    // One kernel per head width - the X|Y stagger with LDS-DMA staging and 16-byte stores; what else follows from the head width is at the top of
    // flash_attn_kernel. The dispatcher only chooses the DMA form at head width 64.
    const int nQ = (int)((Lq + 255) / 256);            // 8 waves x 32 query rows per workgroup
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "%s: grid too large", who);
    const float c = softmax_scale * 1.4426950408889634f;
    // (Round 4: the same stagger on v_mfma_f32_16x16x32_bf16 - flash_attn_m16_kernel, probe library, UG_ATTN_M16=1 - measured +3.5...+4.2 % in a
    // sustained interleaved A/B at 4608^2 / 4096 x 4608 / 8192 x 8704 and -5.6 % INSIDE the cfg2 forward (1113 vs 1177 TFLOP/s, same box, same
    // library, profiles/r04h_attn_m16_in_app.log): its advantage is the higher clock the chip reaches for that shape after ~10 ms of back-to-back
    // launches; a 0.9 ms launch between GEMMs never gets there, and at equal clock its 64 MFMA issues per tile cost the partner wave's softmax more
    // issue slots than 32 do. Not shipped.)
    // Round 6 (profiles/r06_attn_variants.log): BUFD +2.3...+4.6 %, bit-identical; LSUM +1.5...+2.6 % on the cfg5 shapes by itself, +3.9...+6.3 %
    // together with BUFD; at head width 128 LSUM lost 4 % (X is its longer segment).
    // the buffer-form DMAs (BUFD) need one row stride for K and V, a multiple of 16 elements, and byte offsets of a (batch, head)'s keys below 2^31
    const bool bufd_ok = k_row_stride == v_row_stride && k_row_stride % 16 == 0 && Lkv * k_row_stride * 2 < (1ll << 31);
    const dim3 grid((unsigned)nwg), block(512);
    const size_t lds = 2 * 2 * KVB * 2 * dh + 256 * 2 * dh;        // [2][K tile | V tile] + the Q image (32 KiB + 32 KiB at head width 64, 64 + 64 at 128)
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride, (const bf16_t*)k, k_row_stride,
                           k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride, o_batch_stride, (int)heads, (int)Lq,
                           (int)Lkv, nQ, c, lse_out, lse_ld);
    };
    if (dh == 128) launch(flash_attn_kernel<128, false>);
    else if (bufd_ok) launch(flash_attn_kernel<64, true>);
    else launch(flash_attn_kernel<64, false>);
    UG_CHECK_LAUNCH(who);
    return UG_OK;
}

extern "C" int ug_flash_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k,
                                 int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
                                 int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                                 int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                                 ug_stream_t stream) {
    return flash_attn_fwd_impl(__func__, q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                               o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, nullptr, 0, stream);
}

extern "C" int ug_flash_attn_fwd_lse(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k,
                                     int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
                                     int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                                     int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                                     float* lse2, int64_t lse_ld, ug_stream_t stream) {
    UG_REQUIRE(lse2 && lse_ld >= Lq, UG_ERR_BAD_SHAPE, "ug_flash_attn_fwd_lse: lse2 [batches][heads][lse_ld >= Lq] needed");
    return flash_attn_fwd_impl(__func__, q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, v, v_row_stride, v_batch_stride, o, o_row_stride,
                               o_batch_stride, batches, heads, Lq, Lkv, dh, softmax_scale, lse2, lse_ld, stream);
}

// The three stages of the backward, in stream order: the rows' statistics (unless the forward supplied them), dQ, dK and dV. Every kernel takes
// more than 64 KiB of dynamic LDS at head width 128: bwd_launch sets the attribute that allows it once per instantiation.
template <auto KERNEL, typename... Args>
static void bwd_launch(int64_t grid, int lds, hipStream_t s, Args... args) {
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(512), lds, s, args...);
}
static int64_t bwd_grid(const ug_attn_bwd_args& a, int L, int rows) { return (int64_t)((L + rows - 1) / rows) * a.heads * a.batches; }

template <int DH>
static void bwd_launch_lse(const ug_attn_bwd_args& a) {            // lse2 from Q and K: 256 queries per workgroup
    bwd_launch<attn_bwd_kernel<DH, false>>(bwd_grid(a, a.Lq, 256), 2 * (2 * KVB * 2 * DH + 512), a.s, a.q, a.q_rs, a.q_bs, nullptr, 0, 0,
                                           a.k, a.k_rs, a.k_bs, nullptr, 0, 0, a.lse2, a.delta, a.stat_ld, nullptr, 0, 0, a.heads, a.Lq, a.Lkv, (a.Lq + 255) / 256, a.c, a.scale);
}
#ifdef UG_PROBE_BUILD
constexpr bool PAIR_DQ_64 = true;      // the probe library has the pair-scheme dQ kernel at head width 64 too (UG_ATTN_BWD_PAIR_DQ=2)
#else
constexpr bool PAIR_DQ_64 = false;     // product: pair_dq is only ever set at head width 128
#endif
template <int DH>
static void bwd_launch_dq(const ug_attn_bwd_args& a, bool pair_dq) {
    if constexpr (DH == 128 || PAIR_DQ_64) {
        if (pair_dq) {                 // 128 queries per workgroup, [3][K tile | V tile]
            bwd_launch<attn_bwd_dq_kernel<DH>>(bwd_grid(a, a.Lq, 128), 3 * (2 * KVB * 2 * DH), a.s, a.q, a.q_rs, a.q_bs, a.dout, a.do_rs, a.do_bs, a.k, a.k_rs, a.k_bs,
                                               a.v, a.v_rs, a.v_bs, a.lse2, a.delta, a.stat_ld, a.dq, a.dq_rs, a.dq_bs, a.heads, a.Lq, a.Lkv, (a.Lq + 127) / 128,
                                               a.c, a.scale);
            return;
        }
    }
    bwd_launch<attn_bwd_kernel<DH, true>>(bwd_grid(a, a.Lq, 256), 2 * (2 * KVB * 2 * DH + 512), a.s, a.q, a.q_rs, a.q_bs, a.dout, a.do_rs, a.do_bs, a.k, a.k_rs, a.k_bs,
                                          a.v, a.v_rs, a.v_bs, a.lse2, a.delta, a.stat_ld, a.dq, a.dq_rs, a.dq_bs, a.heads, a.Lq, a.Lkv, (a.Lq + 255) / 256, a.c, a.scale);
}
template <int DH>
static void bwd_launch_dkv(const ug_attn_bwd_args& a) {            // 128 keys per workgroup, [3][Q tile | dO tile | statistics] + the exchanged operands
    bwd_launch<attn_bwd_dkv_kernel<DH>>(bwd_grid(a, a.Lkv, 128), 3 * (2 * KVB * 2 * DH + 512) + 2 * 8 * 2048, a.s, a.k, a.k_rs, a.k_bs, a.v, a.v_rs, a.v_bs, a.q, a.q_rs,
                                        a.q_bs, a.dout, a.do_rs, a.do_bs, a.lse2, a.delta, a.stat_ld, a.dk, a.dk_rs, a.dk_bs, a.dv, a.dv_rs, a.dv_bs, a.heads,
                                        a.Lkv, a.Lq, (a.Lkv + 127) / 128, a.c, a.scale);
}
template <int DH>
static void bwd_stages(const ug_attn_bwd_args& a, bool need_lse, bool pair_dq) {
#ifdef UG_PROBE_BUILD     // probe library: UG_ATTN_BWD_DMA=0 / UG_ATTN_BWD_FUSE_DKV=0 send a stage to the frozen template (tools/probe/csrc/attn_bwd_variants.hip)
    const auto variant = [&](int stage) { return ug_attn_bwd_variants(stage, DH, a); };
#else
    const auto variant = [](int) { return false; };
#endif
    if (need_lse && !variant(UG_BWD_STAGE_LSE)) bwd_launch_lse<DH>(a);
    if (!variant(UG_BWD_STAGE_DQ)) bwd_launch_dq<DH>(a, pair_dq);
    if (!variant(UG_BWD_STAGE_DKV)) bwd_launch_dkv<DH>(a);
}

extern "C" int64_t ug_flash_attn_bwd_workspace_bytes(int64_t batches, int32_t heads, int64_t Lq) {
    if (batches <= 0 || heads <= 0 || Lq <= 0) return 0;
    return 2 * batches * heads * ((Lq + 63) / 64 * 64) * (int64_t)sizeof(float);
}

extern "C" int ug_flash_attn_bwd(const void* q, int64_t q_rs, int64_t q_bs, const void* k, int64_t k_rs, int64_t k_bs, const void* v, int64_t v_rs,
                                 int64_t v_bs, const void* o, int64_t o_rs, int64_t o_bs, const void* dout, int64_t do_rs, int64_t do_bs, void* dq,
                                 int64_t dq_rs, int64_t dq_bs, void* dk, int64_t dk_rs, int64_t dk_bs, void* dv, int64_t dv_rs, int64_t dv_bs,
                                 int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale, const float* lse_in,
                                 void* workspace, int64_t workspace_bytes, ug_stream_t stream) {
    if (batches == 0 || Lq == 0) return UG_OK;
    UG_REQUIRE(q && k && v && o && dout && dq && dk && dv && batches > 0 && heads > 0 && Lq > 0 && Lkv > 0, UG_ERR_BAD_SHAPE, "ug_flash_attn_bwd: bad arguments");
    UG_REQUIRE(dh == 128 || dh == 64, UG_ERR_UNSUPPORTED, "ug_flash_attn_bwd: head dim %d not in {64, 128}", dh);
    UG_REQUIRE(Lq < (1 << 30) && Lkv < (1 << 30), UG_ERR_UNSUPPORTED, "ug_flash_attn_bwd: sequence too long");
    // the row-stride bound as in the forward: the streamed operands' LDS-DMAs hold 32-bit byte offsets over a 64-row tile (63 rs + 120 < 2^31)
    const ug_view_rule views[] = {{"q", {q, q_rs, q_bs}, 8, 16, true},          {"k", {k, k_rs, k_bs}, 8, 16, true},     {"v", {v, v_rs, v_bs}, 8, 16, true},
                                  {"o", {o, o_rs, o_bs}, 8, 16, true},          {"dout", {dout, do_rs, do_bs}, 8, 16, true},
                                  {"dq", {dq, dq_rs, dq_bs}, 8, 8, true},       {"dk", {dk, dk_rs, dk_bs}, 8, 8, true},  {"dv", {dv, dv_rs, dv_bs}, 8, 8, true}};
    if (const int rc = ug_check_views("ug_flash_attn_bwd", views)) return rc;
    const int64_t stat_ld = (Lq + 63) / 64 * 64;
    UG_REQUIRE(workspace && ug_aligned(workspace, 16) && workspace_bytes >= ug_flash_attn_bwd_workspace_bytes(batches, heads, Lq), UG_ERR_BAD_SHAPE,
               "ug_flash_attn_bwd: workspace of ug_flash_attn_bwd_workspace_bytes() needed");
    // lse_in: the statistics ug_flash_attn_fwd_lse wrote, [batches][heads][stat_ld] with the padding zero (saves the LSE launch); else computed here
    float* lse2 = lse_in ? const_cast<float*>(lse_in) : (float*)workspace;
    float* delta = (float*)workspace + batches * heads * stat_ld;
    hipStream_t s = (hipStream_t)stream;
    const float c = softmax_scale * 1.4426950408889634f;
    const int nQ = (int)((Lq + 255) / 256), nK = (int)((Lkv + 255) / 256);
    const int64_t gq = (int64_t)nQ * heads * batches, gk = (int64_t)nK * heads * batches;
    UG_REQUIRE(gq < (1ll << 31) && gk < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_flash_attn_bwd: grid too large");
    // fused dK / dV kernel: 128 keys per workgroup (equal row strides are NOT required)
    const int nK2 = (int)((Lkv + 127) / 128);
    const int64_t gk2 = (int64_t)nK2 * heads * batches;
    UG_REQUIRE(gk2 < (1ll << 31) && (int64_t)((Lq + 127) / 128) * heads * batches < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_flash_attn_bwd: grid too large");
    // dQ on 128-query workgroups (attn_bwd_dq_kernel); UG_ATTN_BWD_PAIR_DQ=0: the 256-query DQ mode
    const int64_t gq2 = (int64_t)((Lq + 127) / 128) * heads * batches;
    // Measured (tools/attn_bwd_ab.py, profiles/r03y_attn_bwd_pair_dq.log): dh 128 at 4608^2 / 8704^2 +2.6 % / +2.5 % of the whole backward; dh 128 at
    // 1000^2 -7 %, dh 64 -3 % (half the MFMAs per wave and barrier) -> on by default only for head width 128 and >= 2048 queries (2 forces it everywhere)
    const int pdq = UG_TUNE("UG_ATTN_BWD_PAIR_DQ", 1);
    const bool pair_dq = gq2 < (1ll << 31) && (pdq == 2 || (pdq == 1 && dh == 128 && Lq >= 2048));
    (void)hipMemsetAsync(workspace, 0, (size_t)(2 * batches * heads * stat_ld) * sizeof(float), s);     // padded statistics rows read as 0
    const int64_t total = batches * Lq * heads;
    const auto delta_launch = [&](auto kernel, int per_wg) {        // per_wg: the (batch, query, head) items of a workgroup, 256 / (dh / 8)
        hipLaunchKernelGGL(kernel, dim3((unsigned)((total + per_wg - 1) / per_wg)), dim3(256), 0, s, (const bf16_t*)o, o_rs, o_bs, (const bf16_t*)dout, do_rs,
                           do_bs, delta, stat_ld, total, (int)heads, (int)Lq);
    };
    if (dh == 128) delta_launch(attn_delta_kernel<128>, 16); else delta_launch(attn_delta_kernel<64>, 32);
    const ug_attn_bwd_args a = {(const bf16_t*)q, q_rs, q_bs, (const bf16_t*)k, k_rs, k_bs, (const bf16_t*)v, v_rs, v_bs, (const bf16_t*)dout, do_rs, do_bs,
                                (bf16_t*)dq, dq_rs, dq_bs, (bf16_t*)dk, dk_rs, dk_bs, (bf16_t*)dv, dv_rs, dv_bs, lse2, delta, stat_ld,
                                batches, (int)heads, (int)Lq, (int)Lkv, c, softmax_scale, s};
    if (dh == 128) bwd_stages<128>(a, !lse_in, pair_dq); else bwd_stages<64>(a, !lse_in, pair_dq);
    UG_CHECK_LAUNCH("ug_flash_attn_bwd");
    return UG_OK;
}
