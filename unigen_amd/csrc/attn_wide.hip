// Flash attention forward at head width 512: the single 512-wide head of the AutoencoderKL mid-block (unigen_amd/vae.py, _attention), whose
// default route materialises the [HW, HW] fp32 scores in HBM.  ug_flash_attn_fwd_wide (bf16) and its fp32 verification twin.
//   O = softmax(Q K^T * scale) V, non-causal, no mask, bf16 in/out, fp32 scores / statistics / accumulators, P rounded to bf16 as the P.V operand.
//
// Structure (gfx950, wave64). The two-waves-per-SIMD form of flash_attn_kernel (attention.hip) cannot hold this width: one wave's O accumulator for
// 32 query rows x 512 columns is 256 registers by itself. Here a workgroup is 4 waves = ONE wave per SIMD (__launch_bounds__(256): the whole
// 512-entry unified register file), each wave owning 32 query rows: 128 query rows of one (batch, head) per workgroup.
//   registers per lane: O^T 16 blocks x f32x16 = 256 (the accumulator half), Q fragments 32 x bf16x8 = 128, S^T 16, packed P 8, K / V fragments + addresses.
//   S^T = K Q^T   v_mfma_f32_32x32x16_bf16, 32 k-steps over the 512 columns on ONE accumulator: the query index lands on the LANE, so the softmax row
//                 statistics are lane-local (one exchange with lane ^ 32 per tile), exactly as in flash_attn_kernel.
//   O^T = V^T P^T the S^T registers 8s..8s+7, packed to bf16, ARE the B operand of k-step s; V through ds_read_b64_tr_b16. 16 d-blocks x 2 k-steps.
// K / V tiles of 32 keys (32 KiB each) go HBM -> LDS by LDS-DMA, double buffered: 2 x (K | V) = 128 KiB of dynamic LDS. A 512-wide tile is kept as
// FOUR PANELS of [32 keys][128 columns]: each panel is the XOR-swizzled 256-byte-row image of attn_common.h (row_swz<128>), conflict-free for the row
// reads (K) and the transposed reads (V) alike, so every LDS address of this kernel is one of flash_attn_kernel's at head width 128 plus a panel
// offset. Wave w stages panel w of K and of V: 8 + 8 one-KiB DMAs per tile, issued at the top of the tile that precedes their use and waited for at
// its end; one barrier per tile. Per tile a wave issues 32 + 32 MFMAs against 64 KiB of LDS reads and 16 v_exp_f32 per lane: matrix-paced.
// Ragged tails: rows past Lkv re-read the last key and their scores are masked to -inf; query rows past Lq re-read the last query and skip the store.
// No workspace, no atomics, nothing kept between launches.
#include "ug_common.h"
#include "attn_common.h"

namespace {

constexpr int WDH = 512;                 // head width
constexpr int WKV = 32;                  // keys per tile
constexpr int WQR = 128;                 // query rows per workgroup (4 waves x 32)
constexpr int WPANEL = WKV * 256;        // one [32 keys][128 columns] panel: 8 KiB
constexpr int WTILE = 4 * WPANEL;        // a K (or V) tile: 32 KiB
constexpr int WBUF = 2 * WTILE;          // K tile | V tile
constexpr int WLDS = 2 * WBUF;           // double buffered: 128 KiB

__global__ __launch_bounds__(256) void flash_attn_wide_kernel(
    const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_bs, const bf16_t* __restrict__ k, int64_t k_rs, int64_t k_bs,
    const bf16_t* __restrict__ v, int64_t v_rs, int64_t v_bs, bf16_t* __restrict__ o, int64_t o_rs, int64_t o_bs,
    int heads, int Lq, int Lkv, int nQ, float c /* softmax_scale * log2(e) */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][K tile | V tile], each tile 4 panels
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // XCD-aware block order, as in flash_attn_kernel: the query tiles of one (batch, head) run on one XCD so its K / V stay in that L2
    const int nwg = gridDim.x;
    const int qd = nwg >> 3, rm = nwg & 7;
    const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
    const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + kk;
    // the divisions run on the VALU, so hipcc takes their (wave-uniform) results for per-lane values: the (batch, head) base pointers derived from
    // them would be 64-bit VGPR pairs, live through the loop, in a kernel that has no register to spare
    const int qt = __builtin_amdgcn_readfirstlane(logical % nQ), bh = __builtin_amdgcn_readfirstlane(logical / nQ);
    const int head = __builtin_amdgcn_readfirstlane(bh % heads), b = __builtin_amdgcn_readfirstlane(bh / heads);

    const bf16_t* Qb = q + (int64_t)b * q_bs + head * WDH;
    const bf16_t* Kb = k + (int64_t)b * k_bs + head * WDH;
    const bf16_t* Vb = v + (int64_t)b * v_bs + head * WDH;

    // ---- Q fragments (B operand of S^T = K Q^T): lane (r, h) holds Q[q = r][d = 16 s + 8 h + j] ----
    const int q_row = qt * WQR + wave * 32 + r;
    const int q_ld = q_row < Lq ? q_row : Lq - 1;
    bf16x8 qf[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) qf[s] = *(const bf16x8*)(Qb + (int64_t)q_ld * q_rs + 16 * s + 8 * h);

    // ---- LDS-DMA staging: wave w owns panel w; run j of a panel = its rows 4j .. 4j + 3 (1 KiB), lane l lands at byte 16 l of the run and so
    // fetches chunk (l % 16) ^ row_swz(row) of row 4j + l / 16 (the swizzle is applied on the source side) ----
    const int d_q = lane >> 4, d_c0 = (lane & 15) ^ (d_q << 2);           // row_swz<128>(4j + q) = (q << 2) | (j & 3)
    const int ntiles = (Lkv + WKV - 1) / WKV;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wave * WPANEL;
    auto dma_panel = [&](const bf16_t* base, int64_t rs, int tile, unsigned dst) __attribute__((always_inline)) {
        if (tile * WKV + WKV <= Lkv) {             // whole tile: wave-uniform base (SGPR pair) + per-lane 32-bit byte offset
            const void* tb = uniform_ptr(base + (int64_t)tile * WKV * rs + wave * 128);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                glds16_off(tb, (unsigned)((4 * j + d_q) * (int)rs + ((d_c0 ^ (j & 3)) << 3)) * 2u, dst + j * 1024);
        } else {                                   // ragged last tile: rows past the end re-read the last key (masked in S^T)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int key = tile * WKV + 4 * j + d_q; if (key > Lkv - 1) key = Lkv - 1;
                glds16_ptr(base + (int64_t)key * rs + wave * 128 + ((d_c0 ^ (j & 3)) << 3), dst + j * 1024);
            }
        }
    };
    auto dma_fetch = [&](int tile) __attribute__((always_inline)) {     // K and V of `tile` into buffer tile & 1
        const unsigned dst = lds0 + (tile & 1) * WBUF;
        dma_panel(Kb, k_rs, tile, dst);
        dma_panel(Vb, v_rs, tile, dst + WTILE);
    };
    auto tile_barrier = [&]() __attribute__((always_inline)) {          // this wave's DMAs landed and its LDS reads returned, then everybody's
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    dma_fetch(0);
    // Retire the Q loads here (see flash_attn_kernel): the fragments are read-write operands of an empty asm, so hipcc has them in hand before the loop
    // and does not re-wait for them - with a vmcnt that would drain the K / V prefetch - in every iteration.
#pragma unroll
    for (int s = 0; s < 32; s += 8)
        asm volatile("" : "+v"(qf[s]), "+v"(qf[s + 1]), "+v"(qf[s + 2]), "+v"(qf[s + 3]), "+v"(qf[s + 4]), "+v"(qf[s + 5]), "+v"(qf[s + 6]), "+v"(qf[s + 7]));
    tile_barrier();

    // ---- per-lane LDS read offsets inside a panel (those of flash_attn_kernel at head width 128) ----
    // K row read: row = r, chunk = 2 s' + h  ->  256 r + 16 ((2 s') ^ kx),  kx = h ^ row_swz(r)
    const int k_rowoff = 256 * r;
    const int kx = h ^ row_swz<128>(r);
    // V transposed read: group g = lane >> 4, i = lane & 15. Block rows = keys 16 ks + 4 h + (i >> 2) (+ 8 for the second half of the k-step),
    // columns d = 32 db + 16 (g & 1) + 4 (i & 3) .. + 3. The lane receives column d = 32 db + (lane & 31).
    const int i16 = lane & 15, g16 = lane >> 4;
    const int v_key = 4 * h + (i16 >> 2);
    const int v_lowch = 2 * (g16 & 1) + ((i16 & 3) >> 1);
    const int v_b8 = 8 * (i16 & 1);
    int voff_lo[4], voff_hi[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        const int ch = 4 * db + v_lowch;
        voff_lo[db] = 256 * v_key + 16 * (ch ^ row_swz<128>(v_key)) + v_b8;
        voff_hi[db] = 256 * (v_key + 8) + 16 * (ch ^ row_swz<128>(v_key + 8)) + v_b8;
    }

    f32x16 oacc[16];
#pragma unroll
    for (int db = 0; db < 16; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) dma_fetch(t + 1);      // into the buffer every wave finished reading before the last barrier
        const unsigned char* Kbuf = smem + (t & 1) * WBUF;
        const unsigned char* Vbuf = Kbuf + WTILE;
        // ---- S^T = K Q^T: 32 k-steps on one accumulator ----
        // fragments are read one group of four k-steps ahead of their MFMAs (a sched_barrier per group keeps hipcc from hoisting all 32 reads:
        // with the 256 accumulator and 128 Q registers there is room for two groups in flight, not for eight)
        f32x16 sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
        bf16x8 kf[2][4];
        auto rdk = [&](int g) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 4 * g + j;
                kf[g & 1][j] = *(const bf16x8*)(Kbuf + (s >> 3) * WPANEL + k_rowoff + 16 * ((2 * (s & 7)) ^ kx));
            }
        };
        rdk(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g + 1 < 8) rdk(g + 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[g & 1][j], qf[4 * g + j], sacc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int kv0 = t * WKV;
        if (kv0 + WKV > Lkv) {                     // ragged last tile: keys >= Lkv do not exist
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kv0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (key >= Lkv) sacc[i] = -INFINITY;
            }
        }
        // ---- online softmax, lane-local (this lane: query r, 16 of the tile's 32 keys; lane ^ 32 has the rest) ----
        float tmax = sacc[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) tmax = fmaxf(tmax, sacc[i]);
        tmax = ug_max_halves(tmax);
        // lazy reference point, as in flash_attn_kernel: a row's running max moves only when the tile maximum exceeds it by more than 2^8 in the
        // exponent (P and l stay below 2^8 per element); here the rescale it saves is 256 accumulator registers per lane
        const bool up = (tmax - m_run) * c > 8.0f;
        const float m_new = up ? tmax : m_run;
        if (!__all(!up)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
            l_run *= alpha;
            // The accumulators live in the AGPR half and hipcc's own form of this multiply copies all 256 into VGPRs it does not have (239 spilled):
            // each register is read, scaled and written back in place by one asm statement instead (VALU only: no wait states between the three).
#pragma unroll
            for (int db = 0; db < 16; ++db) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float tmp;
                    asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1" : "+a"(oacc[db][i]), "=&v"(tmp) : "v"(alpha));
                }
            }
            asm volatile("s_nop 7" ::: "memory");   // v_accvgpr_write -> MFMA source C: hipcc pads nothing behind an asm statement
            m_run = m_new;
        }
        const float mc = m_run * c;
        float p[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            p[i] = __builtin_amdgcn_exp2f(fmaf(sacc[i], c, -mc));
            l_run += p[i];
        }
        bf16x8 pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            u32x4 w;
            w.x = pack2bf(p[8 * s2 + 0], p[8 * s2 + 1]); w.y = pack2bf(p[8 * s2 + 2], p[8 * s2 + 3]);
            w.z = pack2bf(p[8 * s2 + 4], p[8 * s2 + 5]); w.w = pack2bf(p[8 * s2 + 6], p[8 * s2 + 7]);
            pf[s2] = __builtin_bit_cast(bf16x8, w);
        }
        // ---- O^T += V^T P^T: 2 k-steps x 16 d-blocks (d-block db = panel db / 4, block db % 4 of it) ----
        bf16x8 vf[2][4];
        auto rdv = [&](int g) __attribute__((always_inline)) {        // group g: k-step g / 4, d-blocks 4 (g % 4) .. + 3 = panel g % 4
            const unsigned char* vb = Vbuf + (g & 3) * WPANEL + (g >> 2) * 16 * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j) vf[g & 1][j] = tr_read_pair(vb + voff_lo[j], vb + voff_hi[j]);
        };
        rdv(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g + 1 < 8) rdv(g + 1);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                oacc[4 * (g & 3) + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[g & 1][j], pf[g >> 2], oacc[4 * (g & 3) + j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        tile_barrier();
    }

    // ---- epilogue: O[q][d] = O^T / l (the store form of flash_attn_kernel: one v_permlane32_swap per dword pair, 16-byte stores) ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    // the row's address is re-derived here from an opaque copy of the thread index: held through the loop it would be spilled
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));
    const int h_e = (tid_e >> 5) & 1;
    const int q_row_e = qt * WQR + (tid_e >> 6) * 32 + (tid_e & 31);
    bf16_t* Orow = o + (int64_t)b * o_bs + (int64_t)(q_row_e < Lq ? q_row_e : Lq - 1) * o_rs + head * WDH + 8 * h_e;
#pragma unroll
    for (int db = 0; db < 16; ++db)
#pragma unroll
        for (int k2 = 0; k2 < 4; k2 += 2) {
            unsigned ax = pack2bf(oacc[db][4 * k2 + 0] * inv, oacc[db][4 * k2 + 1] * inv), ay = pack2bf(oacc[db][4 * k2 + 2] * inv, oacc[db][4 * k2 + 3] * inv);
            unsigned bx = pack2bf(oacc[db][4 * k2 + 4] * inv, oacc[db][4 * k2 + 5] * inv), by = pack2bf(oacc[db][4 * k2 + 6] * inv, oacc[db][4 * k2 + 7] * inv);
            auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
            auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
            u32x4 w; w.x = rx[0]; w.y = ry[0]; w.z = rx[1]; w.w = ry[1];
            if (q_row_e < Lq) *(u32x4*)(Orow + 32 * db + 8 * k2) = w;
            __builtin_amdgcn_sched_barrier(0);      // one 16-byte store at a time: hipcc otherwise copies the accumulators out wholesale and spills
        }
}

}  // namespace

extern "C" int ug_flash_attn_fwd_wide(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k,
                                      int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
                                      int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                                      int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                                      ug_stream_t stream) {
    if (batches == 0 || Lq == 0) return UG_OK;
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && Lq > 0 && Lkv > 0, UG_ERR_BAD_SHAPE, "ug_flash_attn_fwd_wide: bad arguments");
    UG_REQUIRE(dh == WDH, UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide: head dim %d is not 512 (64 and 128: ug_flash_attn_fwd)", dh);
    UG_REQUIRE(Lq < (1 << 30) && Lkv < (1 << 30), UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide: sequence too long");
    // the row-stride bound: the LDS-DMAs address a tile's 32 rows of K and V with 32-bit byte offsets from the tile's base
    const ug_view_rule views[] = {{"q", UG_VIEW(q), 8, 16, false}, {"k", UG_VIEW(k), 8, 16, true}, {"v", UG_VIEW(v), 8, 16, true}, {"o", UG_VIEW(o), 4, 8, false}};
    if (const int rc = ug_check_views(__func__, views)) return rc;
    UG_REQUIRE(softmax_scale > 0.f, UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide: softmax_scale must be positive");
    const int nQ = (int)((Lq + WQR - 1) / WQR);
    const int64_t nwg = (int64_t)nQ * heads * batches;
    UG_REQUIRE(nwg < (1ll << 31), UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide: grid too large");
    // 128 KiB of dynamic LDS: above the 64 KiB default limit, allowed once per process (as bwd_launch in attention.hip)
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)flash_attn_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WLDS); attr = true; }
    hipLaunchKernelGGL(flash_attn_wide_kernel, dim3((unsigned)nwg), dim3(256), WLDS, (hipStream_t)stream, (const bf16_t*)q, q_row_stride, q_batch_stride,
                       (const bf16_t*)k, k_row_stride, k_batch_stride, (const bf16_t*)v, v_row_stride, v_batch_stride, (bf16_t*)o, o_row_stride,
                       o_batch_stride, (int)heads, (int)Lq, (int)Lkv, nQ, softmax_scale * 1.4426950408889634f);
    UG_CHECK_LAUNCH("ug_flash_attn_fwd_wide");
    return UG_OK;
}

extern "C" int ug_flash_attn_fwd_wide_f32(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k,
                                          int64_t k_row_stride, int64_t k_batch_stride, const void* v, int64_t v_row_stride,
                                          int64_t v_batch_stride, void* o, int64_t o_row_stride, int64_t o_batch_stride,
                                          int64_t batches, int32_t heads, int64_t Lq, int64_t Lkv, int32_t dh, float softmax_scale,
                                          ug_stream_t stream) {
    if (batches == 0 || Lq == 0) return UG_OK;
    UG_REQUIRE(q && k && v && o && batches > 0 && heads > 0 && Lq > 0 && Lkv > 0, UG_ERR_BAD_SHAPE, "ug_flash_attn_fwd_wide_f32: bad arguments");
    UG_REQUIRE(dh == WDH, UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide_f32: head dim %d is not 512 (64 and 128: ug_flash_attn_fwd_f32)", dh);
    UG_REQUIRE(Lq < (1 << 30) && Lkv < (1 << 30), UG_ERR_UNSUPPORTED, "ug_flash_attn_fwd_wide_f32: sequence too long");
    // verify_f32.hip's one kernel, 16 lanes per query row (a [64][512 + 4] fp32 query image in LDS, its form at head width 64 and 128, would be 132 KB)
    return ug_flash_attn_f32_launch(__func__, UG_VIEW(q), UG_VIEW(k), UG_VIEW(v), UG_VIEW(o), batches, heads, Lq, Lkv, dh, softmax_scale, {}, stream);
}
