// bf16 MFMA GEMM, ONE WAVE PER SIMD: 256 x 256 output tile per workgroup, 4 waves x (128 x 128) sub-tiles, up to 512 registers per lane.
//
// Why a second structure next to gemm256_kernel (gemm.hip): the 8-wave kernel hands the matrix pipe back and forth between the two waves
// of a SIMD with 8 barrier pairs per 64-deep K-tile and keeps it busy ~64 % of the time (PMC, round 1); its fragments are re-read from LDS
// at 0.375 ds_read_b128 per MFMA. Here a single in-order wave per SIMD overlaps its own LDS reads and LDS-DMA issue with its MFMAs:
//   * per 32-deep K-step a wave issues 64 x v_mfma_f32_16x16x32_bf16 (8 x 8 accumulators of 16 x 16, 256 registers, AGPR side) against
//     16 ds_read_b128 (0.25 per MFMA) for the NEXT step's fragments (two register sets, 128 VGPRs) and 8 LDS-DMA pieces;
//   * ONE barrier per K-step (1024 MFMA cycles) instead of 4 per 1024;
//   * a 4-slot LDS ring of 32 KiB steps [A 256 x 32 | W 256 x 32], refilled 4 steps ahead (global_load_lds_dwordx4, counted vmcnt(16)):
//     step s + 4 is requested during step s into the slot whose fragments were just moved to registers.
// LDS image of a step: 64-byte rows (32 bf16); 16-byte chunk c of row r is stored at position c ^ f((r >> 2) & 3), f = {0, 3, 2, 1}: every
// 16-lane group of a ds_read_b128 (cdna guide, LDS table) then touches 16 distinct 16-byte slots of the 256-byte bank row - conflict-free -
// and the DMA writes stay lane-linear (the permutation is applied to the per-lane SOURCE chunk, guide rule 21).
// Epilogues, row maps, grouped launches, the column split and the XCD-aware tile order are the shared ones of gemm_epilogue.h.
#include "ug_common.h"
#include "gemm_epilogue.h"
#include <type_traits>

namespace {

constexpr int PK = 32;                         // K per step
constexpr int PHALF = 256 * PK * 2;            // bytes of one operand of a step (16 KiB)
constexpr int PSLOT = 2 * PHALF;               // 32 KiB

__device__ __forceinline__ int swz32(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// NW = 4: one wave per SIMD, 128 x 128 per wave (512 registers). NW = 8: two waves per SIMD, 128 x 64 per wave (256 registers): the same
// self-contained step body per wave, but a wave's LDS-DMA issue (which holds its own instruction stream ~35 cycles per 1 KiB piece: measured
// by building the NW = 4 loop without its DMAs, 1340 -> 1620 TFLOP/s at 8192^3) now runs under the SIMD partner's MFMAs.
// VAR (diagnostic builds, UG_PWG_VAR): bit 0 = no DMA in the loop (WRONG results, timing only), bit 1 = waves 4-7 issue their DMAs in the
// second half of the step (stagger against waves 0-3); bit 2 = every wave issues all its LDS reads in the first half of the step.
template <int EPI, int NW, int VAR, int PRING = 4>      // PRING: LDS ring slots (32 KiB each); 5 = all 160 KiB
__global__ __launch_bounds__(64 * NW, NW / 4) void gemm_pwg_kernel(const ug_gemm_desc p, const int tiles_per_group, const int total_tiles) {
    constexpr int NT = 32 / NW;                    // 16-column blocks per wave: 8 (128 columns) or 4 (64 columns)
    constexpr int RPW = 256 / NW;                  // rows of A (and of W) a wave stages per step
    constexpr int NPC = RPW / 16;                  // DMA pieces per operand per wave per step: 4 or 2
    constexpr int NG = 2 * NT;                     // MFMA groups of 4 per step: 16 or 8
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / (NW / 2), wc = wave % (NW / 2);
    const int64_t M = p.M, N = p.N;
    const int nM = (int)((M + 255) / 256), nN = (int)((N + 255) / 256);
    const int nsteps = (int)(p.K / PK);
    const int frow = lane & 15, fch = lane >> 4;
    const int a_off = (wr * 128 + frow) * 64 + ((fch ^ swz32(frow)) << 4);
    const int b_off = PHALF + (wc * 16 * NT + frow) * 64 + ((fch ^ swz32(frow)) << 4);
    const bool late = (VAR & 2) && wave >= NW / 2;

    for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const int g = tile / tiles_per_group;
        const TileCoord tc = tile_of_block(tile - g * tiles_per_group, nM, nN);
        const int64_t m0 = (int64_t)tc.tm * 256, n0 = (int64_t)tc.tn * 256;
        // ---- staging sources: wave w stages rows [RPW w, RPW (w + 1)) of A and of W, 16 rows (1 KiB) per DMA ----
        const bf16_t* asrc[NPC]; const bf16_t* bsrc[NPC];
        {
            const bf16_t* Ab = (const bf16_t*)p.A + (int64_t)g * p.a_gstride;
            const bf16_t* Wb = (const bf16_t*)p.W + (int64_t)g * p.w_gstride;
#pragma unroll
            for (int i = 0; i < NPC; ++i) {
                const int row = wave * RPW + i * 16 + (lane >> 2);
                const int c = (lane & 3) ^ swz32(row);
                int64_t am = m0 + row; if (am > M - 1) am = M - 1;
                int64_t wn = n0 + row; if (wn > N - 1) wn = N - 1;
                asrc[i] = Ab + (int64_t)rowmap32((unsigned)am, (unsigned)p.a_rpb, (unsigned)p.a_bstride) * p.lda + c * 8;
                bsrc[i] = Wb + wn * p.ldw + c * 8;
            }
        }
        // one LDS-DMA piece (1 KiB) of K-step `src_step`, into ring slot `slot_step` % 4: pieces [0, NPC) = this wave's A rows, then its W rows
        auto stage_piece = [&](int piece, int slot_step, int src_step) {
            unsigned char* slot = smem + (slot_step % PRING) * PSLOT + wave * RPW * 64;
            const int64_t ko = (int64_t)src_step * PK;
            if (piece < NPC) glds16(asrc[piece] + ko, slot + piece * 1024);
            else glds16(bsrc[piece - NPC] + ko, slot + PHALF + (piece - NPC) * 1024);
        };
        // Accumulators live in AGPRs and are touched only by the (inline-asm) MFMAs until the epilogue; the two fragment sets live in VGPRs.
        // As builtins in a branchy loop hipcc kept part of the accumulators in VGPRs, copied them through v_accvgpr_* around every step and
        // spilled 360 registers (first build); with explicit operand classes and a branch-free step body there is nothing left to decide.
        f32x4 acc[8][NT];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if constexpr (VAR & 32) asm volatile("" : "+v"(acc[i][j])); else asm volatile("" : "+a"(acc[i][j]));
            }
        bf16x8 af[2][8], bf[2][NT];
        // The previous tile's last step left every LDS read retired (its MFMAs consumed them); its epilogue stores may still be in
        // flight, which only makes the counted waits below wait a little longer (stores retire in issue order ahead of these DMAs).
        __builtin_amdgcn_s_barrier();
        const int last = nsteps - 1;
#pragma unroll
        for (int st = 0; st < PRING; ++st)
#pragma unroll
            for (int pc = 0; pc < 2 * NPC; ++pc) stage_piece(pc, st, st < last ? st : last);      // steps past the end: clamped re-reads nobody consumes
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PRING - 1) * 2 * NPC) : "memory");             // step 0 landed (the younger steps may fly)
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int t = 0; t < 8; ++t) af[0][t] = *(const bf16x8*)(smem + a_off + t * 1024);
#pragma unroll
        for (int t = 0; t < NT; ++t) bf[0][t] = *(const bf16x8*)(smem + b_off + t * 1024);

        auto step = [&](auto set_c, int s) __attribute__((always_inline)) {
            constexpr int SET = decltype(set_c)::value;
            // top of step s: this step's fragments (set SET) were requested during step s - 1; step s + 1's slot must have landed before
            // anybody reads it below: issued so far are steps <= s + PRING - 1, so all but the PRING - 2 youngest steps must be complete.
            if constexpr (VAR & 8) {
                // paired refill: DMAs only in odd steps (steps s + 3 and s + 4 = the two 64-byte halves of the same 128-byte lines, back to back)
                if constexpr (SET == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NPC) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPC) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PRING - 2) * 2 * NPC) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();           // every wave has its set-SET fragments in registers: slot s % 4 is free, slot (s+1) % 4 visible
            __builtin_amdgcn_sched_barrier(0);
            const unsigned char* nslot = smem + ((s + 1) % PRING) * PSLOT;       // past the end: a stale slot, read and never used
            const int src4 = s + PRING < nsteps ? s + PRING : last;     // the step refilled now: s + PRING (named src4 for the 4-slot ring)
            // per group of 4 MFMAs: fragment reads of the next step (8 A + NT W over the groups), and the 2 NPC DMA pieces of step s + 4
            auto reads = [&](int i) __attribute__((always_inline)) {          // read slot i of 0 .. NG - 1
                constexpr int NR = 8 + NT;
                constexpr int RG = (VAR & 4) ? NG / 2 : NG;             // VAR bit 2: all reads in the first half of the step
                if (i >= RG) return;
                for (int r = (i * NR) / RG; r < ((i + 1) * NR) / RG; ++r) {
                    if (r < 8) af[SET ^ 1][r] = *(const bf16x8*)(nslot + a_off + r * 1024);
                    else bf[SET ^ 1][r - 8] = *(const bf16x8*)(nslot + b_off + (r - 8) * 1024);
                }
            };
            const int src3 = s + 3 < nsteps ? s + 3 : last;
            auto dmas = [&](int i) __attribute__((always_inline)) {           // DMA slot i of 0 .. NG - 1
                if constexpr (VAR & 8) {
                    if constexpr (SET == 1) {
                        constexpr int ND = 4 * NPC;
                        for (int d = (i * ND) / NG; d < ((i + 1) * ND) / NG; ++d) {
                            if (d < 2 * NPC) stage_piece(d, s + 3, src3); else stage_piece(d - 2 * NPC, s + 4, src4);
                        }
                    }
                } else if constexpr (!(VAR & 1)) {
                    constexpr int ND = 2 * NPC;
                    for (int d = (i * ND) / NG; d < ((i + 1) * ND) / NG; ++d) stage_piece(d, s + PRING, src4);
                }
            };
#pragma unroll
            for (int i = 0; i < NG; ++i) {
#pragma unroll
                for (int q = 4 * i; q < 4 * i + 4; ++q) {
                    const int mt = q / NT, nt = q % NT;
                    if constexpr (VAR & 16) asm volatile("" :: "v"(bf[SET][nt]), "v"(af[SET][mt]));      // diagnostic: DMA + LDS reads only, no MFMA
                    else if constexpr (VAR & 32) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[mt][nt]) : "v"(bf[SET][nt]), "v"(af[SET][mt]));
                    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[mt][nt]) : "v"(bf[SET][nt]), "v"(af[SET][mt]));
                }
                reads(i);
                if constexpr (VAR & 2) { if (late) dmas((i + NG / 2) % NG); else dmas(i); }
                else dmas(i);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int s = 0; s < nsteps; s += 2) {
            step(std::integral_constant<int, 0>{}, s);
            if (s + 1 < nsteps) step(std::integral_constant<int, 1>{}, s + 1);
        }
        // every DMA still in flight targets slots nobody reads again; drain them before the next tile re-stages the ring, and give the last
        // MFMAs' results their cycles before VALU reads them (hipcc does not see an MFMA in the asm statements: 4 passes, s_nop 15 covers it)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15" ::: "memory");

        // ---- epilogue: lane holds, for row m = .. + mt * 16 + (lane & 15), columns nt * 16 + 4 (lane >> 4) .. + 3 ----
        const bf16_t* bias = p.bias ? (const bf16_t*)p.bias + (int64_t)g * p.bias_gstride : nullptr;
        const TileSplit ts = tile_split<EPI>(p, n0);
        float bv[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int64_t n = n0 + wc * 16 * NT + nt * 16 + (lane >> 4) * 4;
            load_bias4(n < N ? bias : nullptr, n, bv[nt]);
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int64_t m = m0 + wr * 128 + mt * 16 + (lane & 15);
            const bool row_ok = m < M;                         // lanes l and l ^ 16 share the row: the swaps stay paired
            RowCtx rc = row_ctx<EPI>(p, g, (unsigned)(row_ok ? m : M - 1));
            rc.coff += ts.cshift;
#pragma unroll
            for (int np = 0; np < NT / 2; ++np) {
                if (EPI == UG_EPI_BIAS_GELU && !ts.gelu)
                    epi_store_pair16<UG_EPI_BIAS>(p, rc, row_ok, n0 + wc * 16 * NT + np * 32, N, lane, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
                else
                    epi_store_pair16<EPI>(p, rc, row_ok, n0 + wc * 16 * NT + np * 32, N, lane, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
            }
        }
    }
}

// =====================================================================================================================
// Round 3: the WHOLE-LINE variant of the one-wave-per-SIMD structure ("build, do not estimate").
// The kernel above moves its operands in 64-byte row pieces (32-deep K-steps: two requests per 128-byte L2 line), which caps its
// intake at ~46 GB/s per CU. Here the ring unit is ONE OPERAND of a 64-deep K-tile: 256 rows x 128 bytes = 32 KiB, whole lines, the same
// swizzled image as gemm256_kernel (16-byte chunk c of row r at position c ^ (r & 7)); a 1-KiB LDS-DMA piece is 8 rows x 128 B.
// Five units fill the 160 KiB of LDS; unit index u = 2 T (A of K-tile T) or 2 T + 1 (W of K-tile T) lives in slot u % 5.
// Compute steps stay 32 deep (64 MFMAs of 16x16x32 per wave against 16 ds_read_b128 for the NEXT step's fragments, accumulators in
// AGPRs); K-tile T = steps 2 T (chunks 0-3 of a row) and 2 T + 1 (chunks 4-7). A(T) and W(T) are free once the fragments of step
// 2 T + 1 are in registers, i.e. at the barrier on top of step 2 T + 1 - the ONLY barrier per K-tile (2048 MFMA cycles). Refill:
//   step 2 T + 1 issues W(T + 2) into A(T)'s slot, step 2 T + 2 issues A(T + 3) into W(T)'s slot (8 pieces per wave and step);
//   the top of step 2 T + 1 waits vmcnt(8): everything but A(T + 2) - in particular A(T + 1), W(T + 1), read during this step - landed.
// W units have 1-2 steps of lead, A units 3-4. Epilogue: the generic one of the kernel above (this is a measurement build of the
// main loop, reachable through UG_GEMM_PWG=3; the fused epilogues / split-K tail / LoRA segment live in gemm256_kernel).
// =====================================================================================================================
constexpr int QU = 256 * 64 * 2;               // bytes of one ring unit (32 KiB)
constexpr int QRING = 5;

template <int EPI, int VAR>
__global__ __launch_bounds__(256, 1) void gemm_pwg64_kernel(const ug_gemm_desc p, const int tiles_per_group, const int total_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t M = p.M, N = p.N;
    const int nM = (int)((M + 255) / 256), nN = (int)((N + 255) / 256);
    const int nkt = (int)(p.K / 64);
    const int nsteps = 2 * nkt;

    for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        // lane-derived constants of the K loop, re-derived per tile from an opaque copy of the lane id: kept live across the tile loop they were
        // spilled around the epilogue (which moves 256 accumulators through the VGPRs) and reloaded - with a vmcnt(0) - inside the step loop
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        const int frow = lane_m & 15, fch = lane_m >> 4;
        // fragment byte offsets inside a unit for k-half 0 / 1 (chunks fch / 4 + fch), before the 16-row tile offset t * 2048
        const int a_row = (wr * 128 + frow) * 128, b_row = (wc * 128 + frow) * 128;
        const int ch_h0 = ((fch ^ (frow & 7)) << 4), ch_h1 = (((4 + fch) ^ (frow & 7)) << 4);
        const int g = tile / tiles_per_group;
        const TileCoord tc = tile_of_block(tile - g * tiles_per_group, nM, nN, 4);
        const int64_t m0 = (int64_t)tc.tm * 256, n0 = (int64_t)tc.tn * 256;
        // staging sources: wave w stages rows [64 w, 64 w + 64) of every unit, 8 rows (1 KiB) per piece. Whole tiles only (the launcher checks
        // M, N, the A row map's rows-per-batch are multiples of 256): piece i is piece 0 plus i * 8 rows, so two 64-bit lane pointers and
        // wave-uniform byte offsets replace sixteen lane pointers (32 registers: the first build spilled 80)
        const bf16_t* a0; const bf16_t* b0;
        {
            const bf16_t* Ab = (const bf16_t*)p.A + (int64_t)g * p.a_gstride;
            const bf16_t* Wb = (const bf16_t*)p.W + (int64_t)g * p.w_gstride;
            const int row = wave * 64 + (lane_m >> 3);
            const int c = (lane_m & 7) ^ (row & 7);        // rows i * 8 further on have the same (row & 7)
            a0 = Ab + (int64_t)rowmap32((unsigned)(m0 + row), (unsigned)p.a_rpb, (unsigned)p.a_bstride) * p.lda + c * 8;
            b0 = Wb + (n0 + row) * p.ldw + c * 8;
        }
        const int64_t a_pc = 8 * p.lda, b_pc = 8 * p.ldw;      // elements between consecutive pieces
        // buffer form (VAR & 2): resources over the whole operand, per-lane byte offsets of this tile's first piece (the launcher checks they fit 32 bits)
        const bf16_t* const Ab_ = (const bf16_t*)p.A + (int64_t)g * p.a_gstride;
        const bf16_t* const Wb_ = (const bf16_t*)p.W + (int64_t)g * p.w_gstride;
        const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)Ab_, 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)Wb_, 0, 0xffffffff, 0x00020000);
        const int vo_a = (int)((a0 - Ab_) * 2), vo_b = (int)((b0 - Wb_) * 2);
        auto stage_unit = [&](int u, int pc0, int pc1) __attribute__((always_inline)) {     // pieces [pc0, pc1) of unit u (K-tile u >> 1, past the end: clamped re-reads)
            int T = u >> 1; if (T > nkt - 1) T = nkt - 1;
            unsigned char* dst = smem + (u % QRING) * QU + wave * 64 * 128;
            const int64_t ko = (int64_t)T * 64;
            // the piece address is formed where it is used (one 64-bit add of a wave-uniform offset): hoisted out of the step loop, hipcc kept all
            // sixteen piece pointers live and spilled fragment addresses around them (scratch reloads + vmcnt(0) inside the loop)
            const bf16_t* base = (u & 1) ? b0 : a0;
            asm volatile("" : "+v"(base));
            const int64_t pc = (u & 1) ? b_pc : a_pc;
            if constexpr (VAR & 2) {
                // round 4: the vendor kernel's DMA form (hipBLASLt Custom_Cijk_..._MT256x256x64: buffer_load_dwordx4 ... offen lds) - a buffer resource per
                // operand, ONE loop-invariant per-lane byte offset, the K / piece offset as a scalar, M0 the destination: no VALU per DMA at all
                for (int i = pc0; i < pc1; ++i) {
                    const int so = (int)((ko + i * pc) * 2);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds((u & 1) ? rs_b : rs_a, (__attribute__((address_space(3))) void*)(dst + i * 1024), 16,
                                                             (u & 1) ? vo_b : vo_a, so, 0, 0);
                }
            } else {
                for (int i = pc0; i < pc1; ++i) glds16(base + (ko + i * pc), dst + i * 1024);
            }
        };
        f32x4 acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; asm volatile("" : "+a"(acc[i][j])); }
        bf16x8 af[2][8], bf[2][8];
        __builtin_amdgcn_s_barrier();                       // the previous tile's last reads retired (its MFMAs consumed them)
        if constexpr (!(VAR & 1)) {
#pragma unroll
            for (int u = 0; u < QRING; ++u) stage_unit(u, 0, 8);
        }
        asm volatile("s_waitcnt vmcnt(24)" ::: "memory");   // A(0), W(0) landed
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int t = 0; t < 8; ++t) af[0][t] = *(const bf16x8*)(smem + 0 * QU + a_row + t * 2048 + ch_h0);
#pragma unroll
        for (int t = 0; t < 8; ++t) bf[0][t] = *(const bf16x8*)(smem + 1 * QU + b_row + t * 2048 + ch_h0);

        auto step = [&](auto set_c, int s) __attribute__((always_inline)) {
            constexpr int SET = decltype(set_c)::value;      // SET = s & 1: even steps compute k-half 0 and read k-half 1 of the same K-tile
            const int T = s >> 1;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (SET == 1) {
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();                // A(T), W(T) free; A(T + 1), W(T + 1) visible
            }
            __builtin_amdgcn_sched_barrier(0);
            // fragments of step s + 1: SET == 0 -> K-tile T, k-half 1; SET == 1 -> K-tile T + 1, k-half 0 (past the end: stale, never used)
            const int Tn = SET == 0 ? T : T + 1;
            const unsigned char* ua = smem + ((2 * Tn) % QRING) * QU + a_row + (SET == 0 ? ch_h1 : ch_h0);
            const unsigned char* ub = smem + ((2 * Tn + 1) % QRING) * QU + b_row + (SET == 0 ? ch_h1 : ch_h0);
            const int urefill = SET == 1 ? 2 * (T + 2) + 1 : 2 * (T + 2);        // odd step 2 T + 1: W(T + 2); even step 2 T' (T' = T): A(T' + 2) ... see header (step 2 T + 2 issues A(T + 3))
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int q = 4 * i; q < 4 * i + 4; ++q) {
                    const int mt = q / 8, nt = q % 8;
                    if constexpr (VAR & 16) asm volatile("" :: "v"(bf[SET][nt]), "v"(af[SET][mt]));
                    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[mt][nt]) : "v"(bf[SET][nt]), "v"(af[SET][mt]));
                }
                if (i < 8) af[SET ^ 1][i] = *(const bf16x8*)(ua + i * 2048);
                else bf[SET ^ 1][i - 8] = *(const bf16x8*)(ub + (i - 8) * 2048);
                if constexpr (!(VAR & 1)) {
                    // 8 pieces per step, one every other MFMA group; step 0 of a tile issues nothing (A(2) went out with the prologue)
                    if ((i & 1) == 1 && s > 0) stage_unit(urefill, i >> 1, (i >> 1) + 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int s = 0; s < nsteps; s += 2) {
            step(std::integral_constant<int, 0>{}, s);
            step(std::integral_constant<int, 1>{}, s + 1);
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15" ::: "memory");

        // ---- epilogue (generic): lane holds, for row m = .. + mt * 16 + (lane & 15), columns nt * 16 + 4 (lane >> 4) .. + 3 ----
        int lane = lane_m;
        asm volatile("" : "+v"(lane));
        const bf16_t* bias = p.bias ? (const bf16_t*)p.bias + (int64_t)g * p.bias_gstride : nullptr;
        const TileSplit ts = tile_split<EPI>(p, n0);
        float bv[8][4];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int64_t n = n0 + wc * 128 + nt * 16 + (lane >> 4) * 4;
            load_bias4(n < N ? bias : nullptr, n, bv[nt]);
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int64_t m = m0 + wr * 128 + mt * 16 + (lane & 15);
            const bool row_ok = m < M;
            RowCtx rc = row_ctx<EPI>(p, g, (unsigned)(row_ok ? m : M - 1));
            rc.coff += ts.cshift;
#pragma unroll
            for (int np = 0; np < 4; ++np) {
                if (EPI == UG_EPI_BIAS_GELU && !ts.gelu)
                    epi_store_pair16<UG_EPI_BIAS>(p, rc, row_ok, n0 + wc * 128 + np * 32, N, lane, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
                else
                    epi_store_pair16<EPI>(p, rc, row_ok, n0 + wc * 128 + np * 32, N, lane, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
            }
        }
    }
}

// =====================================================================================================================
// Round 4: the same one-wave-per-SIMD structure with the instruction economy of the vendor's hand-written kernel (hipBLASLt
// Custom_Cijk_..._MT256x256x64_MI16x16x1: 128 MFMAs, 32 ds_read_b128, 16 buffer_load ... lds, 3 barriers, 4 waits and TWO VALU instructions per
// K-tile and wave - profiles/r04x_*): gemm_pwg64_kernel above spends 47 VALU and ~60 scalar instructions per K-tile on ring-slot arithmetic
// (slot = unit % 5 at run time) and 64-bit DMA addresses. Here
//   * the ring is TWO K-tiles deep (A | W of tile parity 0, A | W of parity 1: 128 KiB) and the K loop is unrolled by two, so every LDS address is
//     a loop-invariant lane offset plus an immediate;
//   * the DMAs are buffer_load_dwordx4 ... offen lds: one resource per operand, ONE loop-invariant per-lane byte offset, the K-tile / piece offset
//     in an SGPR, the destination in M0 - no VALU;
//   * K-tile T + 2 is requested into parity (T & 1) during steps (T, 1) and (T + 1, 0), right after the barrier on top of step (T, 1) has released
//     that parity's slots (every wave's fragments of (T, 1) are in registers), and is waited for on top of step (T + 1, 1).
// Same fragments, same MFMA order per accumulator as gemm_pwg64_kernel: bit-identical results. Whole tiles, generic epilogue (measurement build).
// =====================================================================================================================
struct Pwg2Tile { int g; int64_t m0, n0; int vo_a, vo_b; const bf16_t* ab; const bf16_t* wb; };     // per-tile staging parameters of gemm_pwg2_kernel
template <int EPI, int VAR = 0>      // VAR bit 0: the next K-tile's wait + barrier in the MIDDLE of the odd step (1.25 K-tiles of DMA lead); bit 1: no epilogue
                                     // (timing only); bit 2: the generic epilogue and no cross-tile prefetch (the first build of this kernel)
__global__ __launch_bounds__(256, 1) void gemm_pwg2_kernel(const ug_gemm_desc p, const int tiles_per_group, const int total_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t M = p.M, N = p.N;
    const int nM = (int)((M + 255) / 256), nN = (int)((N + 255) / 256);
    const int nkt = (int)(p.K / 64);                 // >= 4, even (launcher)
    using lds_ptr = __attribute__((address_space(3))) void*;
    constexpr auto P0 = std::integral_constant<int, 0>{}; constexpr auto P1 = std::integral_constant<int, 1>{};
    constexpr bool RES = EPI == UG_EPI_RES_GATE || EPI == UG_EPI_RES_SCALE;
    constexpr int EPI_A = EPI == UG_EPI_QKV_ROPE ? UG_EPI_BIAS_GELU : EPI;      // what a tile outside the q | k columns runs
    constexpr bool FASTEPI = !(VAR & 4);
    // full-tile epilogue conditions that do not depend on the tile (the launcher admits whole tiles only): 16-byte granularity, row maps that never split a tile
    const bool fast_ok = FASTEPI && p.N % 8 == 0 && p.ldc % 8 == 0 && p.c_gstride % 8 == 0 && p.c_rpb % 256 == 0 && (!RES || (p.ldr % 8 == 0 && p.r_gstride % 8 == 0 && p.r_rpb % 256 == 0));

    // per-tile staging parameters: buffer resources over the group's operands, this lane's byte offset of piece 0 of K-tile 0 (wave w stages rows
    // [64 w, 64 w + 64) of a unit, 8 rows = 1 KiB per piece)
    auto params = [&](int tile) __attribute__((always_inline)) {
        Pwg2Tile t;
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        t.g = tile / tiles_per_group;
        const TileCoord tc = tile_of_block(tile - t.g * tiles_per_group, nM, nN, 4);
        t.m0 = (int64_t)tc.tm * 256; t.n0 = (int64_t)tc.tn * 256;
        const bf16_t* const Ab = (const bf16_t*)p.A + (int64_t)t.g * p.a_gstride;
        const bf16_t* const Wb = (const bf16_t*)p.W + (int64_t)t.g * p.w_gstride;
        t.ab = Ab; t.wb = Wb;
        const int row = wave * 64 + (lane_m >> 3);
        const int c = (lane_m & 7) ^ (row & 7);
        t.vo_a = (int)(((int64_t)rowmap32((unsigned)(t.m0 + row), (unsigned)p.a_rpb, (unsigned)p.a_bstride) * p.lda + c * 8) * 2);
        t.vo_b = (int)(((t.n0 + row) * p.ldw + c * 8) * 2);
        return t;
    };
    const int a_pc = (int)(8 * p.lda * 2), b_pc = (int)(8 * p.ldw * 2);        // bytes between consecutive pieces
    // pieces [pc0, pc1) of unit (parity PAR, operand OP) of K-tile T of tile t
    auto dma = [&](const Pwg2Tile& t, auto par_c, auto op_c, int T, int pc0, int pc1) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value, OP = decltype(op_c)::value;
        unsigned char* dst = smem + (2 * PAR + OP) * QU + wave * 64 * 128;
        // K-tiles past the end (the branch-free loop body requests two per tile pair regardless): an offset beyond the resource's range - the buffer
        // unit answers such a piece with zeros at once, no memory traffic, so the drain behind the loop does not wait out a memory latency for data
        // nobody reads (the first build re-read the last K-tile instead: ~1.5 us per tile)
        const int so = T < nkt ? T * 128 : 0x7ffffff0;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(OP ? t.wb : t.ab), 0, 0x7fffff00, 0x00020000);
        for (int i = pc0; i < pc1; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)(dst + i * 1024), 16, OP ? t.vo_b : t.vo_a, so + i * (OP ? b_pc : a_pc), 0, 0);
    };
    auto request_first = [&](const Pwg2Tile& t) __attribute__((always_inline)) {      // K-tiles 0 and 1 of a tile: 32 pieces per wave
        dma(t, P0, P0, 0, 0, 8); dma(t, P0, P1, 0, 0, 8); dma(t, P1, P0, 1, 0, 8); dma(t, P1, P1, 1, 0, 8);
    };

    Pwg2Tile cur = params(blockIdx.x);
    bool prefetched = false;             // the previous epilogue requested this tile's K-tiles 0, 1 and left exactly 32 C stores per wave behind them
    for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        int lane_m = lane;
        asm volatile("" : "+v"(lane_m));
        const int frow = lane_m & 15, fch = lane_m >> 4;
        // lane offsets of the fragment reads inside a 32 KiB unit: k-half 0 / 1 (chunk fch / 4 + fch of the lane's row), before tile * 2048
        const int a_h0 = (wr * 128 + frow) * 128 + ((fch ^ (frow & 7)) << 4), a_h1 = (wr * 128 + frow) * 128 + (((4 + fch) ^ (frow & 7)) << 4);
        const int b_h0 = (wc * 128 + frow) * 128 + ((fch ^ (frow & 7)) << 4), b_h1 = (wc * 128 + frow) * 128 + (((4 + fch) ^ (frow & 7)) << 4);
        bf16x8 af[2][8], bf[2][8];
        const bool relax = prefetched;
        if (!prefetched) {
            __builtin_amdgcn_s_barrier();                   // the previous tile's last reads retired (its MFMAs consumed them)
            request_first(cur);
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");   // K-tile 0 landed
        } else {
            asm volatile("s_waitcnt vmcnt(48)" ::: "memory");   // ... with K-tile 1's 16 pieces and the epilogue's 32 stores still allowed in flight
        }
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int t = 0; t < 8; ++t) af[0][t] = *(const bf16x8*)(smem + 0 * QU + a_h0 + t * 2048);
#pragma unroll
        for (int t = 0; t < 8; ++t) bf[0][t] = *(const bf16x8*)(smem + 1 * QU + b_h0 + t * 2048);
        // (zeroed HERE, behind the branchy prologue: initialised ahead of it hipcc carried the 256 zeros through the branch in VGPRs and spilled 65 of them)
        f32x4 acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; asm volatile("" : "+a"(acc[i][j])); }

        // one 32-deep step: 64 MFMAs on fragment set SET; between them the 16 reads of the next step's fragments (unit pair NPAR, k-half NH) and, in the
        // second step of a K-tile, the 16 DMA pieces of K-tile dT into the parity that step's top barrier has just freed (DPAR) - every address a
        // lane constant + an immediate
        auto step = [&](auto set_c, auto npar_c, auto nh_c, auto dpar_c, auto dma_c, int dT, bool rlx) __attribute__((always_inline)) {
            constexpr int SET = decltype(set_c)::value, NPAR = decltype(npar_c)::value, NH = decltype(nh_c)::value;
            constexpr bool DO_DMA = decltype(dma_c)::value != 0;
            const unsigned char* ua = smem + (2 * NPAR) * QU + (NH ? a_h1 : a_h0);
            const unsigned char* ub = smem + (2 * NPAR + 1) * QU + (NH ? b_h1 : b_h0);
            // the vendor kernel's grain: ONE other instruction in the shadow of each MFMA (a 16x16x32 MFMA holds the pipe 16 cycles and the wave's issue
            // 4): read behind the group's first MFMA, DMA behind its second - not both behind four MFMAs issued back to back
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int q = 4 * i; q < 4 * i + 4; ++q) {
                    // consecutive MFMAs share their FIRST source operand, as the vendor's stream does (VAR bit 4: the second, the first build's order)
                    const int mt = (VAR & 16) ? q / 8 : q % 8, nt = (VAR & 16) ? q % 8 : q / 8;       // default: shared FIRST operand (+1.5...+2.5 %); bit 4 restores the first build's order
                    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[mt][nt]) : "v"(bf[SET][nt]), "v"(af[SET][mt]));
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr ((VAR & 1) && DO_DMA) {
                        // odd step, late reads: nothing in groups 0-7; the landed K-tile's wait + barrier before group 8; two reads per group after it
                        if (q == 32) {
                            // everything but this step's own first 8 pieces (and, in a prefetched tile's first odd step, the previous epilogue's 32 stores
                            // that sit between K-tile 1's pieces and them on the in-order counter): the K-tile requested a tile ago
                            if (rlx) asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                            __builtin_amdgcn_sched_barrier(0);
                            __builtin_amdgcn_s_barrier();
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (i >= 8 && (q == 4 * i || q == 4 * i + 2)) {
                            const int r = 2 * (i - 8) + (q == 4 * i ? 0 : 1);
                            if (r < 8) af[SET ^ 1][r] = *(const bf16x8*)(ua + r * 2048);
                            else bf[SET ^ 1][r - 8] = *(const bf16x8*)(ub + (r - 8) * 2048);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else if (q == 4 * i) {
                        if (i < 8) af[SET ^ 1][i] = *(const bf16x8*)(ua + i * 2048);
                        else bf[SET ^ 1][i - 8] = *(const bf16x8*)(ub + (i - 8) * 2048);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (q == 4 * i + 1) {
                        if constexpr (DO_DMA && !(VAR & 8)) { if (i < 8) dma(cur, dpar_c, P0, dT, i, i + 1); else dma(cur, dpar_c, P1, dT, i - 8, i - 7); }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        };
        // K-tile pair (T, T + 1), T even: parities 0, 1. K-tile T + 2 is requested in step (T, 1), one whole K-tile before its first read.
        for (int T = 0; T < nkt; T += 2) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            step(P0, P0, P1, P0, P0, 0, false);              // (T, 0): reads (T, 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (!(VAR & 1)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // K-tile T + 1 landed (this wave's pieces; the barrier makes it everybody's)
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();                   // parity 0 free (every wave holds its (T, 1) fragments); parity 1 visible
            __builtin_amdgcn_sched_barrier(0);
            step(P1, P1, P0, P0, P1, T + 2, relax && T == 0);   // (T, 1): reads (T + 1, 0); DMA K-tile T + 2 into parity 0
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            step(P0, P1, P1, P0, P0, 0, false);              // (T + 1, 0): reads (T + 1, 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (!(VAR & 1)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // K-tile T + 2 landed
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();                   // parity 1 free; parity 0 (K-tile T + 2) visible
            __builtin_amdgcn_sched_barrier(0);
            step(P1, P0, P0, P1, P1, T + 3, false);   // (T + 1, 1): reads (T + 2, 0) (past the end: stale, never used); DMA K-tile T + 3 into parity 1
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15" ::: "memory");

        const int g = cur.g;
        const int64_t m0 = cur.m0, n0 = cur.n0;
        prefetched = false;
        if constexpr (VAR & 2) { asm volatile("" :: "a"(acc[0][0]), "a"(acc[7][7])); if (tile + (int)gridDim.x < total_tiles) cur = params(tile + gridDim.x); continue; }      // timing only: no epilogue
        int lane_e = lane_m;
        asm volatile("" : "+v"(lane_e));
        const TileSplit ts = tile_split<EPI>(p, n0);
        bool fast = fast_ok;
        unsigned sample = 0;
        if constexpr (EPI == UG_EPI_RES_GATE) {
            sample = (unsigned)m0 / (unsigned)p.rows_per_sample;
            fast = fast && ((unsigned)m0 + 255u) / (unsigned)p.rows_per_sample == sample;
        }
        if (fast) {
            // ---- full-tile epilogue (round 4), the product kernel's whole-line scheme on this kernel's accumulator layout. Lane (r = lane & 15, lg = lane >> 4)
            // holds, per 16-row block mt and 16-column tile nt, columns nt * 16 + 4 lg .. + 3 of row mt * 16 + r. epi_chunk_full pairs two tiles into this
            // lane's 16-byte chunk of a 64-byte half-line (columns (lg & 1) * 16 + 8 (lg >> 1) .. + 7 of the pair); a 128-byte line = tiles 4 L .. 4 L + 3
            // = halves (4 L, 4 L + 1), (4 L + 2, 4 L + 3); lanes r and r ^ 8 trade halves through DPP row_ror:8, so every store (and residual load) covers
            // 8 rows x 128 contiguous bytes. Order on the in-order VM counter: bias / gate / ALL residual chunks (32 x 16 bytes per lane: the K loop's 128
            // fragment registers are dead) -> the next tile's first 32 DMA pieces -> the 32 C stores: no wait of this epilogue depends on the DMAs, and
            // the next tile's first waits allow for exactly 32 stores.
            const int lg = lane_e >> 4, r16 = lane_e & 15;
            const int colc = (int)n0 + wc * 128 + (lg & 1) * 16 + 8 * (lg >> 1);        // this lane's chunk column inside half 0 of line 0
            bf16_t* const Cb = (bf16_t*)p.C + (int64_t)g * p.c_gstride + colc + ts.cshift;
            const int rl = wr * 128 + (r16 & 7);                                        // store / load A row of this lane inside block mt = 0
            bf16_t* const c_laneA = Cb + (int64_t)(rowmap32((unsigned)m0, (unsigned)p.c_rpb, (unsigned)p.c_bstride) + (unsigned)rl) * p.ldc + (r16 >> 3) * 32;
            const int dB = 8 * (int)p.ldc + (r16 < 8 ? 32 : -32);
            float fb[8][4], fg[8][4];
            {
                const bf16_t* bias = p.bias ? (const bf16_t*)p.bias + (int64_t)g * p.bias_gstride : nullptr;
                const bf16_t* gate = nullptr;
                if constexpr (EPI == UG_EPI_RES_GATE) gate = (const bf16_t*)p.gate + (int64_t)g * p.gate_gstride + (int64_t)sample * p.gate_ld;
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) {
                    const int64_t n = n0 + wc * 128 + nt * 16 + lg * 4;
                    u32x2 pb = (u32x2){0u, 0u}, pg = (u32x2){0u, 0u};
                    if (bias) pb = *(const u32x2*)(bias + n);
                    if constexpr (EPI == UG_EPI_RES_GATE) pg = *(const u32x2*)(gate + n);
                    fb[nt][0] = bflo(pb.x); fb[nt][1] = bfhi(pb.x); fb[nt][2] = bflo(pb.y); fb[nt][3] = bfhi(pb.y);
                    fg[nt][0] = bflo(pg.x); fg[nt][1] = bfhi(pg.x); fg[nt][2] = bflo(pg.y); fg[nt][3] = bfhi(pg.y);
                }
            }
            if constexpr (EPI == UG_EPI_QKV_ROPE) {
                if (n0 < p.qk_until_n) {
                    // ---- q | k tile (head width 128): on this layout a head IS one wave's 128 columns, so the RMSNorm row sum needs no LDS and no other wave -
                    // 32 values per lane, then the four lane groups of the row by permlane swaps (sum_row_groups). Per 16-row block: v = bf16(acc + bias),
                    // rs = rsqrt(mean v^2 + eps), x = bf16(bf16(v rs) w), rotation pairs (x0, x1), (x2, x3) by this lane's (cos, sin) pairs of the row's
                    // position, then the whole-line stores of the generic path. Rounding points as gemm256_kernel's q | k epilogue: same bits.
                    const bf16_t* const wsel = (const bf16_t*)(2 * n0 >= p.qk_until_n ? p.qk_wk : p.qk_wq);
                    float fw[8][4];
#pragma unroll
                    for (int nt = 0; nt < 8; ++nt) {
                        const u32x2 pw = *(const u32x2*)(wsel + nt * 16 + lg * 4);
                        fw[nt][0] = bflo(pw.x); fw[nt][1] = bfhi(pw.x); fw[nt][2] = bflo(pw.y); fw[nt][3] = bfhi(pw.y);
                    }
                    unsigned rpb = (unsigned)p.rope_rpb;
                    asm volatile("" : "+s"(rpb));
                    const unsigned wrap = rpb ? rpb : 0xffffffffu;
                    const unsigned mrow = (unsigned)m0 + wr * 128 + r16;
                    const unsigned rr0 = rpb ? mrow % rpb : mrow;
                    const float* const csb = p.rope_cs + lg * 4;
                    __builtin_amdgcn_sched_barrier(0);
                    if (tile + (int)gridDim.x < total_tiles) {
                        cur = params(tile + gridDim.x);
                        __builtin_amdgcn_s_barrier();
                        request_first(cur);
                        prefetched = true;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    u32x4 cbuf[2][8];
                    auto open_rows = [&](int mt) __attribute__((always_inline)) {
                        unsigned rr = rr0 + mt * 16;
                        if (rr >= wrap) rr -= wrap;
                        const float* q = csb + ((int64_t)p.rope_pos0 + rr) * 128;
                        cbuf[mt & 1][0] = gload16_asm(q);
                        asm volatile("global_load_dwordx4 %0, %1, off offset:64" : "=v"(cbuf[mt & 1][1]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:128" : "=v"(cbuf[mt & 1][2]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:192" : "=v"(cbuf[mt & 1][3]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:256" : "=v"(cbuf[mt & 1][4]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:320" : "=v"(cbuf[mt & 1][5]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:384" : "=v"(cbuf[mt & 1][6]) : "v"(q) : "memory");
                        asm volatile("global_load_dwordx4 %0, %1, off offset:448" : "=v"(cbuf[mt & 1][7]) : "v"(q) : "memory");
                    };
                    open_rows(0);
#pragma unroll
                    for (int mt = 0; mt < 8; ++mt) {
                        if (mt + 1 < 8) open_rows(mt + 1);
                        // younger than this block's 8 loads on the in-order counter: the next block's 8 loads and the previous block's 4 stores
                        if (mt == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                        else if (mt == 7) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
#pragma unroll
                        for (int t8 = 0; t8 < 8; ++t8) asm volatile("" : "+v"(cbuf[mt & 1][t8]));
                        float ss = 0.f;
                        float v[8][4];
#pragma unroll
                        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
                            for (int q = 0; q < 4; q += 2) {
                                float v0 = acc[mt][nt][q] + fb[nt][q], v1 = acc[mt][nt][q + 1] + fb[nt][q + 1];
                                rbf2(v0, v1);
                                v[nt][q] = v0; v[nt][q + 1] = v1;
                                ss += v0 * v0; ss += v1 * v1;
                            }
                        const float tot = sum_row_groups(ss);
                        const float rs = __builtin_amdgcn_rsqf(tot * (1.0f / 128.0f) + p.qk_eps);
                        u32x4 o[4];               // the four 64-byte halves of the row's two lines: tiles (0, 1), (2, 3) | (4, 5), (6, 7)
#pragma unroll
                        for (int pr = 0; pr < 4; ++pr) {
                            unsigned pk[2][2];
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                const int nt = 2 * pr + e;
                                const u32x4 cs = cbuf[mt & 1][nt];
                                const float c0 = __builtin_bit_cast(float, (unsigned)cs.x), s0 = __builtin_bit_cast(float, (unsigned)cs.y);
                                const float c1 = __builtin_bit_cast(float, (unsigned)cs.z), s1 = __builtin_bit_cast(float, (unsigned)cs.w);
                                float x[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q) x[q] = v[nt][q] * rs;
                                rbf2(x[0], x[1]); rbf2(x[2], x[3]);
#pragma unroll
                                for (int q = 0; q < 4; ++q) x[q] = x[q] * fw[nt][q];
                                rbf2(x[0], x[1]); rbf2(x[2], x[3]);
                                pk[e][0] = pack2bf(x[0] * c0 + (-x[1]) * s0, x[1] * c0 + x[0] * s0);
                                pk[e][1] = pack2bf(x[2] * c1 + (-x[3]) * s1, x[3] * c1 + x[2] * s1);
                            }
                            swap16(pk[0][0], pk[1][0]); swap16(pk[0][1], pk[1][1]);
                            o[pr].x = pk[0][0]; o[pr].y = pk[0][1]; o[pr].z = pk[1][0]; o[pr].w = pk[1][1];
                        }
#pragma unroll
                        for (int L = 0; L < 2; ++L) {
                            u32x4 xa, xb;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                xa[q] = (unsigned)__builtin_amdgcn_update_dpp((int)o[2 * L][q], (int)o[2 * L + 1][q], 0x128, 0xF, 0xC, false);
                                xb[q] = (unsigned)__builtin_amdgcn_update_dpp((int)o[2 * L][q], (int)o[2 * L + 1][q], 0x128, 0xF, 0x3, false);
                            }
                            bf16_t* cp = c_laneA + (int64_t)(mt * 16) * p.ldc + L * 64;
                            __builtin_nontemporal_store(xa, (u32x4*)cp);
                            __builtin_nontemporal_store(xb, (u32x4*)(cp + dB));
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    continue;
                }
            }
            u32x4 rbuf[16][2];            // residual: load A / load B of row-line group (mt, L) = 2 mt + L
            if constexpr (RES) {
                const bf16_t* const Rb = (const bf16_t*)p.R + (int64_t)g * p.r_gstride + colc;
                const bf16_t* const r_laneA = Rb + (int64_t)(rowmap32((unsigned)m0, (unsigned)p.r_rpb, (unsigned)p.r_bstride) + (unsigned)rl) * p.ldr + (r16 >> 3) * 32;
                const int dBr = 8 * (int)p.ldr + (r16 < 8 ? 32 : -32);
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    const bf16_t* rp = r_laneA + (int64_t)((rg >> 1) * 16) * p.ldr + (rg & 1) * 64;
                    rbuf[rg][0] = gload16_asm(rp);
                    rbuf[rg][1] = gload16_asm(rp + dBr);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (tile + (int)gridDim.x < total_tiles) {
                cur = params(tile + gridDim.x);
                __builtin_amdgcn_s_barrier();               // every wave's last LDS reads retired (their MFMAs consumed them: s_nop above): the ring is free
                request_first(cur);
                prefetched = true;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                const int mt = rg >> 1, L = rg & 1;
                u32x4 res_own[2] = {(u32x4){0u, 0u, 0u, 0u}, (u32x4){0u, 0u, 0u, 0u}};
                if constexpr (RES) {
                    // younger than this group's two loads: the later groups' loads, the 32 DMA pieces (when requested) and the stores so far
                    if (rg == 0) { if (prefetched) asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int la = (int)rbuf[rg][0][q], lb = (int)rbuf[rg][1][q];
                        res_own[0][q] = (unsigned)__builtin_amdgcn_update_dpp(la, lb, 0xE4, 0xF, 0xC, false);
                        const int z = __builtin_amdgcn_update_dpp(lb, la, 0xE4, 0xF, 0xC, false);
                        res_own[1][q] = (unsigned)__builtin_amdgcn_update_dpp(z, z, 0x128, 0xF, 0xF, false);
                    }
                }
                u32x4 o[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int nt = 4 * L + 2 * hh;
                    o[hh] = (EPI_A == UG_EPI_BIAS_GELU && !ts.gelu)
                        ? epi_chunk_full<UG_EPI_BIAS>(p.alpha, acc[mt][nt], acc[mt][nt + 1], fb[nt], fb[nt + 1], fg[nt], fg[nt + 1], res_own[hh])
                        : epi_chunk_full<EPI_A>(p.alpha, acc[mt][nt], acc[mt][nt + 1], fb[nt], fb[nt + 1], fg[nt], fg[nt + 1], res_own[hh]);
                }
                u32x4 xa, xb;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    xa[q] = (unsigned)__builtin_amdgcn_update_dpp((int)o[0][q], (int)o[1][q], 0x128, 0xF, 0xC, false);
                    xb[q] = (unsigned)__builtin_amdgcn_update_dpp((int)o[0][q], (int)o[1][q], 0x128, 0xF, 0x3, false);
                }
                bf16_t* cp = c_laneA + (int64_t)(mt * 16) * p.ldc + L * 64;
                __builtin_nontemporal_store(xa, (u32x4*)cp);
                __builtin_nontemporal_store(xb, (u32x4*)(cp + dB));
                __builtin_amdgcn_sched_barrier(0);          // one row-line group at a time: hoisting the accumulator reads of later groups spilled 65 registers
            }
            continue;
        }
        // ---- generic epilogue: lane holds, for row m = .. + mt * 16 + (lane & 15), columns nt * 16 + 4 (lane >> 4) .. + 3 ----
        if (tile + (int)gridDim.x < total_tiles) cur = params(tile + gridDim.x);
        const bf16_t* bias = p.bias ? (const bf16_t*)p.bias + (int64_t)g * p.bias_gstride : nullptr;
        float bv[8][4];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int64_t n = n0 + wc * 128 + nt * 16 + (lane_e >> 4) * 4;
            load_bias4(n < N ? bias : nullptr, n, bv[nt]);
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int64_t m = m0 + wr * 128 + mt * 16 + (lane_e & 15);
            const bool row_ok = m < M;
            RowCtx rc = row_ctx<EPI_A>(p, g, (unsigned)(row_ok ? m : M - 1));
            rc.coff += ts.cshift;
#pragma unroll
            for (int np = 0; np < 4; ++np) {
                if (EPI_A == UG_EPI_BIAS_GELU && !ts.gelu)
                    epi_store_pair16<UG_EPI_BIAS>(p, rc, row_ok, n0 + wc * 128 + np * 32, N, lane_e, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
                else
                    epi_store_pair16<EPI_A>(p, rc, row_ok, n0 + wc * 128 + np * 32, N, lane_e, acc[mt][2 * np], acc[mt][2 * np + 1], bv[2 * np], bv[2 * np + 1]);
            }
        }
    }
}

template <int EPI, int VAR = 0>
int launch_pwg2_t(const ug_gemm_desc& d, hipStream_t s) {
    constexpr int PLDS = 4 * QU;
    const int groups = d.groups > 0 ? d.groups : 1;
    const int64_t t256 = ((d.M + 255) / 256) * ((d.N + 255) / 256) * groups;
    UG_REQUIRE(d.K % 128 == 0 && d.K >= 256 && d.M % 256 == 0 && d.N % 256 == 0 && d.a_rpb % 256 == 0, UG_ERR_UNSUPPORTED,
               "ug_gemm_bf16(pwg2): whole 256^2 tiles only, K a multiple of 128 and >= 256 (M=%lld N=%lld K=%lld)", (long long)d.M, (long long)d.N, (long long)d.K);
    UG_REQUIRE((double)d.M * d.lda * 2 < 4.0e9 && (double)d.N * d.ldw * 2 < 4.0e9, UG_ERR_UNSUPPORTED, "ug_gemm_bf16(pwg2): operands beyond 32-bit byte offsets");
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)gemm_pwg2_kernel<EPI, VAR>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
        attr_set = true;
    }
    static int ncu = 0;
    if (ncu == 0) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
        if (ncu <= 0) ncu = 256;
    }
    const int total = (int)t256;
    dim3 grid((unsigned)(total < ncu ? total : ncu), 1, 1);
    hipLaunchKernelGGL((gemm_pwg2_kernel<EPI, VAR>), grid, dim3(256), PLDS, s, d, (int)(t256 / groups), total);
    UG_CHECK_LAUNCH("ug_gemm_bf16(pwg2)");
    return UG_OK;
}

template <int EPI, int VAR>
int launch_pwg64_t(const ug_gemm_desc& d, hipStream_t s) {
    constexpr int PLDS = QRING * QU;
    const int groups = d.groups > 0 ? d.groups : 1;
    const int64_t t256 = ((d.M + 255) / 256) * ((d.N + 255) / 256) * groups;
    UG_REQUIRE(d.K % 64 == 0 && d.K >= 192 && d.M % 256 == 0 && d.N % 256 == 0 && d.a_rpb % 256 == 0, UG_ERR_UNSUPPORTED,
               "ug_gemm_bf16(pwg64): whole 256^2 tiles only, K a multiple of 64 and >= 192 (M=%lld N=%lld K=%lld)", (long long)d.M, (long long)d.N, (long long)d.K);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)gemm_pwg64_kernel<EPI, VAR>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
        attr_set = true;
    }
    static int ncu = 0;
    if (ncu == 0) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
        if (ncu <= 0) ncu = 256;
    }
    const int total = (int)t256;
    dim3 grid((unsigned)(total < ncu ? total : ncu), 1, 1);
    hipLaunchKernelGGL((gemm_pwg64_kernel<EPI, VAR>), grid, dim3(256), PLDS, s, d, (int)(t256 / groups), total);
    UG_CHECK_LAUNCH("ug_gemm_bf16(pwg64)");
    return UG_OK;
}

template <int EPI, int NW, int VAR, int PRING = 4>
int launch_pwg_t(const ug_gemm_desc& d, hipStream_t s) {
    constexpr int PLDS = PRING * PSLOT;
    const int groups = d.groups > 0 ? d.groups : 1;
    const int64_t t256 = ((d.M + 255) / 256) * ((d.N + 255) / 256) * groups;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)gemm_pwg_kernel<EPI, NW, VAR, PRING>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
        attr_set = true;
    }
    static int ncu = 0;
    if (ncu == 0) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
        if (ncu <= 0) ncu = 256;
    }
    const int total = (int)t256;
    dim3 grid((unsigned)(total < ncu ? total : ncu), 1, 1);
    hipLaunchKernelGGL((gemm_pwg_kernel<EPI, NW, VAR, PRING>), grid, dim3(64 * NW), PLDS, s, d, (int)(t256 / groups), total);
    UG_CHECK_LAUNCH("ug_gemm_bf16(pwg)");
    return UG_OK;
}

}  // namespace

// UG_GEMM_PWG=4 and the fused q/k RMSNorm + RoPE launch (head width 128, with RoPE): called by gemm.hip's gemm_launch in the probe build
int ug_gemm_launch_pwg2_qkrope(const ug_gemm_desc& d, hipStream_t s) {
    return launch_pwg2_t<UG_EPI_QKV_ROPE, 1>(d, s);
}

// Called by gemm.hip's dispatcher for shapes the 256^2 tiles fill (no LoRA segment, 16-byte epilogue granularity, not UG_EPI_F32).
// mode (UG_GEMM_PWG): 1 = one wave per SIMD, 2 = two waves per SIMD.
int ug_gemm_launch_pwg(const ug_gemm_desc& d, hipStream_t s) {
    const int mode = ug_env_int("UG_GEMM_PWG", 0);
    const int var = ug_env_int("UG_PWG_VAR", 0);
    if (mode == 4) {                  // round 4: two-K-tile ring, unrolled, buffer-form DMAs, full-tile epilogue + cross-tile prefetch (gemm_pwg2_kernel)
#define UG_PWG2_CASE(E)                                                                                                    \
    case E: return var == 3 ? launch_pwg2_t<E, 3>(d, s) : var == 5 ? launch_pwg2_t<E, 5>(d, s) : var == 0 ? launch_pwg2_t<E, 0>(d, s) : var == 11 ? launch_pwg2_t<E, 11>(d, s) : var == 17 ? launch_pwg2_t<E, 17>(d, s) : launch_pwg2_t<E, 1>(d, s);
        switch (d.epilogue) {
            UG_PWG2_CASE(UG_EPI_BIAS)
            UG_PWG2_CASE(UG_EPI_BIAS_GELU)
            UG_PWG2_CASE(UG_EPI_RES_GATE)
            UG_PWG2_CASE(UG_EPI_RES_SCALE)
            default: UG_FAIL(UG_ERR_UNSUPPORTED, "ug_gemm_bf16(pwg2): epilogue %d", d.epilogue);
        }
#undef UG_PWG2_CASE
    }
    if (mode == 3) {                  // round 3: whole-line (64-deep ring units) one-wave-per-SIMD kernel; var 1 = no DMA, 16 = no MFMA (timing only)
        switch (d.epilogue) {
            case UG_EPI_BIAS: return var == 1 ? launch_pwg64_t<UG_EPI_BIAS, 1>(d, s) : var == 16 ? launch_pwg64_t<UG_EPI_BIAS, 16>(d, s) :
                                     var == 2 ? launch_pwg64_t<UG_EPI_BIAS, 2>(d, s) : launch_pwg64_t<UG_EPI_BIAS, 0>(d, s);
            case UG_EPI_BIAS_GELU: return launch_pwg64_t<UG_EPI_BIAS_GELU, 0>(d, s);
            case UG_EPI_RES_GATE: return launch_pwg64_t<UG_EPI_RES_GATE, 0>(d, s);
            case UG_EPI_RES_SCALE: return launch_pwg64_t<UG_EPI_RES_SCALE, 0>(d, s);
            default: UG_FAIL(UG_ERR_UNSUPPORTED, "ug_gemm_bf16(pwg64): epilogue %d", d.epilogue);
        }
    }
#define UG_PWG_CASE(E)                                                                            \
    case E:                                                                                       \
        if (mode == 2) return var == 2 ? launch_pwg_t<E, 8, 2>(d, s) : launch_pwg_t<E, 8, 0>(d, s);   \
        return launch_pwg_t<E, 4, 0>(d, s);
    switch (d.epilogue) {
        case UG_EPI_BIAS:
            if (mode == 1 && var >= 100) {        // ring-depth probes: var = 100 * slots + (16: DMA only | 0: full kernel)
                if (var == 216) return launch_pwg_t<UG_EPI_BIAS, 4, 16, 2>(d, s);
                if (var == 316) return launch_pwg_t<UG_EPI_BIAS, 4, 16, 3>(d, s);
                if (var == 516) return launch_pwg_t<UG_EPI_BIAS, 4, 16, 5>(d, s);
                if (var == 300) return launch_pwg_t<UG_EPI_BIAS, 4, 0, 3>(d, s);
                if (var == 500) return launch_pwg_t<UG_EPI_BIAS, 4, 0, 5>(d, s);
            }
            if (mode == 2 && var == 32) return launch_pwg_t<UG_EPI_BIAS, 8, 32>(d, s);
            if (mode == 2 && var == 33) return launch_pwg_t<UG_EPI_BIAS, 8, 33>(d, s);
            if (mode == 2) return var == 1 ? launch_pwg_t<UG_EPI_BIAS, 8, 1>(d, s) : var == 2 ? launch_pwg_t<UG_EPI_BIAS, 8, 2>(d, s) :
                                  var == 4 ? launch_pwg_t<UG_EPI_BIAS, 8, 4>(d, s) : var == 6 ? launch_pwg_t<UG_EPI_BIAS, 8, 6>(d, s) : launch_pwg_t<UG_EPI_BIAS, 8, 0>(d, s);
            return var == 1 ? launch_pwg_t<UG_EPI_BIAS, 4, 1>(d, s) : var == 4 ? launch_pwg_t<UG_EPI_BIAS, 4, 4>(d, s) : var == 5 ? launch_pwg_t<UG_EPI_BIAS, 4, 5>(d, s) :
                   var == 8 ? launch_pwg_t<UG_EPI_BIAS, 4, 8>(d, s) : var == 16 ? launch_pwg_t<UG_EPI_BIAS, 4, 16>(d, s) : launch_pwg_t<UG_EPI_BIAS, 4, 0>(d, s);
        UG_PWG_CASE(UG_EPI_BIAS_GELU)
        UG_PWG_CASE(UG_EPI_RES_GATE)
        UG_PWG_CASE(UG_EPI_RES_SCALE)
        default: UG_FAIL(UG_ERR_UNSUPPORTED, "ug_gemm_bf16(pwg): epilogue %d", d.epilogue);
    }
#undef UG_PWG_CASE
}
