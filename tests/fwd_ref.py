"""CPU float64 references of the forward projection kernels: the stand-alone q/k RMSNorm + RoPE pass (ug_qk_rmsnorm_rope), the GEMM's fused
q/k epilogue (UG_EPI_QKV_ROPE), the GEMM with a LoRA K-segment under every epilogue and (second half: flat buffers, sampled rows, the dispatcher's
path restated) the base GEMM, AdaLN modulate and the small linear of tests/test_fuzz_gemm_gpu.py.

Every function takes the operands exactly as the kernel sees them (bf16 or fp32 values, here widened to float64; the buffers and row maps of
the C ABI) and returns two whole output buffers: the exact result (nothing rounded) and a rounding-point variant that rounds to bf16 where the
kernel and diffusers round - the Linear's output bf16(acc + bias) (LoRA inside acc); RMSNorm as bf16(x rs), then bf16(. w); RoPE in fp32; every
store. Elements the call does not write hold the input buffer's values in both. tests/test_fwd_ref_cpu.py checks these functions against the
oracle's formulations in float64; the GPU sweep (tests/test_fuzz_forward_gpu.py) bounds a kernel by 1.5 x the variant's own error."""
import math

import torch

from tests.bwd_ref import F64, bf16, bf16_ulp, err  # noqa: F401  (re-exported for the sweeps)

EPI_BIAS, EPI_BIAS_GELU, EPI_RES_GATE, EPI_RES_SCALE = 0, 1, 2, 3        # include/unigen_hip.h
_K0 = math.sqrt(2.0 / math.pi)


def rowmap(m: torch.Tensor, rpb: int, bstride: int) -> torch.Tensor:
    """logical rows -> physical rows of a (rows per batch, batch stride) row map; rpb 0: identity"""
    return m if rpb == 0 else (m // rpb) * bstride + m % rpb


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    """F.gelu(approximate="tanh") in the sigmoid form: 0.5 x (1 + tanh u) = x sigmoid(2u), no cancellation below x = -5"""
    return x * torch.sigmoid(2.0 * _K0 * (x + 0.044715 * x ** 3))


def _rope(x, cos, sin):
    """pair rotation y[2i] = x[2i] cos[2i] - x[2i+1] sin[2i], y[2i+1] = x[2i+1] cos[2i+1] + x[2i] sin[2i+1]; cos, sin broadcast over heads"""
    y = torch.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * cos[..., 0::2] - x[..., 1::2] * sin[..., 0::2]
    y[..., 1::2] = x[..., 1::2] * cos[..., 1::2] + x[..., 0::2] * sin[..., 1::2]
    return y


def _qk(x, w, has_w, cos, sin, eps, rnd):
    """x [rows, heads, dh] float64; w [rows, dh] (the weight of each row) where has_w [rows]; cos / sin [rows, dh] or None.
    rnd: round bf16(x rs), bf16(. w), RoPE in fp32, bf16 store."""
    rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    u = x * rs
    if rnd:
        u = bf16(u)
    u = u * w[:, None, :]
    if rnd:
        u = bf16(u)
    u = torch.where(has_w[:, None, None], u, x)
    if cos is not None:
        if rnd:
            u = _rope(u.float(), cos.float()[:, None, :], sin.float()[:, None, :]).to(F64)
        else:
            u = _rope(u, cos.to(F64)[:, None, :], sin.to(F64)[:, None, :])
    return bf16(u) if rnd else u


def _weights(ws, pos, split, dh):
    """(w_a, w_b) either may be None -> per-row weights [rows, dh] and whether a row has one: positions < split take w_a"""
    wa, wb = ws
    side_a = pos < split
    one = torch.ones(dh, dtype=F64)
    w = torch.where(side_a[:, None], (one if wa is None else wa.to(F64))[None, :], (one if wb is None else wb.to(F64))[None, :])
    has = torch.where(side_a, torch.tensor(wa is not None), torch.tensor(wb is not None))
    return w, has


def qk_rmsnorm_rope(buf, *, batches, rows_per_batch, q_off, k_off, heads, dh, batch_stride_rows=None, pos_offset=0, wq_a=None, wk_a=None,
                    wq_b=None, wk_b=None, split=0, cos=None, sin=None, eps=1e-6):
    """ug_qk_rmsnorm_rope on buf [physical rows, ld] (row 0 = batch 0, row 0): row r of batch b sits at physical row b * batch_stride_rows + r,
    position pos_offset + r; positions < split take (wq_a, wk_a), the others (wq_b, wk_b); a None weight: no RMSNorm on that side; cos / sin
    [positions, dh] or None: no RoPE; q_off < 0: k only. Returns (exact, rounding-point variant), float64 copies of buf."""
    bs = rows_per_batch if batch_stride_rows is None else batch_stride_rows
    r = torch.arange(rows_per_batch)
    phys = (torch.arange(batches)[:, None] * bs + r[None, :]).flatten()
    pos = (pos_offset + r).repeat(batches)
    cc = None if cos is None else cos.to(F64)[pos]
    sn = None if sin is None else sin.to(F64)[pos]
    src = buf.to(F64)
    outs = (src.clone(), src.clone())
    for off, ws in ((q_off, (wq_a, wq_b)), (k_off, (wk_a, wk_b))):
        if off < 0:
            continue
        w, has = _weights(ws, pos, split, dh)
        x = src[phys, off:off + heads * dh].reshape(-1, heads, dh)
        for o, rnd in zip(outs, (False, True)):
            o[phys, off:off + heads * dh] = _qk(x, w, has, cc, sn, eps, rnd).reshape(-1, heads * dh)
    return outs


def qk_vectors(buf, phys, q_off, k_off, heads, dh):
    """the head vectors a q/k pass touches: [(q heads +) k heads, rows, dh] of the physical rows phys (the layout fwd_ref.err bounds per vector)"""
    offs = [o for o in (q_off, k_off) if o >= 0]
    t = torch.cat([buf[phys, o:o + heads * dh].reshape(len(phys), heads, dh) for o in offs], 1)
    return t.transpose(0, 1)


def pair_table(cs):
    """(cos, sin) pair table [positions, dh / 2, 2] -> the [positions, dh] cos and sin tables of ug_qk_rmsnorm_rope"""
    cs = cs.to(F64)
    return cs[..., 0].repeat_interleave(2, -1), cs[..., 1].repeat_interleave(2, -1)


def _gather(t, m, rpb, bstride):
    return t.to(F64)[rowmap(m, rpb, bstride)]


def _epilogue(v, epilogue, rnd, cols, *, R=None, gate=None, alpha=1.0, gelu_from_n=0):
    """v = the Linear's output (bf16 in the variant) [M, N]; cols the logical column indices"""
    if epilogue == EPI_BIAS_GELU:
        g = cols >= gelu_from_n
        y = gelu_tanh(v)
        return torch.where(g[None, :], bf16(y) if rnd else y, v)
    if epilogue in (EPI_RES_GATE, EPI_RES_SCALE):
        t = gate * v if epilogue == EPI_RES_GATE else alpha * v
        return bf16(R + bf16(t)) if rnd else R + t
    return v


def _store(out, m, cols, rows_map, c_shift_from_n, c_shift, vals):
    """vals [M, N] -> out at physical row map(m), column n (+ c_shift from c_shift_from_n on)"""
    dst = cols + c_shift * (cols >= c_shift_from_n).long() if c_shift_from_n > 0 else cols
    rows = rowmap(m, *rows_map)
    out[rows[:, None], dst[None, :]] = vals


def lora_gemm(a, w, bias, out, *, M, epilogue=EPI_BIAS, t=None, lb=None, a_map=(0, 0), c_map=(0, 0), residual=None, r_map=(0, 0), gate=None,
              rows_per_sample=0, alpha=1.0, gelu_from_n=0, c_shift_from_n=0, c_shift=0):
    """ug_gemm_bf16: acc[m, n] = A[map(m)] . W[n] + T[m] . B[n] (T rows are logical rows, lb [N, r]); v = acc + bias; then the epilogue
    (GELU from column gelu_from_n, R[map(m)] + gate[m // rows_per_sample] v, R + alpha v) stored at C[map(m)], column n (+ c_shift from
    c_shift_from_n). `out` is the C buffer before the call (R may alias it: pass the same tensor). Returns (exact, variant)."""
    m = torch.arange(M)
    N = w.shape[0]
    cols = torch.arange(N)
    acc = _gather(a, m, *a_map)[:, :w.shape[1]] @ w.to(F64).t()
    if t is not None:
        acc = acc + t.to(F64)[:M, :lb.shape[1]] @ lb.to(F64).t()
    if bias is not None:
        acc = acc + bias.to(F64)[None, :N]
    R = _gather(residual, m, *r_map)[:, :N] if residual is not None else None
    G = gate.to(F64)[m // rows_per_sample][:, :N] if gate is not None else None
    res = []
    for rnd in (False, True):
        v = bf16(acc) if rnd else acc
        y = _epilogue(v, epilogue, rnd, cols, R=R, gate=G, alpha=alpha, gelu_from_n=gelu_from_n)
        o = out.to(F64).clone()
        _store(o, m, cols, c_map, c_shift_from_n, c_shift, y)
        res.append(o)
    return tuple(res)


def qkv_rope_gemm(a, w, bias, out, *, M, wq, wk, cs, rope_rpb, pos0, qk_until_n, dh, eps=1e-6, a_map=(0, 0), c_map=(0, 0), gelu_from_n=0,
                  c_shift_from_n=0, c_shift=0):
    """ug_gemm_bf16 with UG_EPI_QKV_ROPE: v = A W^T + bias; columns [0, qk_until_n / 2) are q heads, [qk_until_n / 2, qk_until_n) k heads of
    width dh: RMSNorm (weights wq / wk) and RoPE with the pair table cs [positions, dh / 2, 2] (None: no RoPE) at position
    pos0 + m % rope_rpb (rope_rpb 0: m); the other columns are v, or GELU(v) from gelu_from_n > 0 on; stored through the C row map and the
    column shift. Returns (exact, variant)."""
    m = torch.arange(M)
    N = w.shape[0]
    cols = torch.arange(N)
    acc = _gather(a, m, *a_map)[:, :w.shape[1]] @ w.to(F64).t()
    if bias is not None:
        acc = acc + bias.to(F64)[None, :N]
    pos = pos0 + (m % rope_rpb if rope_rpb else m)
    cc, sn = pair_table(cs[pos]) if cs is not None else (None, None)
    heads = qk_until_n // 2 // dh
    one = torch.ones(M, dtype=torch.bool)
    res = []
    for rnd in (False, True):
        v = bf16(acc) if rnd else acc
        y = v.clone()
        for c0, wn in ((0, wq), (qk_until_n // 2, wk)):
            x = v[:, c0:c0 + heads * dh].reshape(M, heads, dh)
            y[:, c0:c0 + heads * dh] = _qk(x, wn.to(F64)[None, :].expand(M, dh), one, cc, sn, eps, rnd).reshape(M, heads * dh)
        if gelu_from_n > 0:
            y = _epilogue(y, EPI_BIAS_GELU, rnd, cols, gelu_from_n=gelu_from_n)
        o = out.to(F64).clone()
        _store(o, m, cols, c_map, c_shift_from_n, c_shift, y)
        res.append(o)
    return tuple(res)


# ----------------------------------------------------------------------------------------------------------------------------------
# operands of the forward sweep, shared with the sensitivity checks of tests/test_fwd_ref_cpu.py (which must see the same data)
# ----------------------------------------------------------------------------------------------------------------------------------
def spread_rows(g, rows, cols, zero_row=None):
    """N(0, 1) rows scaled by magnitudes log-uniform in [1e-3, 3e2], one all-zero row (index zero_row, default the middle one); bf16 values"""
    x = torch.randn(rows, cols, generator=g, dtype=F64) * torch.exp(torch.empty(rows, 1, dtype=F64).uniform_(math.log(1e-3), math.log(3e2), generator=g))
    x[rows // 2 if zero_row is None else zero_row] = 0.0
    return bf16(x)


def norm_weights(g, dh):
    """(w_a, w_b) bf16 RMSNorm weights of the two sides that differ by O(1): w_b = -w_a (1 + U[0.2, 1])"""
    wa = 1.0 + 0.5 * torch.randn(dh, generator=g, dtype=F64)
    wb = -wa * (1.0 + torch.empty(dh, dtype=F64).uniform_(0.2, 1.0, generator=g))
    return bf16(wa), bf16(wb)


def rope_tables(g, positions, dh):
    """angles uniform in [0, 2 pi) per (position, pair) -> (cos, sin) [positions, dh] fp32 and the pair table [positions, dh / 2, 2] fp32"""
    ang = torch.rand(positions, dh // 2, generator=g, dtype=F64) * (2.0 * math.pi)
    cs = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()
    cos, sin = pair_table(cs)
    return cos.float().contiguous(), sin.float().contiguous(), cs


def lora_operands(g, M, N, K, r, r_pad=None, cancel=False):
    """A [M, K], W [N, K], bias [N], T [M, r_pad], B [N, r_pad] (bf16 values; rank r zero-padded to r_pad) with |T B^T| ~ |A W^T|.
    cancel (needs r >= K): T[:, :K] = A, B[:, :K] = bf16(-0.98 W) - the LoRA term cancels 98 % of A W^T (the rest of the rank and the bias
    scaled to what is left), so a Linear output rounded to bf16 BEFORE the LoRA term is added is ~50 x further from the truth than one bf16
    rounding of the sum."""
    r_pad = r if r_pad is None else r_pad
    a = bf16(torch.randn(M, K, generator=g, dtype=F64))
    w = bf16(torch.randn(N, K, generator=g, dtype=F64) * K ** -0.5)
    b = bf16(0.1 * torch.randn(N, generator=g, dtype=F64))
    t = torch.zeros(M, r_pad, dtype=F64)
    lb = torch.zeros(N, r_pad, dtype=F64)
    t[:, :r] = bf16(torch.randn(M, r, generator=g, dtype=F64))
    lb[:, :r] = bf16(torch.randn(N, r, generator=g, dtype=F64) * r ** -0.5)
    if cancel:
        assert r >= K, (r, K)
        t[:, :K], lb[:, :K] = a, bf16(-0.98 * w)
        t[:, K:] = bf16(0.02 * t[:, K:])                  # the rest of the rank and the bias at the size of what is left
        b = bf16(0.02 * b)
    return a, w, b, t, lb


# ----------------------------------------------------------------------------------------------------------------------------------
# the base GEMM (no LoRA segment), AdaLN modulate and the small linear: references of tests/test_fuzz_gemm_gpu.py. Operands are the FLAT
# buffers of the C ABI (any device; only the rows asked for are gathered and widened to float64 on the CPU), strides in elements.
# ----------------------------------------------------------------------------------------------------------------------------------
EPI_F32 = 4
F32_TOTAL, F32_ROW, FLOOR = 1e-5, 1e-4, 2.0 ** -9
TILE = 256


def _flat_rows(buf, base, width):
    """buf[base[i] + j], j < width, of a flat buffer -> float64 on the CPU"""
    idx = base[:, None] + torch.arange(width)[None, :]
    return buf.reshape(-1)[idx.to(buf.device)].cpu().to(F64)


def gemm(a, w, bias, *, M, N, K, rows=None, epilogue=EPI_BIAS, lda=None, ldw=None, a_map=(0, 0), residual=None, ldr=0, r_map=(0, 0), gate=None,
         gate_ld=0, rows_per_sample=0, alpha=1.0, groups=1, a_gstride=0, w_gstride=0, bias_gstride=0, r_gstride=0, gate_gstride=0,
         gelu_from_n=0, **_):
    """ug_gemm_bf16 without a LoRA segment on the logical rows `rows` (default: all M) of every group: v = A[g][map(m)] . W[g][n] + bias[g][n];
    UG_EPI_F32: v itself (fp32 out, nothing rounded); else the epilogue on v (GELU from column gelu_from_n, R[g][map(m)] + gate[g][m //
    rows_per_sample] v, R + alpha v with alpha as the fp32 the descriptor carries). Returns (exact, variant) [groups, len(rows), N]: the LOGICAL
    values; gemm_dest gives where the kernel stores them (C row map, column split, group stride)."""
    rows = torch.arange(M) if rows is None else rows
    lda, ldw = lda or K, ldw or K
    cols = torch.arange(N)
    alpha = float(torch.tensor(alpha, dtype=torch.float32))
    ex, va = [], []
    for g in range(max(groups, 1)):
        A = _flat_rows(a, g * a_gstride + rowmap(rows, *a_map) * lda, K)
        W = _flat_rows(w, g * w_gstride + cols * ldw, K)
        acc = A @ W.t()
        if bias is not None:
            acc = acc + _flat_rows(bias, torch.tensor([g * bias_gstride]), N)
        R = G = None
        if epilogue in (EPI_RES_GATE, EPI_RES_SCALE):
            R = _flat_rows(residual, g * r_gstride + rowmap(rows, *r_map) * ldr, N)
        if epilogue == EPI_RES_GATE:
            G = _flat_rows(gate, g * gate_gstride + (rows // rows_per_sample) * gate_ld, N)
        for rnd, dst in ((False, ex), (True, va)):
            v = bf16(acc) if rnd and epilogue != EPI_F32 else acc
            dst.append(_epilogue(v, epilogue, rnd, cols, R=R, gate=G, alpha=alpha, gelu_from_n=gelu_from_n))
    return torch.stack(ex), torch.stack(va)


def gemm_dest(rows, *, N, ldc, c_map=(0, 0), groups=1, c_gstride=0, c_shift_from_n=0, c_shift=0, **_):
    """element offsets from the C base of the logical elements (rows x [0, N)) of every group: [groups, len(rows), N]"""
    cols = torch.arange(N, device=rows.device)
    dst = cols + c_shift * (cols >= c_shift_from_n).long() if c_shift_from_n > 0 else cols
    base = rowmap(rows, *c_map) * ldc
    return (torch.arange(max(groups, 1), device=rows.device) * c_gstride)[:, None, None] + base[None, :, None] + dst[None, None, :]


def gemm_store(out, vals, *, M, ldc, c_map=(0, 0), groups=1, c_gstride=0, c_shift_from_n=0, c_shift=0, **_):
    """the whole C buffer after the call: `out` (flat, the buffer before the call) with vals [groups, M, N] stored; everything else untouched"""
    o = out.to(F64).clone()
    m, cols = torch.arange(M), torch.arange(vals.shape[-1])
    rows_phys = int(rowmap(m, *c_map).max()) + 1
    for g in range(max(groups, 1)):
        view = o[g * c_gstride:].as_strided((rows_phys, ldc), (ldc, 1))
        _store(view, m, cols, c_map, c_shift_from_n, c_shift, vals[g])
    return o


def sample_rows(M, *, boundaries=(), seed=0, per_tile=8):
    """the logical rows a large case is judged on in float64: first and last row of every 256-row tile, per_tile seeded rows of each, the rows
    on both sides of every multiple of each period in `boundaries` (rows per sample, rows per batch of the row maps; periods <= 8 have no
    'inside' and are left to the seeded rows), the last 8 rows."""
    import random
    s = set(range(max(0, M - 8), M))
    for t0 in range(0, M, TILE):
        t1 = min(t0 + TILE, M)
        s |= {t0, t1 - 1}
        s |= set(random.Random(seed * 100003 + t0).sample(range(t0, t1), min(per_tile, t1 - t0)))
    for p in boundaries:
        if p > 8:
            for b in range(p, M, p):
                s |= {b - 1, b}
    return torch.tensor(sorted(s))


def tail_from(rows, M):
    """index into the sorted row set `rows` of the first row of the last partial tile (of the last tile if M is a multiple of 256)"""
    t0 = (M - 1) // TILE * TILE
    return int((rows < t0).sum())


def judge(got, truth, var=None, rows_from=None):
    """the judging function of the forward sweeps: (rel-L2, worst row, worst row of the tail) of `got` against the fp64 truth and their bounds -
    max(1.5 x the rounding-point variant's own figure, 2^-9) where a variant is given (bf16 outputs), else the fp32 twins' 1e-5 / 1e-4 / 1e-4.
    -> (figures, bounds, ok)"""
    k = err(got, truth, rows_from=rows_from)
    b = (F32_TOTAL, F32_ROW, F32_ROW) if var is None else tuple(max(1.5 * e, FLOOR) for e in err(var, truth, rows_from=rows_from))
    return k, b, all(x <= y for x, y in zip(k, b))


def gemm_path(c, ncu, force=0, workspace=True):
    """gemm_plan / splitk_plan of csrc/gemm.hip restated (independently: tests/test_gemm_plan_cpu.py holds the two to each other): which kernel a descriptor without a LoRA segment runs on a chip of `ncu` CUs under
    UG_GEMM_FORCE_TILE = force, with or without the caller's workspace -> (tile, rounds of the persistent walk, K-slices of the split-K tail
    (1: none), tail tiles padded to 8, wide16 bits: 1 = 16-byte epilogue accesses, 2 = one row map per tile). The 128^2 kernel: (128, 1, 1, 0, 0).
    c: M, N, K, epilogue, groups, a_map, c_map, r_map, lda, ldw, ldc, ldr, c_gstride, r_gstride, c_off / r_off (elements the C / R base sits
    off a 16-byte boundary, x 2 bytes)."""
    M, N, K, epi, groups = c["M"], c["N"], c["K"], c["epilogue"], max(c.get("groups", 1), 1)
    cdiv = lambda x, y: (x + y - 1) // y
    t256, t128 = cdiv(M, 256) * cdiv(N, 256) * groups, cdiv(M, 128) * cdiv(N, 128) * groups
    nkt = K // 64

    def plan(tiles):
        rem = tiles % ncu
        if rem == 0 or rem * 2 > ncu or not workspace or nkt < 96:
            return 0, 1
        rem8 = (rem + 7) // 8 * 8
        cand = min(ncu // rem8, 8, nkt // 4)
        if cand < 2 or rem8 * cand > 256:             # ug_gemm_workspace_bytes(): 4096 + 256 slabs of 256^2 fp32
            return 0, 1
        return rem8, cand

    big = M >= 192 and N >= 192 and t256 / (cdiv(t256, 256) * 256) >= 0.6 * t128 / (cdiv(t128, 512) * 512)
    if not big and epi != EPI_F32 and M >= 192 and N >= 192 and t256 < ncu:
        nsl = plan(t256)[1]
        if nsl > 1:
            t_split = 1.53 * nkt / nsl + 22.0 + 2.5 * nsl
            t_128 = cdiv(t128, 2 * ncu) * nkt * (0.97 if t128 <= ncu else 1.27)
            big = t_split < 0.9 * t_128
    if force == 128:
        big = False
    if force == 256:
        big = True
    a_rpb, a_bs = c.get("a_map", (0, 0))
    lda, ldw = c.get("lda") or K, c.get("ldw") or K
    if a_rpb > 0 and a_bs < a_rpb:
        big = False
    jumps = cdiv(255, a_rpb) if a_rpb > 0 else 0
    a_jump = (a_bs - a_rpb) * jumps if a_rpb > 0 and a_bs > a_rpb else 0
    if ((255 + a_jump) * lda + K) * 2 + 256 >= 1 << 31 or (255 * ldw + K) * 2 + 256 >= 1 << 31:
        big = False
    if not big:
        return 128, 1, 1, 0, 0
    res = epi in (EPI_RES_GATE, EPI_RES_SCALE)
    ldc, ldr = c.get("ldc") or N, c.get("ldr") or N
    wide = N % 8 == 0 and ldc % 8 == 0 and c.get("c_gstride", 0) % 8 == 0 and c.get("c_off", 0) % 8 == 0 and \
        (not res or (ldr % 8 == 0 and c.get("r_gstride", 0) % 8 == 0 and c.get("r_off", 0) % 8 == 0))
    contig = c.get("c_map", (0, 0))[0] % 256 == 0 and (not res or c.get("r_map", (0, 0))[0] % 256 == 0)
    rem8, nsl = plan(t256)
    return 256, cdiv(t256, ncu), nsl, rem8, int(wide) | (2 if contig else 0)


# ---- AdaLN modulate ----
def adaln_modulate(x, shift, scale, *, rows, D, rows_per_sample, mod_ld, ldx=None, x_map=(0, 0), eps=1e-6, rnd=bf16):
    """ug_adaln_modulate: out[r] = LayerNorm(x[map(r)][:D]; eps, biased variance, no affine) (1 + scale[r // rows_per_sample]) +
    shift[r // rows_per_sample]; x, shift, scale flat buffers (modulation row b at b * mod_ld). Returns (exact, variant) [rows, D]; the variant
    rounds bf16(LN), bf16(1 + scale), bf16(n s1), then + shift rounded by the store."""
    r = torch.arange(rows)
    X = _flat_rows(x, rowmap(r, *x_map) * (ldx or D), D)
    b = (r // rows_per_sample) * mod_ld
    sh, sc = _flat_rows(shift, b, D), _flat_rows(scale, b, D)
    mean = X.mean(-1, keepdim=True)
    n = (X - mean) * torch.rsqrt(((X - mean) ** 2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    return n * (1.0 + sc) + sh, rnd(rnd(rnd(n) * rnd(1.0 + sc)) + sh)


# ---- small linear ----
def silu(x):
    return x * torch.sigmoid(x)


def small_linear_bf16(x, w, bias, *, M, N, K, act_in=0, residual=None, ldx=None, ldw=None, ldr=None):
    """ug_small_linear_bf16: out[m][n] = R[m][n] + bf16(sum_k act(x[m][k]) W[n][k] + b[n]) (act_in 1: SiLU). As for the GEMM's v, the exact
    result rounds nothing - bf16(.) of an fp32 sum is not a function of the operands that a second implementation can reproduce bit for bit.
    Returns (exact, variant) [M, N]; the variant takes bf16(silu(x)) as the operand, rounds bf16(acc + b), and + R is rounded by the store."""
    X = _flat_rows(x, torch.arange(M) * (ldx or K), K)
    W = _flat_rows(w, torch.arange(N) * (ldw or K), K)
    b = 0.0 if bias is None else _flat_rows(bias, torch.tensor([0]), N)
    R = None if residual is None else _flat_rows(residual, torch.arange(M) * (ldr or N), N)
    ex = (silu(X) if act_in else X) @ W.t() + b
    va = bf16((bf16(silu(X)) if act_in else X) @ W.t() + b)
    if R is not None:
        ex, va = ex + R, bf16(va + R)
    return ex, va
