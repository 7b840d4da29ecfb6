"""tests/fwd_ref.py against independent formulations in float64 on small shapes (no GPU): the references the forward projection sweep
(tests/test_fuzz_forward_gpu.py) measures the kernels against are right to 1e-12, their rounding-point variants round where the oracle's bf16
evaluation rounds, and the sweep's tolerance - max(1.5 x the variant's own error, 2^-9) on the rel-L2, the worst row and the worst row of the
last partial tile - is at least 10 x below the error of each plausible slip of a kernel (sensitivity). Also the fusion decision of
unigen_amd.ops.qk_rope_fusable against what the fused epilogue's launcher accepts."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import unigen_ref as R
from tests import fwd_ref as FR

F64 = torch.float64
TOL = 1e-12
FLOOR = 2.0 ** -9


def rel(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm())


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rms(x, w):
    """RMSNorm in float64 (torch's own; the oracle's rms_norm takes its statistics in fp32)"""
    return F.rms_norm(x, (x.shape[-1],), w.to(x.dtype), eps=1e-6)


def _rope_complex(x, cos, sin):
    """RoPE as a complex product: pair (x[2i], x[2i+1]) times cos[2i] + i sin[2i] (tables repeat each value over the pair)"""
    z = torch.view_as_complex(x.reshape(*x.shape[:-1], -1, 2).contiguous())
    e = torch.complex(cos[..., 0::2], sin[..., 0::2])
    return torch.view_as_real(z * e).flatten(-2)


def _qk_case(seed, dh=64, heads=3, B=2, L=37, bstride=41, pos_offset=5, split=20, q_off=8, k_off=None):
    g = _g(seed)
    k_off = q_off + heads * dh + 8 if k_off is None else k_off
    ld = k_off + heads * dh + 24
    buf = FR.spread_rows(g, B * bstride, ld)
    wq_a, wq_b = FR.norm_weights(g, dh)
    wk_a, wk_b = FR.norm_weights(g, dh)
    cos, sin, _ = FR.rope_tables(g, pos_offset + L + 1, dh)
    kw = dict(batches=B, rows_per_batch=L, batch_stride_rows=bstride, pos_offset=pos_offset, q_off=q_off, k_off=k_off, heads=heads, dh=dh,
              wq_a=wq_a, wk_a=wk_a, wq_b=wq_b, wk_b=wk_b, split=split, cos=cos, sin=sin)
    return buf, kw


def _rows(kw):
    r = torch.arange(kw["rows_per_batch"])
    return (torch.arange(kw["batches"])[:, None] * kw["batch_stride_rows"] + r).flatten(), (kw["pos_offset"] + r).repeat(kw["batches"])


@pytest.mark.parametrize("dh", [64, 128])
def test_qk_rmsnorm_rope_reference(dh):
    buf, kw = _qk_case(1 + dh, dh=dh)
    exact, var = FR.qk_rmsnorm_rope(buf, **kw)
    phys, pos = _rows(kw)
    H = kw["heads"]
    touched = torch.zeros_like(buf, dtype=torch.bool)
    for off, (wa, wb) in ((kw["q_off"], (kw["wq_a"], kw["wq_b"])), (kw["k_off"], (kw["wk_a"], kw["wk_b"]))):
        x = buf[phys, off:off + H * dh].reshape(-1, H, dh)
        for side, w in ((pos < kw["split"], wa), (pos >= kw["split"], wb)):
            u = _rms(x[side], w)
            y = _rope_complex(u, kw["cos"].to(F64)[pos[side]][:, None], kw["sin"].to(F64)[pos[side]][:, None])
            got = exact[phys[side], off:off + H * dh].reshape(-1, H, dh)
            assert rel(got, y) < TOL
            # the rounding-point variant against the oracle's bf16 evaluation: RMSNorm in bf16 (fp32 statistics) then apply_rotary_emb (fp32, bf16 out)
            ob = R.apply_rotary_emb(R.rms_norm(x[side].to(torch.bfloat16), w.to(torch.bfloat16)).transpose(0, 1)[None],
                                    kw["cos"][pos[side]], kw["sin"][pos[side]])[0].transpose(0, 1).to(F64)
            vb = var[phys[side], off:off + H * dh].reshape(-1, H, dh)
            assert torch.equal(vb, FR.bf16(vb))
            assert float((vb != ob).to(F64).mean()) < 0.02 and rel(vb, ob) < 2.0 ** -10, (float((vb != ob).to(F64).mean()), rel(vb, ob))
        touched[phys, off:off + H * dh] = True
    # nothing else is written; the zero row stays exactly zero
    assert torch.equal(exact[~touched], buf[~touched]) and torch.equal(var[~touched], buf[~touched])
    z = buf.abs().sum(1) == 0
    assert z.any() and not exact[z].any() and not var[z].any()


def test_qk_rmsnorm_rope_reference_options():
    """NULL weights on one side (no RMSNorm there), no table (no RoPE), k only"""
    buf, kw = _qk_case(7, dh=128, heads=2, q_off=-1, k_off=16)
    kw.update(wk_a=None, cos=None, sin=None)
    exact, var = FR.qk_rmsnorm_rope(buf, **kw)
    phys, pos = _rows(kw)
    H, dh = kw["heads"], kw["dh"]
    x = buf[phys, 16:16 + H * dh].reshape(-1, H, dh)
    got = exact[phys, 16:16 + H * dh].reshape(-1, H, dh)
    a = pos < kw["split"]
    assert torch.equal(got[a], x[a]) and rel(got[~a], _rms(x[~a], kw["wk_b"])) < TOL
    assert torch.equal(exact[:, :16], buf[:, :16]) and torch.equal(var[:, 16 + H * dh:], buf[:, 16 + H * dh:])


def _gather(t, m, rpb, bs):
    """logical rows of a row-mapped buffer, by a plain loop (independent of fwd_ref.rowmap)"""
    return torch.stack([t[(i // rpb) * bs + i % rpb] if rpb else t[i] for i in m.tolist()])


@pytest.mark.parametrize("epi", [FR.EPI_BIAS, FR.EPI_BIAS_GELU, FR.EPI_RES_GATE, FR.EPI_RES_SCALE])
def test_lora_gemm_reference(epi):
    g = _g(10 + epi)
    M, N, K, r, rp = 70, 520, 64, 24, 64
    a, w, b, t, lb = FR.lora_operands(g, M, N, K, r, rp)
    a_phys = torch.cat([a, torch.zeros(40, K, dtype=F64)])        # A row map: 35 rows per batch, batch stride 20 (broadcasting)
    a_map = (35, 20)
    a_phys[:55] = FR.bf16(torch.randn(55, K, generator=g, dtype=F64))
    c_map, r_map = (35, 50), (35, 40)
    out = FR.bf16(torch.randn(100, N + 256 + 8, generator=g, dtype=F64))
    res = FR.bf16(torch.randn(90, N, generator=g, dtype=F64))
    gate = FR.bf16(torch.randn(3, N, generator=g, dtype=F64))
    kw = dict(M=M, epilogue=epi, t=t, lb=lb, a_map=a_map, c_map=c_map)
    if epi in (FR.EPI_RES_GATE, FR.EPI_RES_SCALE):
        kw.update(residual=res, r_map=r_map, gate=gate, rows_per_sample=30, alpha=0.7)
    if epi == FR.EPI_BIAS_GELU:
        kw.update(gelu_from_n=256, c_shift_from_n=256, c_shift=256 + 8)
    m = torch.arange(M)
    A = _gather(a_phys, m, *a_map)
    # peft's LoRA Linear: T = scaling (x A_lora^T), computed by an earlier launch on the logical rows
    A_lora = torch.randn(rp, K, generator=g, dtype=F64)
    t = 0.5 * (A @ A_lora.t())
    kw["t"] = t
    exact, var = FR.lora_gemm(a_phys, w, b, out, **kw)
    y = R.lora_linear(A, w, b, [(A_lora, lb, 0.5)])
    if epi == FR.EPI_BIAS_GELU:
        y = torch.cat([y[:, :256], F.gelu(y[:, 256:], approximate="tanh")], 1)
    elif epi == FR.EPI_RES_GATE:
        y = _gather(res, m, *r_map) + gate[m // 30] * y
    elif epi == FR.EPI_RES_SCALE:
        y = _gather(res, m, *r_map) + 0.7 * y
    rows = torch.tensor([(i // 35) * 50 + i % 35 for i in range(M)])
    cols = torch.arange(N) + (264 * (torch.arange(N) >= 256) if epi == FR.EPI_BIAS_GELU else 0)
    assert rel(exact[rows[:, None], cols[None, :]], y) < TOL
    untouched = torch.ones_like(out, dtype=torch.bool)
    untouched[rows[:, None], cols[None, :]] = False
    assert torch.equal(exact[untouched], out[untouched]) and torch.equal(var[untouched], out[untouched])
    # the plain product in exact fp64 to 1e-12: no LoRA, against F.linear
    e0, v0 = FR.lora_gemm(a, w, b, torch.zeros(M, N, dtype=F64), M=M)
    assert rel(e0, F.linear(a, w, b)) < TOL
    # rounding variant vs the oracle's bf16 evaluation where they share rounding points (no LoRA: bf16(acc + bias), GELU in fp32 of that)
    ob = F.linear(a.to(torch.bfloat16), w.to(torch.bfloat16), b.to(torch.bfloat16)).to(F64)
    assert float((v0 != ob).to(F64).mean()) < 0.02 and float(((v0 - ob).abs() / FR.bf16_ulp(ob).clamp_min(1e-30)).max()) <= 1.0
    eg, vg = FR.lora_gemm(a, w, b, torch.zeros(M, N, dtype=F64), M=M, epilogue=FR.EPI_BIAS_GELU)
    assert rel(eg, F.gelu(F.linear(a, w, b), approximate="tanh")) < TOL
    og = F.gelu(FR.bf16(F.linear(a, w, b)).to(torch.bfloat16), approximate="tanh").to(F64)
    assert float((vg != og).to(F64).mean()) < 0.02


def _qkv_case(seed, D=256, dh=128, K=64, M=512, single=True):
    g = _g(seed)
    N = 7 * D if single else 3 * D
    a = FR.spread_rows(g, M, K)
    w = FR.bf16(torch.randn(N, K, generator=g, dtype=F64) * K ** -0.5)
    b = FR.bf16(0.1 * torch.randn(N, generator=g, dtype=F64))
    wq, wk = FR.norm_weights(g, dh)
    cos, sin, cs = FR.rope_tables(g, 400, dh)
    return a, w, b, wq, wk, cos, sin, cs


@pytest.mark.parametrize("dh", [64, 128])
def test_qkv_rope_gemm_reference(dh):
    """the fused launch = Linear, then the stand-alone pass's arithmetic, then GELU / column shift / row map"""
    D, M, rpb, pos0 = 256, 512, 300, 50
    a, w, b, wq, wk, cos, sin, cs = _qkv_case(3, D=D, dh=dh, M=M)
    out = torch.full((2 * 360, 8 * D), 5.0, dtype=F64)
    kw = dict(M=M, wq=wq, wk=wk, cs=cs, rope_rpb=rpb, pos0=pos0, qk_until_n=2 * D, dh=dh, c_map=(256, 360), gelu_from_n=3 * D,
              c_shift_from_n=3 * D, c_shift=D)
    exact, var = FR.qkv_rope_gemm(a, w, b, out, **kw)
    lin = F.linear(a, w, b)
    m = torch.arange(M)
    rows = (m // 256) * 360 + m % 256
    e = exact[rows]
    assert rel(e[:, 2 * D:3 * D], lin[:, 2 * D:3 * D]) < TOL and rel(e[:, 4 * D:], F.gelu(lin[:, 3 * D:], approximate="tanh")) < TOL
    assert torch.equal(e[:, 3 * D:4 * D], out[rows, 3 * D:4 * D])
    # q / k: the stand-alone reference on the Linear's output, positions pos0 + m % rpb
    pos = pos0 + m % rpb
    H = D // dh
    for c0, wn in ((0, wq), (D, wk)):
        x = lin[:, c0:c0 + D].reshape(M, H, dh)
        y = _rope_complex(_rms(x, wn), cos.to(F64)[pos][:, None], sin.to(F64)[pos][:, None]).reshape(M, D)
        assert rel(e[:, c0:c0 + D], y) < TOL
    # the variant = the stand-alone variant on bf16(Linear); row map / shift as above
    lin_b = FR.bf16(lin)
    sa = FR.qk_rmsnorm_rope(lin_b[:rpb], batches=1, rows_per_batch=rpb, q_off=0, k_off=D, heads=H, dh=dh, wq_b=wq, wk_b=wk,
                            cos=cos[pos0:], sin=sin[pos0:])[1]
    # (positions wrap at rpb: compare the rows below the wrap, where stand-alone position = pos0 + m)
    assert torch.equal(var[rows][:rpb, :2 * D], sa[:rpb, :2 * D])
    assert torch.equal(var[rows][:, 4 * D:], FR.bf16(FR.gelu_tanh(lin_b[:, 3 * D:])))
    untouched = torch.ones_like(out, dtype=torch.bool)
    untouched[rows] = False
    untouched[:, 3 * D:4 * D] = True
    assert torch.equal(exact[untouched], out[untouched])
    # no table at dh 64: RMSNorm only
    if dh == 64:
        e2 = FR.qkv_rope_gemm(a, w[:3 * D], b[:3 * D], torch.zeros(M, 3 * D, dtype=F64), M=M, wq=wq, wk=wk, cs=None, rope_rpb=0, pos0=0, qk_until_n=2 * D, dh=dh)[0]
        assert rel(e2[:, :D], _rms(lin[:, :D].reshape(M, H, dh), wq).reshape(M, D)) < TOL


# ----------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the sweep's tolerance is >= 10 x below each plausible slip
# ----------------------------------------------------------------------------------------------------------------------------------
def _bounds(var, truth, rows_from):
    return tuple(max(1.5 * e, FLOOR) for e in FR.err(var, truth, rows_from=rows_from))


def _assert_caught(name, slip, truth, bounds, rows_from):
    k = FR.err(slip, truth, rows_from=rows_from)
    print(f"{name}: slip rel-L2 {k[0]:.3e} worst row {k[1]:.3e} tail {k[2]:.3e}; bounds {bounds}")
    assert k[0] >= 10 * bounds[0] and k[1] >= 10 * bounds[1], (name, k, bounds)


def test_sensitivity_qk_rmsnorm_rope():
    buf, kw = _qk_case(21, dh=128, heads=4, B=2, L=130, bstride=130, pos_offset=3, split=60)
    phys, _ = _rows(kw)
    sel = lambda t: FR.qk_vectors(t, phys, kw["q_off"], kw["k_off"], kw["heads"], kw["dh"])
    exact, var = FR.qk_rmsnorm_rope(buf, **kw)
    truth = sel(exact)
    rf = truth.shape[-2] // 64 * 64
    bounds = _bounds(sel(var), truth, rf)
    slips = {
        "other side's norm weights": dict(kw, wq_a=kw["wq_b"], wq_b=kw["wq_a"], wk_a=kw["wk_b"], wk_b=kw["wk_a"]),
        "RoPE one position off": dict(kw, pos_offset=kw["pos_offset"] + 1, split=kw["split"] + 1),
        "(cos, sin) swapped": dict(kw, cos=kw["sin"], sin=kw["cos"]),
    }
    for name, skw in slips.items():
        s = FR.qk_rmsnorm_rope(buf, **skw)[1]
        _assert_caught(name, sel(s), truth, bounds, rf)
    # the fused epilogue's table: a slip that reads (sin, cos) from the pair table
    _, _, cs = FR.rope_tables(_g(5), 600, 128)
    a, w, b = FR.spread_rows(_g(6), 512, 128), FR.bf16(torch.randn(768, 128, generator=_g(7), dtype=F64) / 11.3), None
    kq = dict(M=512, wq=kw["wq_b"], wk=kw["wk_b"], rope_rpb=300, pos0=7, qk_until_n=512, dh=128)
    exact, var = FR.qkv_rope_gemm(a, w, b, torch.zeros(512, 768, dtype=F64), cs=cs, **kq)
    bq = _bounds(var[:, :512], exact[:, :512], 256)
    for name, slip in (("pair table swapped", FR.qkv_rope_gemm(a, w, b, torch.zeros(512, 768, dtype=F64), cs=cs.flip(-1), **kq)[1]),
                       ("pair table one position off", FR.qkv_rope_gemm(a, w, b, torch.zeros(512, 768, dtype=F64), cs=cs[1:], **kq)[1])):
        _assert_caught(name, slip[:, :512], exact[:, :512], bq, 256)


def test_sensitivity_lora_gemm():
    g = _g(31)
    M, N, K, r = 300, 1792, 64, 128
    a, w, b, t, lb = FR.lora_operands(g, M, N, K, r)
    out = torch.zeros(M, N, dtype=F64)
    exact, var = FR.lora_gemm(a, w, b, out, M=M, t=t, lb=lb)
    bounds = _bounds(var, exact, 256)
    _assert_caught("LoRA term dropped", FR.lora_gemm(a, w, b, out, M=M)[1], exact, bounds, 256)
    # LoRA added after the bf16 rounding of the Linear's output: visible where the LoRA term cancels most of it (the sweep has such cases)
    a, w, b, t, lb = FR.lora_operands(g, M, N, K, r, cancel=True)
    exact, var = FR.lora_gemm(a, w, b, out, M=M, t=t, lb=lb)
    bounds = _bounds(var, exact, 256)
    late = FR.bf16(FR.bf16(a @ w.t() + b) + t @ lb.t())
    _assert_caught("LoRA added after the rounding", late, exact, bounds, 256)
    # GELU one tile early in the column split (single block: GELU from 3D = 768 on, D = 256)
    a, w, b, t, lb = FR.lora_operands(g, M, N, K, r)
    kw = dict(M=M, epilogue=FR.EPI_BIAS_GELU, t=t, lb=lb, gelu_from_n=768)
    exact, var = FR.lora_gemm(a, w, b, out, **kw)
    bounds = _bounds(var, exact, 256)
    _assert_caught("GELU one tile early", FR.lora_gemm(a, w, b, out, **dict(kw, gelu_from_n=512))[1], exact, bounds, 256)


# ----------------------------------------------------------------------------------------------------------------------------------
# the fusion decision
# ----------------------------------------------------------------------------------------------------------------------------------
def test_qk_rope_fusable_refuses_what_the_fused_launch_refuses(monkeypatch):
    from unigen_amd import ops
    monkeypatch.delenv("UG_GEMM_FUSE_QKROPE", raising=False)
    BF = torch.bfloat16
    D, dh = 3072, 128
    # FLUX at 896 x 1152, B = 4: Ls = 4032 = 15.75 x 256, M = 16128 = 63 x 256, 2268 tiles - the C row map splits tiles
    assert not ops.qk_rope_fusable(4 * 4032, 3 * D, 2 * D, dh, BF, c_rpb=4032, rope_rpb=4032)
    # D = 3072, Ls = 448, B = 8: 504 tiles, the old check accepted it
    assert not ops.qk_rope_fusable(8 * 448, 3 * D, 2 * D, dh, BF, c_rpb=448, rope_rpb=448)
    # SD3.5 attn2 at Ls < 256 and a large batch: no C row map, but positions wrap inside a 16-row group
    assert not ops.qk_rope_fusable(32 * 128, 3 * 1536, 2 * 1536, 64, BF, c_rpb=0, rope_rpb=128)
    # what fuses today: the 1024^2 forward's double block (Ls = 4096) and single block (Lj = 4608), SD3.5 attn2 at Ls = 4096
    assert ops.qk_rope_fusable(2 * 4096, 3 * D, 2 * D, dh, BF, c_rpb=4096, rope_rpb=4096)
    assert ops.qk_rope_fusable(2 * 4608, 7 * D, 2 * D, dh, BF, c_rpb=0, rope_rpb=4608)
    assert ops.qk_rope_fusable(2 * 4096, 3 * 1536, 2 * 1536, 64, BF, c_rpb=0, rope_rpb=4096)
    # rope rows per batch above 256 but not a multiple of it: the epilogue wraps positions inside a tile (fuses)
    assert ops.qk_rope_fusable(4 * 320 * 16, 3 * D, 2 * D, dh, BF, c_rpb=0, rope_rpb=320)
    # below one round of tiles, fp32, other head widths: as before
    assert not ops.qk_rope_fusable(4096, 3 * 512, 2 * 512, dh, BF, c_rpb=4096, rope_rpb=4096)
    assert not ops.qk_rope_fusable(2 * 4096, 3 * D, 2 * D, dh, torch.float32, c_rpb=4096, rope_rpb=4096)
    assert not ops.qk_rope_fusable(2 * 4096, 3 * D, 2 * D, 96, BF, c_rpb=4096, rope_rpb=4096)
    monkeypatch.setenv("UG_GEMM_FUSE_QKROPE", "0")
    assert not ops.qk_rope_fusable(2 * 4096, 3 * D, 2 * D, dh, BF, c_rpb=4096, rope_rpb=4096)


def test_qk_rope_fusable_defaults_describe_an_identity_launch(monkeypatch):
    """Without row maps (the defaults) the decision is the tile-shape check alone, as for a launch straight into a [M, N] buffer."""
    from unigen_amd import ops
    monkeypatch.delenv("UG_GEMM_FUSE_QKROPE", raising=False)
    BF = torch.bfloat16
    assert ops.qk_rope_fusable(4 * 4608, 7 * 3072, 2 * 3072, 128, BF)
    assert ops.qk_rope_fusable(4 * 4608, 7 * 3072, 2 * 3072, 128, BF) == ops.qk_rope_fusable(4 * 4608, 7 * 3072, 2 * 3072, 128, BF, c_rpb=0, rope_rpb=0)
    assert not ops.qk_rope_fusable(4 * 4032, 3 * 3072, 2 * 3072, 128, BF, c_rpb=4032)
    assert not ops.qk_rope_fusable(32 * 128, 3 * 1536, 2 * 1536, 64, BF, rope_rpb=128)
