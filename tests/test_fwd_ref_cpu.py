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


# ----------------------------------------------------------------------------------------------------------------------------------
# the base GEMM, AdaLN modulate and small linear references (tests/test_fuzz_gemm_gpu.py): pins, the path table, sensitivity
# ----------------------------------------------------------------------------------------------------------------------------------
from tests import test_fuzz_gemm_gpu as TG  # noqa: E402  (data and helpers only; nothing in it touches a GPU at import)

CPU = torch.device("cpu")


def _logical(c, o, g=0):
    """logical operands of group g of a case, by plain loops / slices (independent of fwd_ref's index arithmetic)"""
    M, N, K = c["M"], c["N"], c["K"]
    m = torch.arange(M)
    A = _gather(o["a"][g * c["a_gstride"]:][:c["a_rows"] * c["lda"]].view(-1, c["lda"]).to(F64), m, *c["a_map"])[:, :K]
    W = o["w"][g * c["w_gstride"]:][:N * c["ldw"]].view(N, c["ldw"])[:, :K].to(F64)
    b = None if o["bias"] is None else o["bias"][g * c["bias_gstride"]:][:N].to(F64)
    R = G = None
    if c["epilogue"] in (FR.EPI_RES_GATE, FR.EPI_RES_SCALE):
        src = o["c0"][TG.PAD + c["c_off"]:] if c["alias"] else o["r"][c["r_off"]:]
        R = _gather(src[g * c["r_gstride"]:][:c["c_rows"] * c["ldr"]].view(-1, c["ldr"]).to(F64), m, *c["r_map"])[:, :N]
    if c["epilogue"] == FR.EPI_RES_GATE:
        G = o["gate"][g * c["gate_gstride"]:][:c["gate_rows"] * c["gate_ld"]].view(-1, c["gate_ld"])[:, :N].to(F64)[m // c["rows_per_sample"]]
    return A, W, b, R, G


_PIN_CASES = [
    TG._case("pin res_gate", (0,), 300, 520, 128, FR.EPI_RES_GATE, groups=3, rps=70, a_map=(100, 117), c_map=(100, 104), alias=True, c_off=4),
    TG._case("pin res_scale", (0,), 150, 260, 64, FR.EPI_RES_SCALE, groups=2, a_map=(50, 0)),
    TG._case("pin gelu split", (0,), 130, 768, 64, FR.EPI_BIAS_GELU, split=(256, 264), bias=False),
    TG._case("pin f32", (0,), 77, 36, 192, FR.EPI_F32, groups=2, c_map=(40, 50)),
]


@pytest.mark.parametrize("c", _PIN_CASES, ids=lambda c: c["name"])
def test_gemm_reference(c):
    o = TG.gemm_operands(c, 5, CPU)
    exact, var = TG.gemm_reference(c, o, torch.arange(c["M"]))
    for g in range(c["groups"]):
        A, W, b, R, G = _logical(c, o, g)
        y = F.linear(A, W, b)
        if c["epilogue"] == FR.EPI_BIAS_GELU:
            y = torch.cat([y[:, :c["gelu_from_n"]], F.gelu(y[:, c["gelu_from_n"]:], approximate="tanh")], 1)
        elif c["epilogue"] == FR.EPI_RES_GATE:
            y = R + R_gate(G, y)
        elif c["epilogue"] == FR.EPI_RES_SCALE:
            y = R + float(torch.tensor(0.7, dtype=torch.float32)) * y
        assert rel(exact[g], y) < TOL
        assert torch.equal(var[g], exact[g]) if c["epilogue"] == FR.EPI_F32 else torch.equal(var[g], FR.bf16(var[g]))
    # a subset of rows = the same rows of the whole; the store: logical elements land where gemm_dest says, everything else keeps its value
    rows = torch.tensor([0, 3, c["M"] // 2, c["M"] - 1])
    assert torch.equal(TG.gemm_reference(c, o, rows)[0], exact[:, rows])
    base = o["c0"][TG.PAD + c["c_off"]:]
    buf = FR.gemm_store(base, var, **c)
    dest = FR.gemm_dest(torch.arange(c["M"]), **c)
    prow = [(i // c["c_map"][0]) * c["c_map"][1] + i % c["c_map"][0] if c["c_map"][0] else i for i in range(c["M"])]
    n = c["N"] - 1
    assert int(dest[-1, 5, n]) == (c["groups"] - 1) * c["c_gstride"] + prow[5] * c["ldc"] + n + (c["c_shift"] if c["c_shift_from_n"] and n >= c["c_shift_from_n"] else 0)
    w = torch.zeros(buf.numel(), dtype=torch.bool)
    w[dest.reshape(-1)] = True
    assert torch.equal(buf[dest], var) and torch.equal(buf[~w], base.to(F64)[~w]) and int(w.sum()) == dest.numel()


def R_gate(G, y):
    return R._gate(G, y)


def test_gemm_path_table_at_256_cus():
    """every committed case takes the dispatch path it is there for (a dispatcher change that uncovers a path fails here, without a GPU)"""
    for c in TG.GEMM_CASES:
        assert FR.gemm_path(c, 256) == c["path"], (c["name"], FR.gemm_path(c, 256))
        if c["path_nows"]:
            assert FR.gemm_path(c, 256, workspace=False) == c["path_nows"], c["name"]
            assert c["path"][2] > 1 and c["path_nows"][2] == 1
    paths = {c["path"] for c in TG.GEMM_CASES}
    assert {p[1] for p in paths} >= {1, 2, 3} and {p[4] for p in paths if p[0] == 256} == {1, 2, 3} and {p[0] for p in paths} == {128, 256}
    wide = next(c for c in TG.GEMM_CASES if c["a_sparse"])
    assert FR.gemm_path(dict(wide, lda=wide["lda"] - 64), 256)[0] == 256           # just below 2^31 bytes the same shape stays on the 256^2 kernel
    assert all(FR.gemm_path(c, 256, force=128)[0] == 128 for c in TG.GEMM_CASES)


def _reduced(c, **kw):
    """a reduced copy of a committed case: same epilogue, maps and options at a size whose full fp64 truth is cheap"""
    args = dict(M=600, N=1032 if c["N"] % 8 == 0 else 1028, K=min(c["K"], 256))
    args.update(kw)
    return TG._case(c["name"], c["path"], args["M"], args["N"], args["K"], c["epilogue"], groups=args.get("groups", c["groups"]), bias=c["has_bias"],
                    rps=args.get("rps", c["rows_per_sample"] and min(c["rows_per_sample"], 100)), a_map=args.get("a_map", (0, 0)),
                    c_map=args.get("c_map", (0, 0)), alias=c["alias"], split=args.get("split"))


def _ratio(slip, exact, var, rows_from):
    k, b, ok = FR.judge(slip, exact, var=var, rows_from=rows_from)
    return max((x / y if x == x else float("inf")) for x, y in zip(k, b)), ok


def _caught(name, slip, exact, var, rows_from=None, margin=10.0):
    r, ok = _ratio(slip, exact, var, rows_from)
    print(f"{name}: {r:.1f} x the bound")
    assert not ok and r >= margin, (name, r)


def test_sensitivity_gemm():
    by = {c["name"]: c for c in TG.GEMM_CASES}
    # RES_GATE with sample boundaries inside tiles
    c = _reduced(by["rounds2 19x17 tiles ragged, rps 100"])
    o = TG.gemm_operands(c, 1, CPU)
    m = torch.arange(c["M"])
    ref = lambda **kw: TG.gemm_reference(dict(c, **kw.pop("case", {})), dict(o, **kw), m)
    exact, var = ref()
    rf = FR.tail_from(m, c["M"])
    last = (m + 1) % c["rows_per_sample"] == 0                       # the last row of each sample takes the next sample's gate row
    s = var.clone()
    s[0, last[:-1].nonzero().flatten()] = TG.gemm_reference(c, dict(o, gate=o["gate"][c["gate_ld"]:]), m[:-1][last[:-1]])[1][0]
    _caught("gate one sample off next to a boundary", s, exact, var, rf)
    _caught("bias of column n + 1", ref(bias=torch.roll(o["bias"], -1))[1], exact, var, rf)
    _caught("last K-tile dropped", ref(case=dict(K=c["K"] - 64))[1], exact, var, rf)
    wv = o["w"].clone().view(c["N"], c["ldw"])
    wv[:, 64:128] = 0
    _caught("one K-slice dropped", ref(w=wv.reshape(-1))[1], exact, var, rf)
    wv[:, 64:128] = 2 * o["w"].view(c["N"], c["ldw"])[:, 64:128]
    _caught("one K-slice added twice", ref(w=wv.reshape(-1))[1], exact, var, rf)
    s = var.clone()
    s[0, -1] = TG.SENT
    _caught("row M - 1 unwritten", s, exact, var, rf)
    dest = FR.gemm_dest(m, **c)
    wmask = torch.zeros(o["c0"].numel() - TG.PAD, dtype=torch.bool)
    wmask[dest.reshape(-1)] = True
    one_more = FR.gemm_store(torch.cat([o["c0"][TG.PAD:], o["c0"][:c["ldc"]]]), torch.cat([var, var[:, -1:]], 1), **dict(c, M=c["M"] + 1))
    assert not bool((one_more[:wmask.numel()][~wmask] == TG.SENT).all()), "row M written: the sentinel check sees it"
    # a round-2 tile's row replaced by the same row of the tile `CUs` earlier (4 'CUs', tiles in row-major order): judged on all rows, and by
    # the full-output screen's row check (the form that sees it on a row outside the fp64 sample)
    s = var.clone()
    s[0, 300, 0:256] = var[0, 44, 0:256]                             # tile (1, 0) <- tile (0, 0), in-tile row 44
    _caught("a round-2 row from the tile CUs earlier", s, exact, var, rf)
    sr = TG.screen(c, o, False)
    bound = FR.judge(var, exact, var=var, rows_from=rf)[1][1]
    rows_e = TG._row_err(s[0], sr)
    assert float(rows_e[300]) >= 10 * bound and float(TG._row_err(var[0], sr).max()) <= bound
    assert FR.err(TG.screen(c, o, True), exact[0])[0] <= 1e-5
    # RES_SCALE: alpha dropped
    c = _reduced(by["tail 8 of 264, res_scale"])
    o = TG.gemm_operands(c, 2, CPU)
    exact, var = TG.gemm_reference(c, o, m)
    _caught("alpha dropped", TG.gemm_reference(dict(c, alpha=1.0), o, m)[1], exact, var, rf)
    # groups: group g reads group g + 1's weights / gate
    c = _reduced(by["6 groups on the 256^2 kernel"], M=300, N=520, groups=3, rps=1)
    o = TG.gemm_operands(c, 3, CPU)
    m3 = torch.arange(300)
    exact, var = TG.gemm_reference(c, o, m3)
    c2 = dict(c, groups=2)
    _caught("group g reads group g + 1's weights", TG.gemm_reference(c2, dict(o, w=o["w"][c["w_gstride"]:]), m3)[1], exact[:2], var[:2], 256)
    _caught("group g reads group g + 1's gate", TG.gemm_reference(c2, dict(o, gate=o["gate"][c["gate_gstride"]:]), m3)[1], exact[:2], var[:2], 256)
    # the column split: the shift applied one tile early
    c = _reduced(by["tail 14 of 270, column split"], N=1024, split=(512, 264))
    o = TG.gemm_operands(c, 4, CPU)
    exact, var = TG.gemm_reference(c, o, m)
    early = FR.gemm_store(o["c0"][TG.PAD:], var, **dict(c, c_shift_from_n=256))
    _caught("column shift one tile early", early[FR.gemm_dest(m, **c)], exact, var, rf)
    _caught("GELU one tile early", TG.gemm_reference(dict(c, gelu_from_n=256), o, m)[1], exact, var, rf)
    # slips a bf16 bound cannot see (docs/PARITY_TOLERANCES.md names them): both differ from the variant by rounding-boundary flips only
    A, W, b, _, _ = _logical(c, o)
    v = A @ W.t() + b
    pre = torch.where(torch.arange(c["N"])[None] >= 512, FR.bf16(FR.gelu_tanh(v)), FR.bf16(v))
    print("GELU before the rounding of v: %.2f x the bound (not seen)" % _ratio(pre[None], exact, var, rf)[0])
    c = _reduced(by["rounds2 19x17 tiles ragged, rps 100"])
    o = TG.gemm_operands(c, 1, CPU)
    exact, var = TG.gemm_reference(c, o, m)
    print("residual added before the rounding: %.2f x the bound (not seen)" % _ratio(FR.bf16(exact), exact, var, rf)[0])


def test_screen_share_of_the_variant():
    """the share of the rounding-point variant's elements more than one bf16 ulp from the screen's rounded result (here torch's CPU fp32 matmul), on
    sampled rows of every large committed case: the kernel is allowed max(4 x SCREEN_SHARE, 0.1 %)"""
    worst = 0.0
    for i, c in enumerate(TG.GEMM_CASES):
        if not TG._large(c) or c["epilogue"] == FR.EPI_F32:
            continue
        small = dict(c, M=min(c["M"], 16 * max(c["rows_per_sample"], 1), 520), N=min(c["N"], 2056 if c["N"] % 8 == 0 else 2052))
        small = TG._case(c["name"], c["path"], small["M"], small["N"], c["K"], c["epilogue"], bias=c["has_bias"], rps=c["rows_per_sample"],
                         a_map=c["a_map"] if c["a_map"][0] <= 100 else (0, 0), alias=c["alias"],
                         split=(1024, c["c_shift"]) if c["c_shift"] else None)
        o = TG.gemm_operands(small, 7000 + i, CPU)
        rows = FR.sample_rows(small["M"], boundaries=(small["rows_per_sample"],), seed=i, per_tile=4)[:24]
        var = TG.gemm_reference(small, o, rows)[1][0]
        share = float(TG._ulp_far(var.float(), TG.screen(small, o, False)[rows]).float().mean())
        worst = max(worst, share)
        print(f"{c['name']}: {share:.2e}")
    print(f"worst share {worst:.2e}; committed SCREEN_SHARE {TG.SCREEN_SHARE:.2e}; the kernel's allowance {TG.SHARE_BOUND:.2e}")
    assert worst <= TG.SCREEN_SHARE


# ---- AdaLN modulate ----
def test_adaln_modulate_reference():
    for i, case in enumerate(TG.ADALN_CASES):
        D, rows, rps, xmap, ex, eo, m1 = case
        if rows > 200:
            continue
        xb, mod, const = TG.adaln_data(case, 9000 + i, BF16)
        exact, var = FR.adaln_modulate(xb, mod, mod.reshape(-1)[D:], **TG._adaln_kw(case))
        x = _gather(xb, torch.arange(rows), *xmap)[:, :D]
        b = torch.arange(rows) // rps
        y = F.layer_norm(x, (D,), None, None, float(torch.tensor(1e-6, dtype=torch.float32))) * (1 + mod[b, D:2 * D]) + mod[b, :D]
        assert rel(exact, y) < TOL, case
        assert torch.equal(exact[const], mod[b, :D][const]) and torch.equal(var[const], mod[b, :D][const])
        if rps > 1 and xmap[0] == 0:           # the oracle's per-sample form (AdaLayerNormZero / _mod)
            n = rows // rps * rps
            yo = R._mod(R.layer_norm(x[:n].view(-1, rps, D), eps=float(torch.tensor(1e-6, dtype=torch.float32))), mod[:n // rps, D:2 * D], mod[:n // rps, :D])
            assert rel(exact[:n], yo.reshape(n, D)) < TOL
        ob = R._mod(R.layer_norm(x.to(BF16)[:, None]), mod[b, D:2 * D].to(BF16)[:, None], mod[b, :D].to(BF16)[:, None])[:, 0].to(F64)   # bf16 eager rounding points
        assert float((var != ob).to(F64).mean()) < 0.05, (case, float((var != ob).to(F64).mean()))


BF16 = torch.bfloat16


def test_adaln_fp32_layer_norm_boundary():
    """torch's own fp32 F.layer_norm against fp64 on the sweep's rows: it stays inside the twins' 1e-5 / 1e-4 at every row mean of the sweep (up to
    ADALN_TWIN_MAX_MEAN standard deviations), so the twin is held to them on all of ADALN_MEANS; the figures per mean are printed."""
    assert max(TG.ADALN_MEANS) <= TG.ADALN_TWIN_MAX_MEAN
    for D in (64, 1536, 4096):
        g = _g(D)
        for mean in TG.ADALN_MEANS + (256.0, 1024.0):
            x = ((torch.randn(256, D, generator=g, dtype=F64) + mean) * 3.0).float()
            k = FR.err(F.layer_norm(x, (D,), None, None, 1e-6), F.layer_norm(x.to(F64), (D,), None, None, 1e-6))
            print(f"F.layer_norm fp32, D {D}, mean {mean:g} sd: rel-L2 {k[0]:.2e} worst row {k[1]:.2e}")
            if mean <= TG.ADALN_TWIN_MAX_MEAN:
                assert k[0] <= FR.F32_TOTAL and k[1] <= FR.F32_ROW, (D, mean, k)


def test_sensitivity_adaln():
    case = (200, 130, 50, (65, 70), 0, 8, False)
    D, rows, rps = case[:3]
    xb, mod, const = TG.adaln_data(case, 1, BF16)
    kw = TG._adaln_kw(case)
    exact, var = FR.adaln_modulate(xb, mod, mod.reshape(-1)[D:], **kw)
    rf = (rows - 1) // 4 * 4
    _caught("shift / scale swapped", FR.adaln_modulate(xb, mod.reshape(-1)[D:], mod, **kw)[1], exact, var, rf)
    _caught("another sample's modulation row", FR.adaln_modulate(xb, mod.reshape(-1)[kw["mod_ld"]:], mod.reshape(-1)[kw["mod_ld"] + D:],
                                                                 **dict(kw, rows=100))[1], exact[:100], var[:100], 96)
    # eps dropped: 0 x rsqrt(0) on a constant row is NaN, which fails every comparison
    x = _gather(xb, torch.arange(rows), *case[3])[:, :D]
    b = torch.arange(rows) // rps
    noeps = (x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, unbiased=False, keepdim=True)) * (1 + mod[b, D:2 * D]) + mod[b, :D]
    assert len(const) and noeps[const].isnan().all() and not FR.judge(FR.bf16(noeps), exact, var=var, rows_from=rf)[2]
    # unbiased variance: 1 / (2 D) relative - below a bf16 bound from D = 64 up (named in the document); the fp32 twin's bounds see it at every D <= 4096
    for D in (64, 4096):
        x = torch.randn(16, D, generator=_g(D), dtype=F64)
        e = F.layer_norm(x, (D,), None, None, 1e-6)
        u = (x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, unbiased=True, keepdim=True) + 1e-6)
        _caught(f"unbiased variance at D {D} (fp32 twin's bounds)", u, e, None)
        print("  against a bf16 bound: %.2f x (below the 10 x margin)" % _ratio(FR.bf16(u), e, FR.bf16(e), None)[0])


# ---- small linear ----
def test_small_linear_reference_and_sensitivity():
    case = (15, 24, 520, True, True, True)
    M, N, K = case[:3]
    x, w, b, r = TG.small_linear_data(case, 1)
    kw = dict(M=M, N=N, K=K, ldx=K + 8, ldw=K + 16, ldr=N + 8)
    exact, var = FR.small_linear_bf16(x, w, b, act_in=1, residual=r, **kw)
    assert float(x.abs().max()) == 30.0
    assert rel(exact, r[:, :N] + F.linear(F.silu(x[:, :K]), w[:, :K], b)) < TOL
    assert rel(FR.small_linear_bf16(x, w, None, act_in=0, **kw)[0], F.linear(x[:, :K], w[:, :K])) < TOL
    ob = (r[:, :N].to(BF16) + F.linear(F.silu(x[:, :K].to(BF16)), w[:, :K].to(BF16), b.to(BF16))).to(F64)        # the oracle's bf16 evaluation (adaln_zero's linear)
    assert float((var != ob).to(F64).mean()) < 0.05
    _caught("SiLU dropped", FR.small_linear_bf16(x, w, b, act_in=0, residual=r, **kw)[1], exact, var)
    _caught("the last 8 of K dropped", FR.small_linear_bf16(x, w, b, act_in=1, residual=r, **dict(kw, K=K - 8))[1], exact, var)
    dup = var.clone()
    dup[:, N - 2] = var[:, N - 1]
    _caught("column N - 1 duplicated into N - 2", dup, exact, var)
    # the same two local slips at the sweep's largest sizes: printed (the per-row bound's margin shrinks as sqrt(8 / K), sqrt(2 / N))
    case = (3, 1000, 4096, True, True, False)
    x, w, b, _ = TG.small_linear_data(case, 2)
    kw = dict(M=3, N=1000, K=4096, ldx=4104, ldw=4112)
    exact, var = FR.small_linear_bf16(x, w, b, act_in=1, **kw)
    r1, ok1 = _ratio(FR.small_linear_bf16(x, w, b, act_in=1, **dict(kw, K=4088))[1], exact, var, None)
    dup = var.clone()
    dup[:, 998] = var[:, 999]
    r2, ok2 = _ratio(dup, exact, var, None)
    print(f"K 4096: last 8 of K dropped {r1:.1f} x; N 1000: duplicated column {r2:.1f} x")
    assert not ok1 and not ok2
