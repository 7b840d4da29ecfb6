"""Seeded random-shape sweeps of the training backward kernels against the float64 references of tests/bwd_ref.py (themselves checked against
torch.autograd by tests/test_bwd_ref_cpu.py): ug_flash_attn_bwd (with the forward's LSE and with lse = NULL, joint and separate layouts, own
row / batch strides per operand, sentinel-filled outputs), the forward's output and base-2 LSE it consumes, the fp32 verification backward of
attention (the GEMM formulation and its row kernels), the top-1 gate, GELU(tanh), q/k RMSNorm + RoPE, AdaLN, colsum and the Linear backward.

Tolerances (docs/PARITY_TOLERANCES.md, "Backward sweep"):
  - fp32 twins: rel-L2 <= 1e-5 against the fp64 truth, every row <= 1e-4.
  - bf16 element-wise outputs (gelu_tanh_bwd, attn_prob, attn_dscore): every element within one bf16 ulp of the fp64 value, plus an absolute
    term for what fp32 arithmetic cannot resolve: 2^-20 (16 fp32 ulps) of the magnitude of the terms that cancel, scaled by the exponent argument
    where an fp32 exp of a rounded argument is taken, and 2^-100 |dy| where fp32 intermediates are subnormal (GELU below x = -9.9).
  - bf16 reductions and attention: rel-L2 to the fp64 truth <= max(1.5 x the error of the rounding-point variant of bwd_ref - bf16 P and dS as
    operands, bf16(x + c), bf16 outputs - against the same truth, 2^-9: the largest relative error a bf16 output rounding alone can make).
  - per row: the same bound, from the variant's own worst row, on the worst (batch, head, row) of dq / dk / dv / dx / dW, and separately on the
    rows of the last, partial 64-row tile. A global rel-L2 hides one wrong row among thousands; this does not.
  Where an output is an fp32 difference that can cancel (dS = P (dP - delta), d logits = g (dg - g.dg)), 2^-20 of the cancellation-free
  magnitude bwd_ref returns is allowed before the relative error counts (one key: dq = dk = 0 exactly).
Out-of-bounds writes are looked for with in-bounds sentinels (spare rows and columns of every output buffer), never by provoking a fault."""
import math
import random

import pytest
import torch

from tests import bwd_ref as BR

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FLOOR = 2.0 ** -9
F32_TOTAL, F32_ROW = 1e-5, 1e-4
SENT_O, SENT_D, SENT_LSE = 3.0, 7.0, -77.0


def _pad64(n):
    return (n + 63) // 64 * 64


def _tail(L):
    """first row of the last, partial 64-row tile (None: L is a multiple of 64)"""
    return None if L % 64 == 0 else L // 64 * 64


def _check(name, got, truth, case, var=None, mag=None, rows_from=None):
    """rel-L2, worst row, worst tail row of `got` against the fp64 truth: bf16 (var given) within max(1.5 x var's own, FLOOR), fp32 absolute."""
    k = BR.err(got, truth, mag, rows_from)
    if var is None:
        bounds = (F32_TOTAL, F32_ROW, F32_ROW)
    else:
        bounds = tuple(max(1.5 * e, FLOOR) for e in BR.err(var, truth, mag, rows_from))
    print(f"{name}: rel-L2 {k[0]:.3e} (bound {bounds[0]:.3e}), worst row {k[1]:.3e} ({bounds[1]:.3e}), tail {k[2]:.3e} ({bounds[2]:.3e})")
    for what, e, b in zip(("rel-L2", "worst row", "worst row of the partial tile"), k, bounds):
        assert e <= b, (name, what, e, b, case)


def _check_elem(name, got, truth, tol, case):
    d = (got.double().cpu() - truth).abs()
    bad = d > tol
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError((name, f"{int(bad.sum())} elements out of bound", "first", i, float(got.flatten()[i]), float(truth.flatten()[i]),
                              float(tol.flatten()[i]), case))


def _sentinel_ok(buf, rows, cols, fill):
    t = buf.detach().cpu().clone()
    t[..., :rows, :cols] = fill
    return bool((t == fill).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# flash attention forward + backward through the C ABI
# ----------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 17, 63, 64, 65, 127, 129, 200, 333, 520, 1023, 1025]


def _attn_case(rng, dh, B, H, Lq, Lkv, joint=None):
    if joint is None:
        joint = rng.random() < 0.5 and Lq <= Lkv
    return dict(dh=dh, B=B, H=H, Lq=Lq, Lkv=Lkv, joint=joint, kv_shared=rng.random() < 0.5, qoff=rng.randint(0, Lkv - Lq) if joint else 0,
                pads=[8 * rng.choice([0, 1, 2, 3, 8]) for _ in range(8)], rpads=[rng.choice([0, 1, 5]) for _ in range(8)])


def _run_attention(gpu, c, seed, data=None):
    """Forward with LSE, then the backward with that LSE and with lse = NULL, on the layout c, against bwd_ref.attention. data None: N(0, 1)
    operands drawn from `seed`, scale dh^-0.5, the forward bounded by the rounding-point variant O_r; returns whether the two backward runs
    agree bit for bit. data (bwd_ref.attention_regime's dict: q, k, v, do as [B, H, L, dh] bf16): those operands with c["scale"], every other
    element of the operand buffers - spare rows, pad columns, the key buffer's unused query columns - NaN, the forward bounded by the
    lazy-reference-point variant O_l; returns what the regimes sweep checks further (tests/test_fuzz_attention_gpu.py)."""
    from unigen_amd import lib as L, ops
    B, H, dh, Lq, Lkv = c["B"], c["H"], c["dh"], c["Lq"], c["Lkv"]
    D, scale = H * dh, c.get("scale", dh ** -0.5)
    g = torch.Generator().manual_seed(seed)
    P, R = c["pads"], c["rpads"]

    def new(rows, width, i, fill=None):       # [B, rows + spare rows, width + spare columns]: batch stride padded by whole rows
        shape = (B, rows + R[i], width + P[i])
        if fill is None and data is not None:
            fill = float("nan")
        return torch.randn(*shape, generator=g).to(BF) if fill is None else torch.full(shape, fill, dtype=BF)

    spec = {}
    if c["joint"]:                                     # queries are rows [qoff, qoff + Lq) of the key buffer
        X = new(Lkv, (3 if c["kv_shared"] else 2) * D, 0)
        spec["q"], spec["k"] = (X, c["qoff"], 0), (X, 0, D)
        spec["v"] = (X, 0, 2 * D) if c["kv_shared"] else (new(Lkv, D, 1), 0, 0)
    else:
        spec["q"] = (new(Lq, D, 0), 0, 0)
        if c["kv_shared"]:
            KV = new(Lkv, 2 * D, 1)
            spec["k"], spec["v"] = (KV, 0, 0), (KV, 0, D)
        else:
            spec["k"], spec["v"] = (new(Lkv, D, 1), 0, 0), (new(Lkv, D, 2), 0, 0)
    spec["o"] = (new(Lq, D, 3, SENT_O), 0, 0)
    spec["do"] = (new(Lq, D, 4), 0, 0)
    if data is not None:
        for n, rows in (("q", Lq), ("k", Lkv), ("v", Lkv), ("do", Lq)):
            t, r0, c0 = spec[n]
            t[:, r0:r0 + rows, c0:c0 + D] = data[n].transpose(1, 2).reshape(B, rows, D)
    on_gpu = {}
    for t, _, _ in spec.values():
        if id(t) not in on_gpu:
            on_gpu[id(t)] = t.to(gpu)

    def abi(name):          # (flat view at the operand's first element, row stride, batch stride)
        t, r0, c0 = spec[name]
        gt = on_gpu[id(t)]
        rs = t.shape[2]
        return gt.view(-1)[r0 * rs + c0:], rs, t.shape[1] * rs

    def heads(t, r0, c0, rows):
        return t[:, r0:r0 + rows, c0:c0 + D].reshape(B, rows, H, dh).transpose(1, 2).double()

    lse = torch.full((B, H, _pad64(Lq)), SENT_LSE, device=gpu, dtype=F32)
    (qv, q_rs, q_bs), (kv, k_rs, k_bs), (vv, v_rs, v_bs), (ov, o_rs, o_bs) = abi("q"), abi("k"), abi("v"), abi("o")
    ops.flash_attn(qv, kv, vv, ov, batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(q_rs, q_bs), k_strides=(k_rs, k_bs), v_strides=(v_rs, v_bs),
                   o_strides=(o_rs, o_bs), scale=scale, lse=lse)
    torch.cuda.synchronize()
    o_buf = on_gpu[id(spec["o"][0])]
    assert _sentinel_ok(o_buf, Lq, D, SENT_O), ("forward wrote outside its output", c)
    assert bool((lse[..., Lq:] == SENT_LSE).all()), ("forward wrote LSE rows beyond Lq", c)
    lse[..., Lq:] = 0.0                               # ABI: the padding of the statistics reads as zero

    lib = L.load()
    dov = abi("do")
    runs = {}
    for mode in ("lse", "none"):
        outs = dict(dq=new(Lq, D, 5, SENT_D).to(gpu), dk=new(Lkv, D, 6, SENT_D).to(gpu), dv=new(Lkv, D, 7, SENT_D).to(gpu))
        st = lambda t: (t.data_ptr(), t.shape[2], t.shape[1] * t.shape[2])
        ws = torch.empty(int(lib.ug_flash_attn_bwd_workspace_bytes(B, H, Lq)), device=gpu, dtype=torch.uint8)
        rc = lib.ug_flash_attn_bwd(qv.data_ptr(), q_rs, q_bs, kv.data_ptr(), k_rs, k_bs, vv.data_ptr(), v_rs, v_bs, ov.data_ptr(), o_rs, o_bs,
                                   dov[0].data_ptr(), dov[1], dov[2], *st(outs["dq"]), *st(outs["dk"]), *st(outs["dv"]), B, H, Lq, Lkv, dh, scale,
                                   lse.data_ptr() if mode == "lse" else None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        L.check(rc, "ug_flash_attn_bwd")
        torch.cuda.synchronize()
        for n, rows in (("dq", Lq), ("dk", Lkv), ("dv", Lkv)):
            assert _sentinel_ok(outs[n], rows, D, SENT_D), (f"{n} written outside its rows / columns", mode, c)
        runs[mode] = {n: t.cpu() for n, t in outs.items()}

    # fp64 truth on the kernel's own operands; delta from the bf16 O the forward produced
    t = lambda n, rows: heads(spec[n][0], spec[n][1], spec[n][2], rows)
    o_k = heads(o_buf.cpu(), 0, 0, Lq)
    ref = BR.attention(t("q", Lq), t("k", Lkv), t("v", Lkv), t("do", Lq), scale, o=o_k, lsum_bf16=dh == 64, fwd_tile=None if data is None else 64)
    _check("forward O", o_k, ref["O"], c, var=ref["O_r" if data is None else "O_l"], rows_from=_tail(Lq))
    # base-2 LSE: fp32 scores and sums (2^-16 (1 + |lse2|) covers 256 fp32 ulps of the row sum); at head width 64 the row sum adds the bf16-rounded
    # probabilities P.V multiplies (each within 2^-9 of its value: |d log2 l| <= 2^-9 / ln 2)
    lse_k = lse[..., :Lq].double().cpu()
    tol = (2.0 ** -9 / math.log(2.0) if dh == 64 else 0.0) + 2.0 ** -16 * (1.0 + ref["lse2"].abs())
    _check_elem("forward lse2", lse_k, ref["lse2"], tol, c)
    for mode, got in runs.items():
        for n, rows in (("dq", Lq), ("dk", Lkv), ("dv", Lkv)):
            # regimes sweep: with the forward's LSE the kernels recompute P from it, so the variant does too (bwd_ref `*_rl`; at head width 64 that
            # LSE is the log of a sum of bf16-rounded probabilities, which a peaked row does not average out)
            var = ref[n + ("_rl" if data is not None and mode == "lse" else "_r")]
            if var is not ref[n + "_r"]:
                other = BR.err(ref[n + "_r"], ref[n], ref.get(n + "_m"), _tail(rows))
                print(f"bwd[{mode}] {n}: 1.5 x the *_r variant (not asserted): rel-L2 {1.5 * other[0]:.3e}, worst row {1.5 * other[1]:.3e}, tail {1.5 * other[2]:.3e}")
            _check(f"bwd[{mode}] {n}", heads(got[n], 0, 0, rows), ref[n], dict(c, mode=mode), var=var, mag=ref.get(n + "_m"), rows_from=_tail(rows))
    same = all(torch.equal(runs["lse"][n], runs["none"][n]) for n in ("dq", "dk", "dv"))
    print(f"attention {c}: backward with the forward's LSE and with lse=NULL bit-identical: {same}")
    if data is None:
        return same

    def forward_again(dtype):
        """the forward without the LSE on the same operands widened to `dtype`, into a fresh sentinel-filled output -> that buffer (on the host)"""
        cast = {i: t.to(dtype) for i, t in on_gpu.items()}
        out = torch.full_like(cast[id(spec["o"][0])], SENT_O)

        def view(name):
            t, r0, c0 = spec[name]
            return (out if name == "o" else cast[id(t)]).view(-1)[r0 * t.shape[2] + c0:]
        ops.flash_attn(view("q"), view("k"), view("v"), view("o"), batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(q_rs, q_bs),
                       k_strides=(k_rs, k_bs), v_strides=(v_rs, v_bs), o_strides=(o_rs, o_bs), scale=scale)
        torch.cuda.synchronize()
        assert _sentinel_ok(out, Lq, D, SENT_O), ("forward wrote outside its output", str(dtype), c)
        return out.cpu()

    return dict(ref=ref, o=o_k, o_buf=o_buf.cpu(), runs={m: {n: heads(t, 0, 0, Lq if n == "dq" else Lkv) for n, t in r.items()} for m, r in runs.items()},
                same=same, heads=heads, forward_again=forward_again, lse2=lse_k, k_rs=k_rs, v_rs=v_rs)


@pytest.mark.parametrize("seed", range(40))
def test_flash_attention_backward_random_shapes(gpu, seed):
    rng = random.Random(5000 + seed)
    dh = rng.choice([128, 128, 64])
    B, H = rng.choice([1, 2, 3]), rng.choice([1, 2, 3, 5])
    Lq, Lkv = rng.choice(LENGTHS), rng.choice(LENGTHS)
    if B * H * Lq * Lkv > 6_000_000:          # keep the fp64 reference of one case under ~1 s on the host
        B = 1
    _run_attention(gpu, _attn_case(rng, dh, B, H, Lq, Lkv), seed)


@pytest.mark.parametrize("name,dh,B,H,Lq,Lkv,joint", [
    ("pair_dq_below", 128, 1, 1, 2047, 2047, False),      # dh 128 below / at / above the pair-scheme dQ switch (Lq >= 2048)
    ("pair_dq_at", 128, 1, 1, 2048, 2048, True),
    ("pair_dq_above", 128, 1, 1, 2049, 2049, False),
    ("sd35_joint_dh64", 64, 1, 1, 4429, 4429, True),      # SD3.5 training: 4096 + 333 tokens at head width 64
    ("deep_queries", 128, 1, 2, 300, 2300, True),          # 300 queries deep inside 2300 keys
    ("heads24", 128, 1, 24, 333, 520, False),
])
def test_flash_attention_backward_fixed_long(gpu, name, dh, B, H, Lq, Lkv, joint):
    rng = random.Random(name)
    c = _attn_case(rng, dh, B, H, Lq, Lkv, joint)
    if name == "deep_queries":
        c["qoff"] = 1700
    _run_attention(gpu, dict(c, name=name), 77)


# ----------------------------------------------------------------------------------------------------------------------------------
# fp32 verification backward of attention: autograd.FlashAttention on fp32 tensors (the GEMM formulation, padding to 64, the row kernels)
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_attention_backward_fp32_verification_path(gpu, seed):
    from unigen_amd import autograd as A
    rng = random.Random(6000 + seed)
    dh = rng.choice([128, 128, 64])
    B, H = rng.choice([1, 2]), rng.choice([1, 2, 3])
    Lq, Lkv = rng.choice(LENGTHS[:10]), rng.choice(LENGTHS[:10])
    joint = rng.random() < 0.5 and Lq <= Lkv
    D, pad = H * dh, 8 * rng.choice([0, 1, 2])
    c = dict(dh=dh, B=B, H=H, Lq=Lq, Lkv=Lkv, joint=joint, pad=pad)
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, Lkv, 3 * D + pad, generator=g)
    Q = None if joint else torch.randn(B, Lq, D + pad, generator=g)
    qoff = rng.randint(0, Lkv - Lq) if joint else 0
    do = torch.randn(B, Lq, D, generator=g)
    Xg = X.to(gpu).requires_grad_(True)
    Qg = None if joint else Q.to(gpu).requires_grad_(True)
    q = Xg[:, qoff:qoff + Lq, :D] if joint else Qg[:, :, :D]
    out = A.attention(q, Xg[:, :, D:2 * D], Xg[:, :, 2 * D:3 * D], H)
    out.backward(do.to(gpu))
    torch.cuda.synchronize()
    hd = lambda t, L_: t.reshape(B, L_, H, dh).transpose(1, 2).double()
    qh = hd(X[:, qoff:qoff + Lq, :D] if joint else Q[:, :, :D], Lq)
    ref = BR.attention(qh, hd(X[:, :, D:2 * D], Lkv), hd(X[:, :, 2 * D:3 * D], Lkv), hd(do, Lq), dh ** -0.5, o=hd(out.detach().cpu(), Lq))
    _check("fp32 forward O", hd(out.detach().cpu(), Lq), ref["O"], c)
    gx = Xg.grad.cpu()
    gq = gx[:, qoff:qoff + Lq, :D] if joint else Qg.grad.cpu()[:, :, :D]
    if joint:                                        # rows of the key buffer outside the queries carry no q gradient
        rest = gx[..., :D].clone()
        rest[:, qoff:qoff + Lq] = 0
        assert float(rest.abs().max()) == 0.0, c
    for n, got, rows in (("dq", gq, Lq), ("dk", gx[:, :, D:2 * D], Lkv), ("dv", gx[:, :, 2 * D:3 * D], Lkv)):
        _check(f"fp32 bwd {n}", hd(got, rows), ref[n], c, mag=ref.get(n + "_m"), rows_from=_tail(rows))


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,cols,valid,groups", [(300, 200, 129, 1), (65, 1025, 1000, 3), (130, 128, 64, 24)])
def test_attention_row_kernels(gpu, dtype, rows, cols, valid, groups):
    """ug_row_lse, ug_attn_prob (valid_cols < cols: padded keys get P = 0), ug_attn_dscore and ug_rowdot (lda > groups * cols) directly."""
    from unigen_amd import ops
    g = torch.Generator().manual_seed(rows + cols)
    case = dict(dtype=str(dtype), rows=rows, cols=cols, valid=valid, groups=groups)
    scale = 0.125
    Sb = torch.randn(rows, cols + 24, generator=g) * 12
    S = Sb.to(gpu)[:, :cols]
    lse = ops.row_lse(S, scale, valid)
    torch.cuda.synchronize()
    Sd = Sb[:, :cols].double()
    ref_lse = BR.row_lse(Sd, scale, valid)
    # argument rounding (|scale S| + |lse|) u, per-thread serial sums of valid / 256 terms and an 8-level tree: 16 ulps of margin on each
    amax = (scale * Sd[:, :valid]).abs().amax(-1)
    _check_elem("row_lse", lse.double().cpu(), ref_lse, 2.0 ** -20 * (1 + amax + ref_lse.abs() + valid / 256), case)
    P = ops.attn_prob(S, lse, scale, dtype, valid)
    torch.cuda.synchronize()
    ref_P = BR.attn_prob(Sd, lse.double().cpu(), scale, valid)
    rel = 2.0 ** -20 * (1 + (scale * Sd).abs() + lse.double().cpu().abs()[:, None])
    tol = ref_P * rel + (BR.bf16_ulp(ref_P) if dtype == BF else 0)
    _check_elem("attn_prob", P, ref_P, tol, case)
    assert float(P[:, valid:].abs().max()) == 0.0 if valid < cols else True, case
    dPb = torch.randn(rows, cols + 8, generator=g)
    delta = torch.randn(rows, generator=g)
    dS = ops.attn_dscore(P, dPb.to(gpu)[:, :cols], delta.to(gpu), scale)
    torch.cuda.synchronize()
    ref_dS = BR.attn_dscore(P.double().cpu(), dPb[:, :cols].double(), delta.double(), scale)
    _check_elem("attn_dscore", dS, ref_dS, BR.bf16_ulp(ref_dS) if dtype == BF else 2.0 ** -21 * ref_dS.abs(), case)
    gc = 40 if groups == 24 else 64 * groups + 8
    a, b = (torch.randn(rows, groups * gc + 16, generator=g).to(dtype) for _ in range(2))
    out = ops.rowdot(a.to(gpu)[:, :groups * gc], b.to(gpu)[:, :groups * gc], groups)
    torch.cuda.synchronize()
    ad, bd = a[:, :groups * gc].double(), b[:, :groups * gc].double()
    mag = BR.rowdot(ad.abs(), bd.abs(), groups)
    _check_elem("rowdot", out.double().cpu(), BR.rowdot(ad, bd, groups), (gc / 64 + 8) * 2.0 ** -24 * mag, case)


# ----------------------------------------------------------------------------------------------------------------------------------
# top-1 gate, GELU(tanh), q/k RMSNorm + RoPE, AdaLN
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_moe_gate_bwd_random_shapes(gpu, seed):
    from unigen_amd import ops
    rng = random.Random(7000 + seed)
    E = rng.choice([1, 2, 3, 6, 12, 16])
    S = rng.choice([1, 3, 4, 5, 127, 128, 129, 1000, 4099])
    D = rng.choice([8, 64, 504, 512, 520, 1536, 3072])
    ld = rng.choice([D, D + 8, 2 * D])
    dt = F32 if seed % 4 == 3 else BF
    c = dict(E=E, S=S, D=D, ld=ld, dtype=str(dt))
    g = torch.Generator().manual_seed(seed)
    xb, cb = (torch.randn(S, ld, generator=g).to(dt) for _ in range(2))
    wg = (torch.randn(E, D, generator=g) * D ** -0.5).to(dt)
    gates = torch.softmax(torch.randn(S, E, generator=g) * 2, -1)
    dgates = torch.randn(S, E, generator=g)
    xg, cg = xb.to(gpu), cb.to(gpu)
    dx, dw = ops.moe_gate_bwd(gates.to(gpu), dgates.to(gpu), xg[:, :D], cg[:, :D], wg.to(gpu))
    torch.cuda.synchronize()
    ref = BR.moe_gate_bwd(gates.double(), dgates.double(), xb[:, :D], cb[:, :D], wg)
    var = lambda n: ref[n + "_r"] if dt == BF else None
    _check("gate d(x + c)", dx, ref["dx"], c, var=var("dx"), mag=ref["dx_m"], rows_from=_tail(S))
    _check("gate d wg", dw, ref["dw"], c, var=var("dw"), mag=ref["dw_m"])


def gelu_tanh_bwd_truth_and_tol(x, dy, dtype):
    """-> (fp64 dx, per-element bound) of ug_gelu_tanh_bwd on x, dy as stored in dtype (tests/test_pointwise_gpu.py applies the same bound)"""
    xd, dyd = x.double(), dy.double()
    ref, mag = BR.gelu_tanh_bwd(xd, dyd)
    # fp32: exp(-2u) of a rounded argument (relative error ~ |2u| u), the two added terms (16 ulps of their magnitudes), subnormal s below x = -9.9
    two_u = (2 * 0.7978845608 * (xd + 0.044715 * xd ** 3)).abs()
    return ref, BR.ABS_U * (1 + two_u) * mag + 2.0 ** -100 * dyd.abs() + (BR.bf16_ulp(ref) if dtype == BF else 2.0 ** -20 * ref.abs())


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("n,offset", [(1, 0), (7, 0), (8, 0), (9, 0), (4095, 0), (257 * 4096 + 3, 0), (4096, 1)])
def test_gelu_tanh_bwd_sweep(gpu, dtype, n, offset):
    """x over [-10, 10] with exact zeros; n = 8 k takes the 16-byte path, other lengths and a view one element off alignment the scalar one."""
    from unigen_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n + offset, generator=g) * 20 - 10
    x[offset::5] = 0.0
    x[-1] = -10.0
    if n > 2:
        x[offset + 1] = 10.0
    x, dy = x.to(dtype), torch.randn(n + offset, generator=g).to(dtype)
    got = ops.gelu_tanh_bwd(x.to(gpu)[offset:], dy.to(gpu)[offset:])
    torch.cuda.synchronize()
    ref, tol = gelu_tanh_bwd_truth_and_tol(x[offset:], dy[offset:], dtype)
    _check_elem("gelu_tanh_bwd", got, ref, tol, dict(n=n, offset=offset, dtype=str(dtype)))


@pytest.mark.parametrize("seed", range(16))
def test_qk_rmsnorm_rope_bwd_random_shapes(gpu, seed):
    from unigen_amd import ops
    rng = random.Random(8000 + seed)
    dh, heads = rng.choice([32, 64, 96, 128, 256]), rng.choice([1, 3, 24])
    batches, rpb = rng.choice([1, 2, 3]), rng.choice([1, 17, 64, 100, 333])
    if heads == 24:
        rpb = min(rpb, 100)
    pos_offset = rng.choice([0, 5, 100])
    with_w, with_rope = rng.random() < 0.75, rng.random() < 0.75
    if not (with_w or with_rope):
        with_w = True
    HD, rows = heads * dh, batches * rpb
    packed = rng.random() < 0.5                       # x inside a packed qkv buffer (row stride 3 H dh), dy with its own stride
    dt = F32 if seed % 4 == 3 else BF
    c = dict(dh=dh, heads=heads, batches=batches, rpb=rpb, pos_offset=pos_offset, w=with_w, rope=with_rope, packed=packed, dtype=str(dt))
    g = torch.Generator().manual_seed(seed)
    xb = torch.randn(rows, 3 * HD if packed else HD, generator=g).to(dt)
    x0 = rng.choice([0, HD]) if packed else 0
    dyb = torch.randn(rows, HD + (8 if packed else 0), generator=g).to(dt)
    w = (1 + 0.2 * torch.randn(dh, generator=g)).to(dt) if with_w else None
    ang = torch.rand(pos_offset + rpb, dh // 2, generator=g) * 6.28
    cos, sin = (ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()) if with_rope else (None, None)
    dx, dw = ops.qk_rmsnorm_rope_bwd(xb.to(gpu)[:, x0:x0 + HD], dyb.to(gpu)[:, :HD], None if w is None else w.to(gpu),
                                     None if cos is None else cos.to(gpu), None if sin is None else sin.to(gpu), rows_per_batch=rpb,
                                     pos_offset=pos_offset, heads=heads, dh=dh)
    torch.cuda.synchronize()
    ref_dx, ref_dw = BR.qk_rmsnorm_rope_bwd(xb[:, x0:x0 + HD], dyb[:, :HD], w, cos, sin, rpb, pos_offset, heads, dh)
    bf = dt == BF
    per_vec = lambda t: t.reshape(rows, heads, dh).transpose(0, 1)       # rows of a head: the tail check sees the last tile of each head
    _check("qk dx", per_vec(dx.cpu()), per_vec(ref_dx), c, var=per_vec(BR.bf16(ref_dx)) if bf else None, rows_from=_tail(rows))
    assert (dw is None) == (w is None), c
    if dw is not None:
        _check("qk dw", dw.cpu(), ref_dw, c, var=BR.bf16(ref_dw) if bf else None)


@pytest.mark.parametrize("seed", range(16))
def test_adaln_modulate_bwd_random_shapes(gpu, seed):
    from unigen_amd import ops
    rng = random.Random(9000 + seed)
    D = rng.choice([8, 520, 4096, 8 * rng.randint(1, 512), 64, 1536])
    rps = rng.choice([1, 7, 333, None])
    samples = rng.choice([1, 2, 3]) if rps != 1 else rng.choice([1, 3, 64, 700])
    if rps is None:                                   # one sample, all its rows
        samples, rps = 1, rng.choice([5, 200, 1000])
    if D * rps * samples > 3_000_000:
        samples = 1
    rows = rps * samples
    dt = F32 if seed % 4 == 3 else BF
    ldx, lddy = D + 8 * rng.choice([1, 4, 64]), D + 8 * rng.choice([0, 1])
    j = rng.randint(0, 5)
    c = dict(D=D, rps=rps, samples=samples, ldx=ldx, lddy=lddy, scale_col=j, dtype=str(dt))
    g = torch.Generator().manual_seed(seed)
    xb, dyb = torch.randn(rows, ldx, generator=g).to(dt), torch.randn(rows, lddy, generator=g).to(dt)
    mod = (0.3 * torch.randn(samples, 6 * D, generator=g)).to(dt)          # the scale is a column slice of the modulation embedding
    dx, dsh, dsc = ops.adaln_modulate_bwd(xb.to(gpu)[:, :D], dyb.to(gpu)[:, :D], mod.to(gpu)[:, j * D:(j + 1) * D], rows_per_sample=rps)
    torch.cuda.synchronize()
    r_dx, r_dsh, r_dsc = BR.adaln_modulate_bwd(xb[:, :D], dyb[:, :D], mod[:, j * D:(j + 1) * D], rps)
    bf = dt == BF
    _check("adaln dx", dx.cpu(), r_dx, c, var=BR.bf16(r_dx) if bf else None, rows_from=_tail(rows))
    _check("adaln d shift", dsh.cpu(), r_dsh, c, var=BR.bf16(r_dsh) if bf else None)
    _check("adaln d scale", dsc.cpu(), r_dsc, c, var=BR.bf16(r_dsc) if bf else None)


# ----------------------------------------------------------------------------------------------------------------------------------
# colsum and the Linear backward (dW through zero-padded transposes to pad64(M))
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,cols,rpg,with_b,alpha", [(1, 8, None, False, 1.0), (300, 520, 100, True, 0.5), (4099, 192, None, True, -1.25),
                                                        (777, 1032, 7, False, 3.0)])
def test_colsum_sweep(gpu, dtype, rows, cols, rpg, with_b, alpha):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(rows + cols)
    a = torch.randn(rows, cols + 8, generator=g).to(dtype)
    b = torch.randn(rows, cols, generator=g).to(dtype) if with_b else None
    got = ops.colsum(a.to(gpu)[:, :cols], None if b is None else b.to(gpu), rows_per_group=rpg, alpha=alpha)
    torch.cuda.synchronize()
    ref = BR.colsum(a[:, :cols], b, rpg, alpha)
    _check("colsum", got.cpu(), ref, dict(rows=rows, cols=cols, rpg=rpg, b=with_b, alpha=alpha, dtype=str(dtype)),
           var=BR.bf16(ref) if dtype == BF else None)


@pytest.mark.parametrize("M", [1, 7, 65, 777, 4099])
@pytest.mark.parametrize("res_scale", [False, True])
def test_linear_backward_sweep(gpu, M, res_scale):
    from unigen_amd import autograd as A
    rng = random.Random(M * 2 + res_scale)
    N, K = 64 * rng.choice([1, 2, 5]), 64 * rng.choice([1, 3, 4])
    dt = F32 if M == 65 and res_scale else BF
    alpha = 0.7 if res_scale else 1.0
    c = dict(M=M, N=N, K=K, res_scale=res_scale, alpha=alpha, dtype=str(dt))
    g = torch.Generator().manual_seed(M)
    x, w, b = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) * K ** -0.5).to(dt), (0.1 * torch.randn(N, generator=g)).to(dt)
    r, dy = torch.randn(M, N, generator=g).to(dt), torch.randn(M, N, generator=g).to(dt)
    xg, wg, bg = (t.to(gpu).requires_grad_(True) for t in (x, w, b))
    rg = r.to(gpu).requires_grad_(True)
    y = A.linear_res_scale(rg, xg, wg, bg, alpha) if res_scale else A.linear(xg, wg, bg)
    y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    du = (dy * alpha) if res_scale else dy                # the backward's d(linear) = alpha * dy, a bf16 tensor op: the operand the GEMMs see
    r_dx, r_dw, r_db = BR.linear_bwd(x, w, du)
    bf = dt == BF
    if res_scale:
        assert torch.equal(rg.grad.cpu(), dy), c
    _check("linear dx", xg.grad.cpu(), r_dx, c, var=BR.bf16(r_dx) if bf else None, rows_from=_tail(M))
    _check("linear dW", wg.grad.cpu(), r_dw, c, var=BR.bf16(r_dw) if bf else None, rows_from=_tail(N))
    _check("linear db", bg.grad.cpu(), r_db, c, var=BR.bf16(r_db) if bf else None)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("adjacent", [True, False])
@pytest.mark.parametrize("M", [7, 65])
def test_linear_n_backward(gpu, M, adjacent, dtype):
    """autograd.linear_n directly: three projections of one x, K = 128, N = (64, 128, 64); M = 65 is one full 64-row tile plus one row (wgrad pads to
    128). adjacent: the weights / biases are row blocks of one [256, 128] / [256] buffer (the packed launch); otherwise separate allocations (one
    launch per projection). dy reaches projections 0 and 2 only: dx = dy_0 w_0 + dy_2 w_2, accumulated in launch order (the bf16 variant rounds
    each launch's output); projection 1 gets no gradient."""
    from unigen_amd import autograd as A
    K, Ns = 128, (64, 128, 64)
    rows = [slice(sum(Ns[:i]), sum(Ns[:i + 1])) for i in range(3)]
    c = dict(M=M, adjacent=adjacent, dtype=str(dtype))
    g = torch.Generator().manual_seed(100 + M)
    x = torch.randn(M, K, generator=g).to(dtype)
    W, Bv = (torch.randn(sum(Ns), K, generator=g) * K ** -0.5).to(dtype), (0.1 * torch.randn(sum(Ns), generator=g)).to(dtype)
    dys = {i: torch.randn(M, Ns[i], generator=g).to(dtype) for i in (0, 2)}
    xg = x.to(gpu).requires_grad_(True)
    if adjacent:                                         # separate leaves whose storage is one buffer, as engine._pack leaves q / k / v
        Wg, Bg = W.to(gpu), Bv.to(gpu)
        ws, bs = [Wg[r].detach().requires_grad_(True) for r in rows], [Bg[r].detach().requires_grad_(True) for r in rows]
    else:                                                # one allocation each, with a spare row / element behind it: never back to back
        spare = lambda t: torch.cat([t, t[:1]]).to(gpu)[:t.shape[0]].detach().requires_grad_(True)
        ws, bs = [spare(W[r]) for r in rows], [spare(Bv[r]) for r in rows]
    back_to_back = all(b.data_ptr() == a.data_ptr() + a.numel() * a.element_size() for a, b in zip(ws[:-1], ws[1:]))
    assert back_to_back == adjacent, c
    outs = A.linear_n(xg, ws, bs)
    torch.autograd.backward([outs[0], outs[2]], [dys[0].to(gpu), dys[2].to(gpu)])
    torch.cuda.synchronize()
    bf = dtype == BF
    var = lambda t: BR.bf16(t) if bf else None
    for i, r in enumerate(rows):
        y = x.double() @ W[r].double().t() + Bv[r].double()
        _check(f"linear_n y{i}", outs[i].detach().cpu(), y, c, var=var(y), rows_from=_tail(M))
    refs = {i: BR.linear_bwd(x, W[rows[i]], dys[i]) for i in (0, 2)}
    dx = refs[0][0] + refs[2][0]
    _check("linear_n dx", xg.grad.cpu(), dx, c, var=BR.bf16(BR.bf16(refs[0][0]) + BR.bf16(refs[2][0])) if bf else None, rows_from=_tail(M))
    for i in (0, 2):
        _check(f"linear_n dW{i}", ws[i].grad.cpu(), refs[i][1], c, var=var(refs[i][1]), rows_from=_tail(Ns[i]))
        _check(f"linear_n db{i}", bs[i].grad.cpu(), refs[i][2], c, var=var(refs[i][2]))
    for p in (ws[1], bs[1]):                             # no dy reached projection 1
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, c


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("M", [7, 65])
def test_linear_cat2_backward(gpu, M, dtype):
    """autograd.linear_cat2 directly: F.linear(cat([a, m], -1), w, b) with Ka = 128, Km = 256, N = 64 against the Linear backward over the
    materialised concatenation, split at column Ka."""
    from unigen_amd import autograd as A
    Ka, Km, N = 128, 256, 64
    c = dict(M=M, dtype=str(dtype))
    g = torch.Generator().manual_seed(200 + M)
    a, m = torch.randn(M, Ka, generator=g).to(dtype), torch.randn(M, Km, generator=g).to(dtype)
    w, b = (torch.randn(N, Ka + Km, generator=g) * (Ka + Km) ** -0.5).to(dtype), (0.1 * torch.randn(N, generator=g)).to(dtype)
    dy = torch.randn(M, N, generator=g).to(dtype)
    ag, mg, wg, bg = (t.to(gpu).requires_grad_(True) for t in (a, m, w, b))
    y = A.linear_cat2(ag, mg, wg, bg)
    y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    am = torch.cat([a, m], 1)
    r_y = am.double() @ w.double().t() + b.double()
    r_dx, r_dw, r_db = BR.linear_bwd(am, w, dy)
    var = lambda t: BR.bf16(t) if dtype == BF else None
    _check("linear_cat2 y", y.detach().cpu(), r_y, c, var=var(r_y), rows_from=_tail(M))
    _check("linear_cat2 da", ag.grad.cpu(), r_dx[:, :Ka], c, var=var(r_dx[:, :Ka]), rows_from=_tail(M))
    _check("linear_cat2 dm", mg.grad.cpu(), r_dx[:, Ka:], c, var=var(r_dx[:, Ka:]), rows_from=_tail(M))
    _check("linear_cat2 dw", wg.grad.cpu(), r_dw, c, var=var(r_dw), rows_from=_tail(N))
    _check("linear_cat2 db", bg.grad.cpu(), r_db, c, var=var(r_db))
