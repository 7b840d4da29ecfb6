"""Seeded random-shape sweeps of the forward projection paths against the float64 references of tests/fwd_ref.py (themselves checked against
the oracle's formulations by tests/test_fwd_ref_cpu.py): the stand-alone q/k RMSNorm + RoPE pass (ug_qk_rmsnorm_rope and its _f32 twin), the
GEMM's fused q/k epilogue (UG_EPI_QKV_ROPE) in its single-block and double-block forms, and the GEMM's LoRA K-segment under every epilogue in
both tile kernels; plus the engine's fall-back where the fused epilogue refuses a geometry.

Tolerances (docs/PARITY_TOLERANCES.md, "Forward projection sweep"):
  - fp32 twins: rel-L2 <= 1e-5 against the fp64 truth, every row <= 1e-4.
  - bf16: rel-L2 <= max(1.5 x the error of fwd_ref's rounding-point variant against the same truth, 2^-9), and the same bound from the
    variant's own worst row on the worst (row, head) vector of q / k or the worst row of a GEMM output, and separately on the rows of the last
    partial tile (64 rows for the q/k pass, 256 for the GEMMs).
Every element a call must not write (v columns, leading-dimension padding, the gap rows of a batch stride or row map, the column split's gap,
the joint buffer's context rows) is compared bit for bit with its value before the call: out-of-bounds writes are looked for with in-bounds
sentinels, never by provoking a fault."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from tests import fwd_ref as FR

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FLOOR = 2.0 ** -9
F32_TOTAL, F32_ROW = 1e-5, 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds(var, truth, rows_from):
    return tuple(max(1.5 * e, FLOOR) for e in FR.err(var, truth, rows_from=rows_from))


def _check(name, got, truth, case, var=None, rows_from=None):
    """rel-L2, worst row, worst tail row of `got` against the fp64 truth: bf16 (var given) within max(1.5 x var's own, FLOOR), fp32 absolute."""
    k = FR.err(got, truth, rows_from=rows_from)
    bounds = (F32_TOTAL, F32_ROW, F32_ROW) if var is None else _bounds(var, truth, rows_from)
    print(f"{name}: rel-L2 {k[0]:.3e} (bound {bounds[0]:.3e}), worst row {k[1]:.3e} ({bounds[1]:.3e}), tail {k[2]:.3e} ({bounds[2]:.3e})")
    for what, e, b in zip(("rel-L2", "worst row", "worst row of the partial tile"), k, bounds):
        assert e <= b, (name, what, e, b, case)
    return k


def _tail(rows, tile):
    return None if rows % tile == 0 else rows // tile * tile


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_qk_rmsnorm_rope (bf16 and _f32)
# ----------------------------------------------------------------------------------------------------------------------------------
def _qk_case(rng):
    dh = rng.choice([64, 128])
    heads = rng.choice([1, 2, 3, 5, 8, 24])
    B = rng.randint(1, 3)
    L = rng.choice([1, 63, 65, 200, 1000, 1037])
    while B * L * heads > 50000:
        heads = max(1, heads // 2)
    q_off = rng.choice([-1, 0, 0, 16])
    if q_off >= 0:
        k_off = q_off + heads * dh + rng.choice([0, 0, 8, 64])
    else:
        k_off = rng.choice([0, 8, 128])
    ld = k_off + heads * dh + heads * dh + rng.choice([0, 8, 40])        # v heads behind k, then padding
    pos_offset = rng.choice([0, 0, 5, 512])
    return dict(dh=dh, heads=heads, B=B, L=L, bstride=L + rng.choice([0, 0, 3, 17]), pos_offset=pos_offset, q_off=q_off, k_off=k_off, ld=ld,
                split=rng.choice([0, pos_offset + L // 2, pos_offset + L + 10 ** 6]), sides=rng.choice(["both", "both", "a", "b", "none"]),
                rope=rng.random() < 0.75)


@pytest.mark.parametrize("seed", range(16))
def test_qk_rmsnorm_rope_random_shapes(gpu, seed):
    from unigen_amd import ops
    c = _qk_case(random.Random(seed))
    g = torch.Generator().manual_seed(1000 + seed)
    dh, H, B, L, bs = c["dh"], c["heads"], c["B"], c["L"], c["bstride"]
    phys = (torch.arange(B)[:, None] * bs + torch.arange(L)).flatten()
    buf = FR.spread_rows(g, B * bs + 2, c["ld"], zero_row=int(phys[len(phys) // 2]))
    wq_a, wq_b = FR.norm_weights(g, dh)
    wk_a, wk_b = FR.norm_weights(g, dh)
    if c["sides"] in ("b", "none"):
        wq_a = wk_a = None
    if c["sides"] in ("a", "none"):
        wq_b = wk_b = None
    cos, sin, _ = FR.rope_tables(g, c["pos_offset"] + L, dh) if c["rope"] else (None, None, None)
    kw = dict(batches=B, rows_per_batch=L, batch_stride_rows=bs, pos_offset=c["pos_offset"], q_off=c["q_off"], k_off=c["k_off"], heads=H, dh=dh,
              split=c["split"])
    ws = dict(wq_a=wq_a, wk_a=wk_a, wq_b=wq_b, wk_b=wk_b)
    exact, var = FR.qk_rmsnorm_rope(buf, cos=cos, sin=sin, **ws, **kw)
    touched = torch.zeros_like(buf, dtype=torch.bool)
    for off in (c["q_off"], c["k_off"]):
        if off >= 0:
            touched[phys[:, None], torch.arange(off, off + H * dh)[None, :]] = True
    vec = lambda t: FR.qk_vectors(t, phys, c["q_off"], c["k_off"], H, dh)
    for dt in (BF, F32):
        gb = buf.to(dt).to(gpu)
        dev = lambda t: None if t is None else t.to(dt).to(gpu)
        ops.qk_rmsnorm_rope(gb, ld=c["ld"], cos=None if cos is None else cos.to(gpu), sin=None if sin is None else sin.to(gpu),
                            **{k: dev(v) for k, v in ws.items()}, **kw)
        torch.cuda.synchronize()
        got = gb.cpu()
        assert torch.equal(got[~touched], buf.to(dt)[~touched]), ("written outside the q / k heads of its rows", dt, c)
        assert not got[buf.abs().sum(1) == 0].any(), ("the all-zero row is not exactly zero", dt, c)
        name = f"qk_rmsnorm_rope {str(dt)[6:]} seed {seed}"
        _check(name, vec(got), vec(exact), c, var=vec(var) if dt == BF else None, rows_from=_tail(B * L, 64))


# ----------------------------------------------------------------------------------------------------------------------------------
# UG_EPI_QKV_ROPE: the fused q/k epilogue
# ----------------------------------------------------------------------------------------------------------------------------------
def _qkv_case(rng):
    while True:
        single = rng.random() < 0.5
        D = rng.choice([256, 512, 768, 1536])
        dh, rope = rng.choice([(128, True), (64, True), (64, False)])
        K = rng.choice([64, 128, 320, 512, 1024])
        if single:                     # single block: positions per sample Lj, possibly not a multiple of 256 (tiles straddle samples)
            Lj, B = rng.choice([(256, 1), (320, 4), (384, 2), (448, 4), (1280, 1)])
            Ls, Lc, M, N = Lj, 0, B * Lj, 7 * D
        else:                          # double block sample rows: C row map into the joint buffer, positions from Lc
            Ls, B = rng.choice([(256, 1), (256, 3), (512, 2)])
            Lc = rng.choice([24, 77, 256])
            M, N = B * Ls, 3 * D
        if M * N * K <= 6e8:
            break
    a_pad = rng.choice([0, 0, 13])     # a monotonic A row map: rows per batch Ls, batch stride Ls + a_pad
    return dict(single=single, D=D, dh=dh, rope=rope, K=K, B=B, Ls=Ls, Lc=Lc, M=M, N=N, a_pad=a_pad)


@pytest.mark.parametrize("seed", range(10))
def test_qkv_rope_epilogue_random_shapes(gpu, seed):
    from unigen_amd import lib as L, ops
    c = _qkv_case(random.Random(seed))
    g = torch.Generator().manual_seed(2000 + seed)
    D, dh, K, B, Ls, Lc, M, N = c["D"], c["dh"], c["K"], c["B"], c["Ls"], c["Lc"], c["M"], c["N"]
    H = D // dh
    a_map = (Ls, Ls + c["a_pad"]) if c["a_pad"] else (0, 0)
    a = FR.spread_rows(g, B * (Ls + c["a_pad"]), K)
    w = FR.bf16(torch.randn(N, K, generator=g, dtype=F64) * K ** -0.5)
    b = FR.bf16(0.1 * torch.randn(N, generator=g, dtype=F64))
    wq, wk = FR.norm_weights(g, dh)[0], FR.norm_weights(g, dh)[0]             # one weight per projection (no text / image sides)
    cos, sin, cs = FR.rope_tables(g, Lc + Ls, dh)
    if not c["rope"]:
        cos = sin = cs = None
    if c["single"]:
        Lj, ldc, rows = Ls, 8 * D, M
        kw = dict(gelu_from_n=3 * D, c_shift_from_n=3 * D, c_shift=D)
        c_map, pos0 = (0, 0), 0
    else:
        Lj, ldc, rows = Lc + Ls, 3 * D, B * (Lc + Ls)
        kw = {}
        c_map, pos0 = (Ls, Lc + Ls), Lc
    junk = FR.bf16(torch.randn(rows, ldc, generator=g, dtype=F64))
    off = Lc if not c["single"] else 0                                          # the launch's C base: row Lc of the joint buffer
    exact, var = (torch.cat([junk[:off], t]) for t in FR.qkv_rope_gemm(a, w, b, junk[off:], M=M, wq=wq, wk=wk, cs=cs, rope_rpb=Ls, pos0=pos0,
                                                                        qk_until_n=2 * D, dh=dh, a_map=a_map, c_map=c_map, **kw))
    ad, wd, bd, wqd, wkd = (t.to(BF).to(gpu) for t in (a, w, b, wq, wk))
    cmap = ops.RowMap(*c_map)
    amap = ops.RowMap(*a_map)

    def launch(qk):
        buf = junk.to(BF).to(gpu)
        ops.gemm(ad, wd, bd, buf[off:], M=M, ldc=ldc, a_map=amap, c_map=cmap, epilogue=L.EPI_BIAS_GELU if c["single"] else L.EPI_BIAS,
                 qk_rope=ops.QkRope(wqd, wkd, None if cs is None else cs.to(gpu), Ls, pos0, 2 * D, dh=dh) if qk else None, **kw)
        return buf

    one, plain = launch(True), launch(False)
    two = plain.clone()
    tab = dict(cos=cos.to(gpu), sin=sin.to(gpu)) if cs is not None else {}
    ops.qk_rmsnorm_rope(two[off:], batches=B, rows_per_batch=Ls, batch_stride_rows=Lj if not c["single"] else Ls, pos_offset=pos0, ld=ldc, q_off=0,
                        k_off=D, heads=H, dh=dh, wq_b=wqd, wk_b=wkd, split=0, **tab)
    torch.cuda.synchronize()
    one, plain, two = one.cpu(), plain.cpu(), two.cpu()
    m = torch.arange(M)
    prow = FR.rowmap(m, *c_map) + off                                           # physical rows of the logical rows
    qk = torch.zeros(rows, ldc, dtype=torch.bool)
    qk[prow[:, None], torch.arange(2 * D)[None, :]] = True
    # everything but the q / k heads: bit-identical to the same launch without the fused epilogue (v / mlp columns, the attention slot's gap,
    # the joint buffer's context rows); and those untouched elements still hold the sentinels
    assert torch.equal(one[~qk], plain[~qk]), ("v / mlp columns or untouched elements differ from the plain launch", c)
    written = torch.zeros(rows, ldc, dtype=torch.bool)
    written[prow[:, None], torch.arange(N)[None, :] + (D * (torch.arange(N) >= 3 * D) if c["single"] else 0)] = True
    assert torch.equal(one[~written], junk.to(BF)[~written]), ("written outside its rows / columns", c)
    name = f"qkv_rope seed {seed} ({'single' if c['single'] else 'double'}, D {D}, dh {dh}, K {K}, M {M})"
    vec = lambda t: FR.qk_vectors(t, prow, 0, D, H, dh)
    k1 = _check(name + " q/k", vec(one), vec(exact), c, var=vec(var), rows_from=M - 256)
    vcols = torch.cat([torch.arange(2 * D, 3 * D), torch.arange(4 * D, 8 * D)]) if c["single"] else torch.arange(2 * D, 3 * D)
    sel = lambda t: t[prow][:, vcols]
    _check(name + " v/mlp", sel(one), sel(exact), c, var=sel(var), rows_from=M - 256)
    # the fused epilogue is as close to the truth as the two-launch path (GEMM, then ug_qk_rmsnorm_rope)
    k2 = FR.err(vec(two), vec(exact))
    print(f"{name}: two-launch rel-L2 {k2[0]:.3e}")
    assert k1[0] <= 1.05 * k2[0] + 1e-5, (k1[0], k2[0], c)


# ----------------------------------------------------------------------------------------------------------------------------------
# LoRA K-segment: both tile kernels, every epilogue, row maps, the column split; one child (UG_GEMM_FORCE_TILE is read per call only with
# UG_ENV_DYNAMIC=1)
# ----------------------------------------------------------------------------------------------------------------------------------
LORA_CASES = [   # M, N, K, rank, padded rank, epilogue, A map, C map, column split (gelu / shift from, shift), cancel
    (300, 1000, 64, 40, 64, FR.EPI_BIAS, None, None, None, False),
    (1000, 1284, 128, 64, 128, FR.EPI_BIAS, (250, 300), (250, 260), None, False),
    (2049, 520, 192, 100, 192, FR.EPI_BIAS_GELU, None, None, None, False),
    (1537, 1792, 128, 128, 128, FR.EPI_BIAS_GELU, (512, 520), None, (768, 256), False),
    (1000, 1280, 320, 200, 256, FR.EPI_RES_GATE, (500, 0), (500, 510), None, False),         # broadcasting A map (bstride < rpb)
    (4000, 200, 128, 64, 64, FR.EPI_RES_SCALE, (1000, 400), (1000, 1000), None, False),       # R aliased to C; broadcasting A map
    (777, 1024, 64, 128, 128, FR.EPI_BIAS, None, None, None, True),                           # LoRA cancels 98 % of A W^T
    (2304, 768, 128, 160, 192, FR.EPI_RES_GATE, (256, 256), (768, 800), None, True),
    (513, 2048, 256, 256, 256, FR.EPI_BIAS_GELU, None, (171, 180), (512, 8), False),
]


def _lora_child():
    """runs in a child process with UG_ENV_DYNAMIC=1: every LORA_CASES entry with UG_GEMM_FORCE_TILE = 128, 256, 0 and through ug_gemm_f32;
    prints one JSON record per case"""
    from unigen_amd import lib as L, ops
    dev = torch.device("cuda:0")
    for i, (M, N, K, r, rp, epi, amap, cmap, split, cancel) in enumerate(LORA_CASES):
        g = torch.Generator().manual_seed(3000 + i)
        a, w, b, t, lb = FR.lora_operands(g, M, N, K, r, rp, cancel=cancel)
        amap, cmap = amap or (0, 0), cmap or (0, 0)
        a_rows = M if amap[0] == 0 else (M - 1) // amap[0] * amap[1] + amap[0]
        a_phys = FR.bf16(torch.randn(a_rows, K + 8, generator=g, dtype=F64))            # lda = K + 8
        a_phys[FR.rowmap(torch.arange(M), *amap), :K] = a                               # (a broadcasting map reads some rows twice: last write wins)
        a = a_phys[FR.rowmap(torch.arange(M), *amap), :K]
        gelu_from, shift = split if split else (0, 0)
        ldc = N + shift + 8
        c_rows = M if cmap[0] == 0 else (M - 1) // cmap[0] * cmap[1] + cmap[0]
        out0 = FR.bf16(torch.randn(c_rows + 1, ldc, generator=g, dtype=F64))
        t_buf = torch.zeros(M, rp + 8, dtype=F64); t_buf[:, :rp] = t                  # ldt > r
        b_buf = torch.zeros(N, rp + 24, dtype=F64); b_buf[:, :rp] = lb
        rps = cmap[0] or M
        gate = FR.bf16(torch.randn((M + rps - 1) // rps, N, generator=g, dtype=F64))
        kw = dict(M=M, epilogue=epi)
        ref_kw = dict(kw, t=t, lb=lb, a_map=amap, c_map=cmap)
        if split:
            kw.update(gelu_from_n=gelu_from, c_shift_from_n=gelu_from, c_shift=shift)
            ref_kw.update(gelu_from_n=gelu_from, c_shift_from_n=gelu_from, c_shift=shift)
        if epi in (FR.EPI_RES_GATE, FR.EPI_RES_SCALE):
            ref_kw.update(residual=out0, r_map=cmap, gate=gate, rows_per_sample=rps, alpha=0.7)
        exact, var = FR.lora_gemm(a_phys, w, b, out0, **ref_kw)
        rows = FR.rowmap(torch.arange(M), *cmap)
        cols = torch.arange(N) + (shift * (torch.arange(N) >= gelu_from) if split else 0)
        written = torch.zeros_like(out0, dtype=torch.bool)
        written[rows[:, None], cols[None, :]] = True
        logical = lambda o: o[rows[:, None], cols[None, :]]

        def run(dt):
            d = lambda x: x.to(dt).to(dev)
            out = d(out0)
            extra = {}
            if epi in (FR.EPI_RES_GATE, FR.EPI_RES_SCALE):
                extra = dict(residual=out, r_map=ops.RowMap(*cmap), alpha=0.7)                  # R aliases C
                if epi == FR.EPI_RES_GATE:
                    extra.update(gate=d(gate), gate_ld=N, rows_per_sample=rps)
            ops.gemm(d(a_phys), d(w), d(b), out, lda=K + 8, a_map=ops.RowMap(*amap), c_map=ops.RowMap(*cmap), lora_t=d(t_buf)[:, :rp],
                     lora_b=d(b_buf)[:, :rp], **kw, **extra)
            torch.cuda.synchronize()
            return out.cpu()

        outs = {}
        for tile in ("128", "256", "0"):
            os.environ["UG_GEMM_FORCE_TILE"] = tile
            outs[tile] = run(BF)
        os.environ.pop("UG_GEMM_FORCE_TILE")
        rec = dict(case=i, M=M, N=N, K=K, r=r, rp=rp, epi=epi, cancel=cancel,
                   same=all(torch.equal(outs[k], outs["128"]) for k in outs),
                   untouched=all(torch.equal(o[~written], out0.to(BF)[~written]) for o in outs.values()),
                   err=FR.err(logical(outs["256"]), logical(exact), rows_from=_tail(M, 256) or M - 256),
                   bound=_bounds(logical(var), logical(exact), _tail(M, 256) or M - 256))
        if not cancel:                 # (the fp32 twin's accumulation error grows 50 x where the LoRA term cancels A W^T)
            o32 = run(F32)
            rec["f32"] = FR.err(logical(o32), logical(exact), rows_from=_tail(M, 256) or M - 256)
            rec["f32_untouched"] = bool(torch.equal(o32[~written], out0.float()[~written]))
        print("LORA " + json.dumps(rec), flush=True)


def test_lora_segment_random_shapes(gpu):
    env = dict(os.environ, UG_ENV_DYNAMIC="1")
    p = subprocess.run([sys.executable, "-c", "from tests.test_fuzz_forward_gpu import _lora_child; _lora_child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("LORA ")]
    assert len(recs) == len(LORA_CASES)
    for r in recs:
        e, bnd = r["err"], r["bound"]
        print(f"lora case {r['case']} (M {r['M']} N {r['N']} K {r['K']} r {r['r']}/{r['rp']} epi {r['epi']} cancel {r['cancel']}): "
              f"rel-L2 {e[0]:.3e} ({bnd[0]:.3e}) worst row {e[1]:.3e} ({bnd[1]:.3e}) tail {e[2]:.3e} ({bnd[2]:.3e})" +
              (f"; f32 {r['f32'][0]:.3e} / {r['f32'][1]:.3e}" if "f32" in r else ""))
        assert r["same"], ("128^2 and 256^2 kernels differ", r)
        assert r["untouched"] and r.get("f32_untouched", True), ("written outside its rows / columns", r)
        for what, x, y in zip(("rel-L2", "worst row", "worst row of the partial tile"), e, bnd):
            assert x <= y, (what, x, y, r)
        if "f32" in r:
            assert r["f32"][0] <= F32_TOTAL and r["f32"][1] <= F32_ROW and r["f32"][2] <= F32_ROW, r


# ----------------------------------------------------------------------------------------------------------------------------------
# the engine's fusion decision: geometries the fused epilogue refuses run the stand-alone pass
# ----------------------------------------------------------------------------------------------------------------------------------
def test_engine_falls_back_where_the_fused_epilogue_refuses(gpu, monkeypatch):
    """A FLUX double block at D = 3072, 24 heads, Ls = 448, B = 8 (504 tiles: one full round; Ls not a multiple of 256 - the C row map into
    the joint buffer would split tiles) and an SD3.5 dual block whose attn2 runs at Ls = 128 < 256, B = 32 (288 tiles): both ran into
    UG_ERR_UNSUPPORTED / UG_ERR_BAD_SHAPE from the fused launch before qk_rope_fusable knew the row maps. Each must run, and be bit-identical to
    the same call with the fused epilogue switched off (UG_GEMM_FUSE_QKROPE=0)."""
    from unigen_amd.engine import _Stream
    from unigen_amd.flux import UniGenFlux
    from unigen_amd.sd3 import UniGenSD3
    monkeypatch.delenv("UG_GEMM_FUSE_QKROPE", raising=False)
    g = torch.Generator(device=gpu).manual_seed(5)
    rn = lambda *s: (torch.randn(*s, generator=g, device=gpu)).to(BF)

    def twice(run):
        outs = []
        for env in ("1", "0"):
            monkeypatch.setenv("UG_GEMM_FUSE_QKROPE", env)
            outs.append(run())
            torch.cuda.synchronize()
        monkeypatch.delenv("UG_GEMM_FUSE_QKROPE")
        return outs

    # FLUX double block
    D, B, Ls, Lc = 3072, 8, 448, 64
    model = UniGenFlux.from_config(dict(num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=24, joint_attention_dim=64,
                                        pooled_projection_dim=64), device=gpu, dtype=BF)
    model.init_synthetic_(seed=2, std=0.02, bias_std=0.02)
    x, e, temb = rn(B * Ls, D), rn(B * Lc, D), rn(B, D)
    img = torch.stack([torch.zeros(Ls), torch.arange(Ls) // 16, torch.arange(Ls) % 16], 1).to(gpu)
    rope = model._rope([torch.zeros(Lc, 3, device=gpu), img], None)

    def flux():
        xs, es = x.clone(), e.clone()
        model._emb_tab.clear()
        model._double_block("transformer_blocks.0", B, _Stream(xs, Ls), _Stream(xs, Ls), _Stream(es, Lc), _Stream(es, Lc), temb, rope, "base")
        return xs, es

    (x1, e1), (x2, e2) = twice(flux)
    assert torch.equal(x1, x2) and torch.equal(e1, e2) and x1.isfinite().all()
    del model
    # SD3.5 dual block: attn2 over the sample stream at Ls = 128
    D, B, Ls, Lc = 1536, 32, 128, 24
    sd3 = UniGenSD3.from_config(dict(sample_size=16, num_layers=1, attention_head_dim=64, num_attention_heads=24, joint_attention_dim=64,
                                     caption_projection_dim=D, pooled_projection_dim=64, pos_embed_max_size=16, dual_attention_layers=[0]),
                                device=gpu, dtype=BF)
    sd3.init_synthetic_(seed=3, std=0.02, bias_std=0.02)
    x, e, temb = rn(B * Ls, D), rn(B * Lc, D), rn(B, D)

    def sd3_block():
        xs, es = x.clone(), e.clone()
        sd3._emb_tab.clear()
        sd3._double_block("transformer_blocks.0", B, _Stream(xs, Ls), _Stream(xs, Ls), _Stream(es, Lc), None, temb, None, "base", dual=True,
                          ctx_continuous=True)          # the last block: context_pre_only, as UniGenSD3.forward calls it
        return xs

    y1, y2 = twice(sd3_block)
    assert torch.equal(y1, y2) and y1.isfinite().all()
