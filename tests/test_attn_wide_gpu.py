"""ug_flash_attn_fwd_wide and ug_flash_attn_fwd_wide_f32 (csrc/attn_wide.hip: flash attention forward at head width 512) through the C ABI, against
the float64 reference of tests/attn_wide_ref.py (checked on the host by tests/test_attn_wide_ref_cpu.py over the same case ids).

Every case runs in three layouts - q, k, v in buffers of their own (row stride H 512); packed into one buffer (row stride 3 H 512: 1536 for one head);
packed with 8 pad columns (1544) - with spare rows behind every sample, so a batch stride is never L x the row stride. Every element of the operand
buffers that is not an operand is NaN; the output buffer is pre-filled with a sentinel that must survive outside the [Lq, H 512] window.
Bounds (docs/PARITY_TOLERANCES.md, "Flash attention at head width 512"): bf16 rel-L2 over the tensor AND the worst query row within
max(1.5 x err(O_v), 2^-9), the same again on the rows a peaked regime acts on; the fp32 twin on the widened operands within 1e-5 / 1e-4 (the bounds
test_fuzz_attention_gpu applies to ug_flash_attn_fwd_f32); all outputs finite; a second launch into the same output bit-identical."""
import pytest
import torch

from tests import attn_wide_ref as WR
from tests import bwd_ref as BR

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
F32_TOTAL, F32_ROW = 1e-5, 1e-4
SENT = 3.0
LAYOUTS = ("separate", "packed", "packed_pad8")
SPARE_Q, SPARE_KV, SPARE_O = 2, 3, 1          # spare rows behind every sample


def _flat(t):
    """[B, H, L, 512] -> [B, L, H 512]"""
    B, H, L_, dh = t.shape
    return t.transpose(1, 2).reshape(B, L_, H * dh)


def _build(d, layout, dtype, dev):
    """-> dict(q, k, v: (base tensor, row stride, batch stride), o: the sentinel-filled output buffer [B, Lq + spare, H 512 + 8])"""
    B, H, Lq, Lkv = d["B"], d["H"], d["Lq"], d["Lkv"]
    D = H * WR.DH
    nan = float("nan")
    q, k, v = (_flat(d[n]).to(dtype) for n in "qkv")
    if layout == "separate":
        Q = torch.full((B, Lq + SPARE_Q, D), nan, dtype=dtype)
        K = torch.full((B, Lkv + SPARE_KV, D), nan, dtype=dtype)
        V = torch.full((B, Lkv + SPARE_KV, D), nan, dtype=dtype)
        Q[:, :Lq], K[:, :Lkv], V[:, :Lkv] = q, k, v
        Q, K, V = Q.to(dev), K.to(dev), V.to(dev)
        views = dict(q=Q, k=K, v=V)
    else:
        W = 3 * D + (8 if layout == "packed_pad8" else 0)
        X = torch.full((B, max(Lq, Lkv) + SPARE_KV, W), nan, dtype=dtype)
        X[:, :Lq, :D], X[:, :Lkv, D:2 * D], X[:, :Lkv, 2 * D:3 * D] = q, k, v
        X = X.to(dev)
        views = dict(q=X, k=X[0, 0, D:], v=X[0, 0, 2 * D:])
        Q = K = V = X
    out = dict(q=(views["q"], Q.stride(1), Q.stride(0)), k=(views["k"], K.stride(1), K.stride(0)), v=(views["v"], V.stride(1), V.stride(0)))
    out["o"] = torch.full((B, Lq + SPARE_O, D + 8), SENT, dtype=dtype, device=dev)
    return out


def _launch(fn, d, buf):
    o = buf["o"]
    args = []
    for n in "qkv":
        t, rs, bs = buf[n]
        args += [t.data_ptr(), rs, bs]
    from unigen_amd import lib as ULIB
    ULIB.check(fn(*args, o.data_ptr(), o.stride(1), o.stride(0), d["B"], d["H"], d["Lq"], d["Lkv"], WR.DH, d["scale"],
                  torch.cuda.current_stream().cuda_stream), "flash_attn_fwd_wide")


def _window(d, o):
    """the output window as [B, H, Lq, 512] on the host, and whether the sentinel is intact everywhere else"""
    B, H, Lq = d["B"], d["H"], d["Lq"]
    D = H * WR.DH
    oc = o.detach().cpu()
    rest = oc.clone()
    rest[:, :Lq, :D] = SENT
    return oc[:, :Lq, :D].reshape(B, Lq, H, WR.DH).transpose(1, 2), bool((rest == SENT).all())


@pytest.mark.parametrize("case_id", WR.case_ids())
def test_wide_forward_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d, ref = WR.case_data(case_id), WR.case_reference(case_id)
    b_total, b_row = WR.bounds(ref)
    rows = d["rows"]
    for layout in LAYOUTS:
        tag = (case_id, layout)
        buf = _build(d, layout, BF, gpu)
        _launch(cdll.ug_flash_attn_fwd_wide, d, buf)
        torch.cuda.synchronize()
        first = buf["o"].clone()
        got, intact = _window(d, buf["o"])
        assert intact, ("the output sentinel outside the [Lq, H 512] window was overwritten", tag)
        assert bool(torch.isfinite(got).all()), ("a NaN of the padding (or of a masked key) reached the output", tag)
        total, worst, _ = BR.err(got, ref["O"])
        print(f"{case_id} [{layout}]: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
        assert total <= b_total and worst <= b_row, (tag, total, b_total, worst, b_row)
        if len(rows):
            r_total, r_row = WR.bounds(ref, rows)
            ct, cw, _ = BR.err(got[..., rows, :], ref["O"][..., rows, :])
            print(f"{case_id} [{layout}] chosen rows: rel-L2 {ct:.3e} ({r_total:.3e}), worst row {cw:.3e} ({r_row:.3e})")
            assert ct <= r_total and cw <= r_row, (tag, "chosen rows", ct, r_total, cw, r_row)
        _launch(cdll.ug_flash_attn_fwd_wide, d, buf)                  # again, into the same output
        torch.cuda.synchronize()
        assert torch.equal(buf["o"], first), ("two launches into the same output differ", tag)
    # the fp32 twin on the widened operands (one layout per case, all three over the case list)
    layout = LAYOUTS[WR.case_ids().index(case_id) % len(LAYOUTS)]
    buf = _build(d, layout, F32, gpu)
    _launch(cdll.ug_flash_attn_fwd_wide_f32, d, buf)
    torch.cuda.synchronize()
    got, intact = _window(d, buf["o"])
    assert intact and bool(torch.isfinite(got).all()), (case_id, layout, "fp32 twin: sentinel or NaN")
    total, worst, _ = BR.err(got, ref["O"])
    print(f"{case_id} fp32 twin [{layout}]: rel-L2 {total:.3e} (bound {F32_TOTAL:.0e}), worst row {worst:.3e} ({F32_ROW:.0e})")
    assert total <= F32_TOTAL and worst <= F32_ROW, (case_id, layout, total, worst)


def test_wide_forward_replays_from_a_graph(gpu):
    """one stream, one kernel node: the launch keeps no state and needs no workspace, so a replay gives the bits of a direct launch"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    case_id = "gaussian-1x2x257x520"
    d = WR.case_data(case_id)
    buf = _build(d, "packed_pad8", BF, gpu)
    _launch(cdll.ug_flash_attn_fwd_wide, d, buf)                      # direct (and the one-time dynamic-LDS attribute, outside the capture)
    torch.cuda.synchronize()
    direct = buf["o"].clone()
    buf["o"].fill_(SENT)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(cdll.ug_flash_attn_fwd_wide, d, buf)
    torch.cuda.synchronize()
    for _ in range(2):
        buf["o"].fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf["o"], direct), "a graph replay differs from the direct launch"
    b_total, b_row = WR.bounds(WR.case_reference(case_id))
    total, worst, _ = BR.err(_window(d, buf["o"])[0], WR.case_reference(case_id)["O"])
    assert total <= b_total and worst <= b_row, (total, worst)


def test_ops_flash_attn_routes_head_width_512(gpu):
    from unigen_amd import lib as ULIB
    from unigen_amd import ops
    case_id = "gaussian-2x1x100x333"
    d, ref = WR.case_data(case_id), WR.case_reference(case_id)
    b_total, b_row = WR.bounds(ref)
    for dtype in (BF, F32):
        buf = _build(d, "separate", dtype, gpu)
        (q, q_rs, q_bs), (k, k_rs, k_bs), (v, v_rs, v_bs), o = buf["q"], buf["k"], buf["v"], buf["o"]
        kw = dict(batches=d["B"], heads=d["H"], dh=WR.DH, Lq=d["Lq"], Lkv=d["Lkv"], q_strides=(q_rs, q_bs), k_strides=(k_rs, k_bs),
                  v_strides=(v_rs, v_bs), o_strides=(o.stride(1), o.stride(0)))
        ops.flash_attn(q, k, v, o, **kw)                                   # scale defaults to 512^-0.5, the case's
        torch.cuda.synchronize()
        got, intact = _window(d, o)
        total, worst, _ = BR.err(got, ref["O"])
        assert intact and total <= (b_total if dtype == BF else F32_TOTAL) and worst <= (b_row if dtype == BF else F32_ROW), (dtype, total, worst)
    lse = torch.zeros(d["B"], d["H"], 128, device=gpu, dtype=F32)
    with pytest.raises(ULIB.UniGenHipError, match="lse"):
        ops.flash_attn(q.to(BF), k.to(BF), v.to(BF), o.to(BF), lse=lse, **kw)
