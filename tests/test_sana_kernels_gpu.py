"""ug_linear_attn and ug_glu_dwconv3x3 with their fp32 twins (csrc/sana.hip) through the C ABI, against the float64 references of tests/sana_ref.py
(checked on the host by tests/test_sana_ref_cpu.py over the same case ids).

Linear attention: every case runs in three layouts - q, k, v in buffers of their own (row stride H 32); packed into one buffer (row stride 3 H 32);
packed with 8 pad columns - with spare rows behind every sample. Every element of the operand buffers that is not an operand is NaN; the output buffer
and the workspace are pre-filled with a sentinel, which must survive outside the [N, H 32] window of the output.
GLU depthwise convolution: NaN rows before and behind the tensor (a read outside the image shows up), the output's pad columns must be exactly zero.
Bounds (docs/PARITY_TOLERANCES.md, "Sana kernels and block"): bf16 rel-L2 over the tensor AND the worst row within 1.5 x err(O_v); the fp32 twins
within 1e-5 / 1e-4; all outputs finite; a second launch, a launch on a NaN-polluted workspace and a graph replay bit-identical."""
import pytest
import torch

from tests import bwd_ref as BR
from tests import sana_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
F32_TOTAL, F32_ROW = 1e-5, 1e-4
SENT = 3.0
LAYOUTS = ("separate", "packed", "packed_pad8")
SPARE, SPARE_O = 3, 1                         # spare rows behind every sample


def _flat(t):
    """[B, H, N, 32] -> [B, N, H 32]"""
    B, H, N, dh = t.shape
    return t.transpose(1, 2).reshape(B, N, H * dh)


def _build(d, layout, dtype, dev):
    B, H, N = d["B"], d["H"], d["N"]
    D = H * R.DH
    nan = float("nan")
    q, k, v = (_flat(d[n]).to(dtype) for n in "qkv")
    if layout == "separate":
        bufs = []
        for t in (q, k, v):
            X = torch.full((B, N + SPARE, D), nan, dtype=dtype)
            X[:, :N] = t
            bufs.append(X.to(dev))
        views = dict(zip("qkv", ((X, X.stride(1), X.stride(0)) for X in bufs)))
    else:
        W = 3 * D + (8 if layout == "packed_pad8" else 0)
        X = torch.full((B, N + SPARE, W), nan, dtype=dtype)
        X[:, :N, :D], X[:, :N, D:2 * D], X[:, :N, 2 * D:3 * D] = q, k, v
        X = X.to(dev)
        views = dict(q=(X, X.stride(1), X.stride(0)), k=(X[0, 0, D:], X.stride(1), X.stride(0)), v=(X[0, 0, 2 * D:], X.stride(1), X.stride(0)))
    views["o"] = torch.full((B, N + SPARE_O, D + 8), SENT, dtype=dtype, device=dev)
    return views


def _workspace(cdll, d, dev, fill=SENT):
    return torch.full((int(cdll.ug_linear_attn_workspace_bytes(d["B"], d["H"], d["N"])) // 4,), fill, dtype=F32, device=dev)


def _launch(fn, d, buf, ws):
    from unigen_amd import lib as ULIB
    o = buf["o"]
    args = []
    for n in "qkv":
        t, rs, bs = buf[n]
        args += [t.data_ptr(), rs, bs]
    ULIB.check(fn(*args, o.data_ptr(), o.stride(1), o.stride(0), d["B"], d["H"], d["N"], R.DH, ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "linear_attn")


def _window(d, o):
    """the output window as [B, H, N, 32] on the host, and whether the sentinel is intact everywhere else"""
    B, H, N = d["B"], d["H"], d["N"]
    D = H * R.DH
    oc = o.detach().cpu()
    rest = oc.clone()
    rest[:, :N, :D] = SENT
    return oc[:, :N, :D].reshape(B, N, H, R.DH).transpose(1, 2), bool((rest == SENT).all())


@pytest.mark.parametrize("case_id", R.attn_case_ids())
def test_linear_attn_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.attn_case(case_id)
    b_total, b_row = R.bounds(d["O"], d["O_v"])
    for layout in LAYOUTS:
        tag = (case_id, layout)
        buf, ws = _build(d, layout, BF, gpu), _workspace(cdll, d, gpu)
        _launch(cdll.ug_linear_attn, d, buf, ws)
        torch.cuda.synchronize()
        first = buf["o"].clone()
        got, intact = _window(d, buf["o"])
        assert intact, ("the output sentinel outside the [N, H 32] window was overwritten", tag)
        assert bool(torch.isfinite(got).all()), ("a NaN of the padding reached the output", tag)
        total, worst, _ = BR.err(got, d["O"])
        print(f"{case_id} [{layout}]: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
        assert total <= b_total and worst <= b_row, (tag, total, b_total, worst, b_row)
        assert bool((got[d["zero"]] == 0).all()), ("a row without a positive query entry / a head without a positive key entry must be exactly 0", tag)
        ws.fill_(float("nan"))                                        # the launch-state contract: nothing of an earlier call is read
        _launch(cdll.ug_linear_attn, d, buf, ws)
        torch.cuda.synchronize()
        assert torch.equal(buf["o"], first), ("a second launch, on a NaN-polluted workspace, differs", tag)
    # the fp32 twin on the widened operands (one layout per case, all three over the case list)
    layout = LAYOUTS[R.attn_case_ids().index(case_id) % len(LAYOUTS)]
    buf, ws = _build(d, layout, F32, gpu), _workspace(cdll, d, gpu, float("nan"))
    _launch(cdll.ug_linear_attn_f32, d, buf, ws)
    torch.cuda.synchronize()
    got, intact = _window(d, buf["o"])
    assert intact and bool(torch.isfinite(got).all()), (case_id, layout, "fp32 twin: sentinel or NaN")
    total, worst, _ = BR.err(got, d["O"])
    print(f"{case_id} fp32 twin [{layout}]: rel-L2 {total:.3e} (bound {F32_TOTAL:.0e}), worst row {worst:.3e} ({F32_ROW:.0e})")
    assert total <= F32_TOTAL and worst <= F32_ROW, (case_id, layout, total, worst)
    assert bool((got[d["zero"]] == 0).all())


def test_linear_attn_replays_from_a_graph(gpu):
    """three kernel nodes on one stream, no state between launches: a replay gives the bits of a direct launch"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.attn_case("gaussian-1x4x257")
    buf, ws = _build(d, "packed_pad8", BF, gpu), _workspace(cdll, d, gpu)
    _launch(cdll.ug_linear_attn, d, buf, ws)
    torch.cuda.synchronize()
    direct = buf["o"].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(cdll.ug_linear_attn, d, buf, ws)
    torch.cuda.synchronize()
    for _ in range(2):
        buf["o"].fill_(SENT)
        ws.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf["o"], direct), "a graph replay differs from the direct launch"


def test_ops_linear_attn(gpu):
    from unigen_amd import ops
    d = R.attn_case("gaussian-2x3x64")
    b_total, b_row = R.bounds(d["O"], d["O_v"])
    for dtype in (BF, F32):
        buf = _build(d, "packed", dtype, gpu)
        (q, q_rs, q_bs), (k, k_rs, k_bs), (v, v_rs, v_bs), o = buf["q"], buf["k"], buf["v"], buf["o"]
        ops.linear_attn(q, k, v, o, batches=d["B"], heads=d["H"], N=d["N"], q_strides=(q_rs, q_bs), k_strides=(k_rs, k_bs), v_strides=(v_rs, v_bs),
                        o_strides=(o.stride(1), o.stride(0)))
        torch.cuda.synchronize()
        got, intact = _window(d, o)
        total, worst, _ = BR.err(got, d["O"])
        assert intact and total <= (b_total if dtype == BF else F32_TOTAL) and worst <= (b_row if dtype == BF else F32_ROW), (dtype, total, worst)
    with pytest.raises(ValueError, match="workspace"):
        ops.linear_attn(q, k, v, o, batches=d["B"], heads=d["H"], N=d["N"], q_strides=(q_rs, q_bs), k_strides=(k_rs, k_bs), v_strides=(v_rs, v_bs),
                        o_strides=(o.stride(1), o.stride(0)), workspace=torch.empty(64, dtype=torch.uint8, device=gpu))


# ---------------------------------------------------------------- GLU depthwise convolution --------------------------------------------------------
GUARD = 2                                     # NaN pixel rows before and behind the tensor


def _glu_build(d, dtype, dev):
    B, H, W, C, pad = d["B"], d["H"], d["W"], d["C"], d["pad"]
    X = torch.full((GUARD * W + B * H * W + GUARD * W, 2 * C), float("nan"), dtype=dtype)
    X[GUARD * W:GUARD * W + B * H * W] = d["x"].reshape(-1, 2 * C).to(dtype)
    out = torch.full((B * H * W + 1, C + pad + 8), SENT, dtype=dtype)      # a spare row and 8 spare columns keep the sentinel
    w9 = d["w"].reshape(2 * C, 9).t().contiguous().to(dtype)
    return dict(X=X.to(dev), x=None, out=out.to(dev), w9=w9.to(dev), b=d["b"].to(dtype).to(dev))


def _glu_launch(fn, d, buf):
    from unigen_amd import lib as ULIB
    x = buf["X"][GUARD * d["W"]:]
    ULIB.check(fn(x.data_ptr(), buf["X"].stride(0), buf["w9"].data_ptr(), buf["b"].data_ptr(), buf["out"].data_ptr(), d["C"] + d["pad"],
                  d["B"], d["H"], d["W"], d["C"], torch.cuda.current_stream().cuda_stream), "glu_dwconv3x3")


def _glu_window(d, out):
    """(the [B, H, W, C] result, the pad columns, whether the sentinel is intact elsewhere): `out` is addressed by the kernel with row stride C + pad"""
    B, H, W, C, pad = d["B"], d["H"], d["W"], d["C"], d["pad"]
    n, ld = B * H * W, C + pad
    flat = out.detach().cpu().reshape(-1)
    used = flat[:n * ld].reshape(n, ld)
    return used[:, :C].reshape(B, H, W, C), used[:, C:], bool((flat[n * ld:] == SENT).all())


@pytest.mark.parametrize("case_id", R.glu_case_ids())
def test_glu_dwconv_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.glu_case(case_id)
    b_total, b_row = R.bounds(d["O"], d["O_v"])
    buf = _glu_build(d, BF, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3, d, buf)
    torch.cuda.synchronize()
    first = buf["out"].clone()
    got, padcols, intact = _glu_window(d, buf["out"])
    assert intact, "the output sentinel behind the last row was overwritten"
    assert bool(torch.isfinite(got).all()), "a NaN from outside the image reached the output"
    assert bool((padcols == 0).all()) and not bool(torch.signbit(padcols).any()), "the pad columns [C, ldo) must be exactly zero"
    total, worst, _ = BR.err(got, d["O"])
    print(f"{case_id}: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
    assert total <= b_total and worst <= b_row, (case_id, total, b_total, worst, b_row)
    _glu_launch(cdll.ug_glu_dwconv3x3, d, buf)
    torch.cuda.synchronize()
    assert torch.equal(buf["out"], first), "two launches into the same output differ"
    buf = _glu_build(d, F32, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3_f32, d, buf)
    torch.cuda.synchronize()
    got, padcols, intact = _glu_window(d, buf["out"])
    assert intact and bool(torch.isfinite(got).all()) and bool((padcols == 0).all()), (case_id, "fp32 twin: sentinel, NaN or pad columns")
    total, worst, _ = BR.err(got, d["O"])
    print(f"{case_id} fp32 twin: rel-L2 {total:.3e} (bound {F32_TOTAL:.0e}), worst row {worst:.3e} ({F32_ROW:.0e})")
    assert total <= F32_TOTAL and worst <= F32_ROW, (case_id, total, worst)


def test_glu_dwconv_replays_from_a_graph(gpu):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.glu_case("glu-2x5x7x40-pad24")
    buf = _glu_build(d, BF, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3, d, buf)
    torch.cuda.synchronize()
    direct = buf["out"].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _glu_launch(cdll.ug_glu_dwconv3x3, d, buf)
    torch.cuda.synchronize()
    for _ in range(2):
        buf["out"].fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf["out"], direct), "a graph replay differs from the direct launch"
