"""ug_linear_attn_bwd and ug_glu_dwconv3x3_bwd with their fp32 twins (csrc/sana_bwd.hip) through the C ABI, against the float64 closed forms of
tests/sana_bwd_ref.py (checked on the host by tests/test_sana_bwd_ref_cpu.py over the same case ids).

Linear attention: the forward's cases, dout ~ N(0, 1) (seeded), `state` taken from a forward call on the same operands. Two layouts - q, k, v, dq, dk, dv
in buffers of their own; q | k | v packed into one buffer with 8 NaN pad columns and dq | dk | dv as the column blocks of one [M][3 D (+ 8)] buffer -
with spare NaN rows behind every sample. Outputs and workspace are pre-filled with a sentinel, which must survive outside the written windows and in the guard words behind the workspace.
GLU depthwise convolution: the forward's cases and (1, 17, 33, 8); NaN rows before and behind x and dout, NaN in dout's pad columns (they are not read),
sentinels behind dx's 2C columns, behind its last row, and behind dw9 / dbias.

Bounds (docs/PARITY_TOLERANCES.md, "Sana backward"): bf16 rel-L2 over each gradient tensor AND the worst row within 1.5 x err(G_v) against float64; the
fp32 twins within 1e-5 / 1e-4. One exception, which no fp32 evaluation can avoid: with ONE token the output is v whatever q and k are, so dq and dk
are exact zeros (1e-17 in float64) that the formulas reach as differences of terms of order one; there, and only there, BR.err's allowance for an fp32
difference that cancels applies (2^-20 of the cancelling terms' magnitude, absolutely). All outputs finite; the rows / heads
whose forward output is identically zero have exactly zero gradients; a second launch on a NaN-filled workspace and a graph replay are bit-identical;
NULL dw9 / dbias leaves dx bit-identical. dw9 is compared as the kernel leaves it, [9][2C] (a row = one tap)."""
import pytest
import torch

from tests import bwd_ref as BR
from tests import sana_bwd_ref as G
from tests import sana_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
F32_TOTAL, F32_ROW = 1e-5, 1e-4
SENT = 3.0
NAN = float("nan")
LAYOUTS = ("separate", "packed_pad8")
SPARE, SPARE_O = 3, 1                         # spare rows behind every sample (inputs: NaN; outputs: sentinel)
STATE = 32 * 32 + 32


def _flat(t):
    """[B, H, N, 32] -> [B, N, H 32]"""
    B, H, N, dh = t.shape
    return t.transpose(1, 2).reshape(B, N, H * dh)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _attn_build(d, layout, dtype, dev):
    """-> dict of (base tensor, row stride, batch stride) views for q, k, v, do, dq, dk, dv, and the output buffers under "outs" """
    B, N = d["B"], d["N"]
    D = d["H"] * R.DH
    v = {}
    own = lambda t: torch.cat([t.to(dtype), torch.full((B, SPARE, t.shape[-1]), NAN, dtype=dtype)], 1).to(dev)
    X = own(_flat(d["do"]))
    v["do"] = (X, X.stride(1), X.stride(0))
    if layout == "separate":
        for n in "qkv":
            X = own(_flat(d[n]))
            v[n] = (X, X.stride(1), X.stride(0))
        outs = [torch.full((B, N + SPARE_O, D + 8), SENT, dtype=dtype, device=dev) for _ in range(3)]
        for n, o in zip(("dq", "dk", "dv"), outs):
            v[n] = (o, o.stride(1), o.stride(0))
    else:
        X = torch.full((B, N + SPARE, 3 * D + 8), NAN, dtype=dtype)
        X[:, :N, :D], X[:, :N, D:2 * D], X[:, :N, 2 * D:3 * D] = (_flat(d[n]).to(dtype) for n in "qkv")
        X = X.to(dev)
        for i, n in enumerate("qkv"):
            v[n] = (X[0, 0, i * D:], X.stride(1), X.stride(0))
        o = torch.full((B, N + SPARE_O, 3 * D + 8), SENT, dtype=dtype, device=dev)
        outs = [o]
        for i, n in enumerate(("dq", "dk", "dv")):
            v[n] = (o[0, 0, i * D:], o.stride(1), o.stride(0))
    v["outs"] = outs
    return v


def _state(cdll, d, buf, dtype, dev):
    """the forward's state for these operands: the first B H 1056 floats of ug_linear_attn's workspace after a call"""
    from unigen_amd import lib as ULIB
    B, H, N = d["B"], d["H"], d["N"]
    ws = torch.full((int(cdll.ug_linear_attn_workspace_bytes(B, H, N)) // 4,), NAN, dtype=F32, device=dev)
    o = torch.empty(B, N, H * R.DH, dtype=dtype, device=dev)
    args = []
    for n in "qkv":
        t, rs, bs = buf[n]
        args += [t.data_ptr(), rs, bs]
    fn = cdll.ug_linear_attn if dtype == BF else cdll.ug_linear_attn_f32
    ULIB.check(fn(*args, o.data_ptr(), o.stride(1), o.stride(0), B, H, N, R.DH, ws.data_ptr(), _stream()), "linear_attn")
    return ws[:B * H * STATE].clone()


GUARD_WORDS = 8                               # behind the attention workspace: an overrun of the partials would show


def _attn_ws(cdll, d, dev, fill):
    return torch.full((int(cdll.ug_linear_attn_bwd_workspace_bytes(d["B"], d["H"], d["N"])) // 4 + GUARD_WORDS,), fill, dtype=F32, device=dev)


def _guard_intact(ws, fill):
    g = ws[-GUARD_WORDS:]
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _attn_launch(fn, d, buf, state, ws):
    from unigen_amd import lib as ULIB
    args = []
    for n in ("q", "k", "v", "do"):
        t, rs, bs = buf[n]
        args += [t.data_ptr(), rs, bs]
    args.append(state.data_ptr())
    for n in ("dq", "dk", "dv"):
        t, rs, bs = buf[n]
        args += [t.data_ptr(), rs, bs]
    ULIB.check(fn(*args, d["B"], d["H"], d["N"], R.DH, ws.data_ptr(), (ws.numel() - GUARD_WORDS) * 4, _stream()), "linear_attn_bwd")


def _attn_windows(d, layout, buf):
    """-> ({dq, dk, dv: [B, H, N, 32] on the host}, whether the sentinel is intact everywhere else)"""
    B, H, N = d["B"], d["H"], d["N"]
    D = H * R.DH
    got, intact = {}, True
    cpu = [o.detach().cpu() for o in buf["outs"]]
    for i, n in enumerate(("dq", "dk", "dv")):
        o, c0 = (cpu[i], 0) if layout == "separate" else (cpu[0], i * D)
        got[n] = o[:, :N, c0:c0 + D].reshape(B, N, H, R.DH).transpose(1, 2)
    for o in cpu:
        rest = o.clone()
        rest[:, :N, :D if layout == "separate" else 3 * D] = SENT
        intact = intact and bool((rest == SENT).all())
    return got, intact


def _attn_check(d, got, tag, f32):
    for n in ("dq", "dk", "dv"):
        mag = d["G"]["mag"][n] if (d["N"] == 1 and n != "dv") else None      # one token: dq and dk are exact zeros reached as differences
        b_total, b_row = (F32_TOTAL, F32_ROW) if f32 else G.bounds(d["G"][n], d["G_v"][n], mag)
        assert bool(torch.isfinite(got[n]).all()), ("a NaN of the padding reached", n, tag)
        total, worst, _ = BR.err(got[n], d["G"][n], mag)
        raw = BR.err(got[n], d["G"][n])
        print(f"{tag} {n}: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e}); without any cancellation allowance {raw[0]:.3e} / {raw[1]:.3e}")
        assert total <= b_total and worst <= b_row, (tag, n, total, b_total, worst, b_row)
    z = d["zero"]                                                    # [B, H, N]: the rows whose forward output is identically zero
    if d["id"].startswith("negative_query_row"):
        assert bool((got["dq"][z] == 0).all()), ("a query row without a positive entry has no gradient", tag)
    if d["id"].startswith("negative_key_head"):
        assert all(bool((got[n][z] == 0).all()) for n in ("dq", "dk", "dv")), ("a head without a positive key entry has no gradient", tag)


@pytest.mark.parametrize("case_id", G.attn_case_ids())
def test_linear_attn_bwd_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = G.attn_case(case_id)
    for layout in LAYOUTS:
        tag = (case_id, layout)
        buf = _attn_build(d, layout, BF, gpu)
        state, ws = _state(cdll, d, buf, BF, gpu), _attn_ws(cdll, d, gpu, SENT)
        _attn_launch(cdll.ug_linear_attn_bwd, d, buf, state, ws)
        torch.cuda.synchronize()
        first = [o.clone() for o in buf["outs"]]
        got, intact = _attn_windows(d, layout, buf)
        assert intact, ("the output sentinel outside the [N, H 32] windows was overwritten", tag)
        assert _guard_intact(ws, SENT), ("the words behind the workspace were written", tag)
        _attn_check(d, got, tag, False)
        ws.fill_(NAN)                                                 # the launch-state contract: nothing of an earlier call is read
        _attn_launch(cdll.ug_linear_attn_bwd, d, buf, state, ws)
        torch.cuda.synchronize()
        assert all(torch.equal(o, f) for o, f in zip(buf["outs"], first)), ("a second launch, on a NaN-polluted workspace, differs", tag)
        assert _guard_intact(ws, NAN), ("the words behind the workspace were written", tag)
    layout = LAYOUTS[G.attn_case_ids().index(case_id) % len(LAYOUTS)]    # the fp32 twin: one layout per case, both over the case list
    buf = _attn_build(d, layout, F32, gpu)
    state, ws = _state(cdll, d, buf, F32, gpu), _attn_ws(cdll, d, gpu, NAN)
    _attn_launch(cdll.ug_linear_attn_bwd_f32, d, buf, state, ws)
    torch.cuda.synchronize()
    got, intact = _attn_windows(d, layout, buf)
    assert intact and _guard_intact(ws, NAN), (case_id, layout, "fp32 twin: sentinel, or the words behind the workspace")
    _attn_check(d, got, (case_id, layout, "fp32"), True)


def test_linear_attn_bwd_replays_from_a_graph(gpu):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = G.attn_case("gaussian-1x4x257")
    buf = _attn_build(d, "packed_pad8", BF, gpu)
    state, ws = _state(cdll, d, buf, BF, gpu), _attn_ws(cdll, d, gpu, SENT)
    _attn_launch(cdll.ug_linear_attn_bwd, d, buf, state, ws)
    torch.cuda.synchronize()
    direct = buf["outs"][0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _attn_launch(cdll.ug_linear_attn_bwd, d, buf, state, ws)
    torch.cuda.synchronize()
    for _ in range(2):
        buf["outs"][0].fill_(SENT)
        ws.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf["outs"][0], direct), "a graph replay differs from the direct launch"


def test_ops_linear_attn_bwd(gpu):
    from unigen_amd import lib as ULIB
    from unigen_amd import ops
    d = G.attn_case("gaussian-2x3x64")
    for dtype in (BF, F32):
        buf = _attn_build(d, "packed_pad8", dtype, gpu)
        state = _state(ULIB.load(), d, buf, dtype, gpu)
        st = lambda n: (buf[n][1], buf[n][2])
        ops.linear_attn_bwd(buf["q"][0], buf["k"][0], buf["v"][0], buf["do"][0], state, buf["dq"][0], buf["dk"][0], buf["dv"][0], batches=d["B"], heads=d["H"],
                            N=d["N"], q_strides=st("q"), k_strides=st("k"), v_strides=st("v"), do_strides=st("do"), dq_strides=st("dq"), dk_strides=st("dk"),
                            dv_strides=st("dv"))
        torch.cuda.synchronize()
        got, intact = _attn_windows(d, "packed_pad8", buf)
        assert intact
        _attn_check(d, got, ("ops", dtype), dtype == F32)
    with pytest.raises(ValueError, match="workspace"):
        ops.linear_attn_bwd(buf["q"][0], buf["k"][0], buf["v"][0], buf["do"][0], state, buf["dq"][0], buf["dk"][0], buf["dv"][0], batches=d["B"], heads=d["H"],
                            N=d["N"], q_strides=st("q"), k_strides=st("k"), v_strides=st("v"), do_strides=st("do"), dq_strides=st("dq"), dk_strides=st("dk"),
                            dv_strides=st("dv"), workspace=torch.empty(64, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="state"):
        ops.linear_attn_bwd(buf["q"][0], buf["k"][0], buf["v"][0], buf["do"][0], state[:-1], buf["dq"][0], buf["dk"][0], buf["dv"][0], batches=d["B"],
                            heads=d["H"], N=d["N"], q_strides=st("q"), k_strides=st("k"), v_strides=st("v"), do_strides=st("do"), dq_strides=st("dq"),
                            dk_strides=st("dk"), dv_strides=st("dv"))


# ---------------------------------------------------------------- GLU depthwise convolution --------------------------------------------------------
GUARD = 2                                     # NaN pixel rows before and behind x and dout


def _glu_build(d, dtype, dev, with_w=True):
    B, H, W, C, pad = d["B"], d["H"], d["W"], d["C"], d["pad"]
    n = B * H * W
    X = torch.full((GUARD * W + n + GUARD * W, 2 * C), NAN, dtype=dtype)
    X[GUARD * W:GUARD * W + n] = d["x"].reshape(-1, 2 * C).to(dtype)
    DO = torch.full((GUARD * W + n + GUARD * W, C + pad), NAN, dtype=dtype)        # the pad columns stay NaN: they are not read
    DO[GUARD * W:GUARD * W + n, :C] = d["do"].reshape(-1, C).to(dtype)
    elem = 2 if dtype == BF else 4
    from unigen_amd import lib as ULIB
    wsb = int(ULIB.load().ug_glu_dwconv3x3_bwd_workspace_bytes(B, H, W, C, elem))
    buf = dict(X=X.to(dev), DO=DO.to(dev), dx=torch.full((n + 1, 2 * C + 8), SENT, dtype=dtype, device=dev),
               w9=d["w"].reshape(2 * C, 9).t().contiguous().to(dtype).to(dev), b=d["b"].to(dtype).to(dev),
               ws=torch.full((wsb // 4 + 4,), NAN, dtype=F32, device=dev), wsb=wsb)
    buf["dw9"] = torch.full((9 * 2 * C + 8,), SENT, dtype=F32, device=dev) if with_w else None
    buf["db"] = torch.full((2 * C + 8,), SENT, dtype=F32, device=dev) if with_w else None
    return buf


def _glu_launch(fn, d, buf):
    from unigen_amd import lib as ULIB
    off = GUARD * d["W"]
    ULIB.check(fn(buf["X"][off:].data_ptr(), buf["X"].stride(0), buf["w9"].data_ptr(), buf["b"].data_ptr(), buf["DO"][off:].data_ptr(), buf["DO"].stride(0),
                  buf["dx"].data_ptr(), buf["dx"].stride(0), None if buf["dw9"] is None else buf["dw9"].data_ptr(),
                  None if buf["db"] is None else buf["db"].data_ptr(), d["B"], d["H"], d["W"], d["C"], buf["ws"].data_ptr(), buf["wsb"], _stream()),
               "glu_dwconv3x3_bwd")


def _glu_windows(d, buf):
    B, H, W, C = d["B"], d["H"], d["W"], d["C"]
    n = B * H * W
    dx = buf["dx"].detach().cpu()
    intact = bool((dx[:n, 2 * C:] == SENT).all()) and bool((dx[n:] == SENT).all())
    got = dict(dx=dx[:n, :2 * C].reshape(B, H, W, 2 * C))
    if buf["dw9"] is not None:
        dw9, db = buf["dw9"].cpu(), buf["db"].cpu()
        intact = intact and bool((dw9[9 * 2 * C:] == SENT).all()) and bool((db[2 * C:] == SENT).all())
        got["dw"], got["db"] = dw9[:9 * 2 * C].reshape(9, 2 * C), db[:2 * C]
    return got, intact


def _glu_truth(d, which):
    t = dict(d[which])
    t["dw"] = t["dw"].reshape(-1, 9).t()                              # [2C, 1, 3, 3] -> the kernel's [9][2C]
    return t


def _glu_check(d, got, tag, f32):
    Gt, Gv = _glu_truth(d, "G"), _glu_truth(d, "G_v")
    for n in ("dx", "dw", "db"):
        b_total, b_row = (F32_TOTAL, F32_ROW) if f32 else G.bounds(Gt[n], Gv[n])
        assert bool(torch.isfinite(got[n]).all()), ("a NaN from outside the image or from dout's pad columns reached", n, tag)
        total, worst, _ = BR.err(got[n], Gt[n])
        print(f"{tag} {n}: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
        assert total <= b_total and worst <= b_row, (tag, n, total, b_total, worst, b_row)


@pytest.mark.parametrize("case_id", G.glu_case_ids())
def test_glu_dwconv_bwd_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = G.glu_case(case_id)
    buf = _glu_build(d, BF, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3_bwd, d, buf)
    torch.cuda.synchronize()
    first = {n: buf[n].clone() for n in ("dx", "dw9", "db")}
    got, intact = _glu_windows(d, buf)
    assert intact, ("a sentinel behind dx's columns, its last row, dw9 or dbias was overwritten", case_id)
    assert bool(torch.isnan(buf["ws"][buf["wsb"] // 4:]).all()), "the words behind the workspace were written"
    _glu_check(d, got, case_id, False)
    buf["ws"].fill_(NAN)
    _glu_launch(cdll.ug_glu_dwconv3x3_bwd, d, buf)
    torch.cuda.synchronize()
    assert all(torch.equal(buf[n], first[n]) for n in first), "a second launch, on a NaN-polluted workspace, differs"
    frozen = _glu_build(d, BF, gpu, with_w=False)                     # NULL dw9 / dbias: no reduction, the same dx
    _glu_launch(cdll.ug_glu_dwconv3x3_bwd, d, frozen)
    torch.cuda.synchronize()
    assert torch.equal(frozen["dx"], first["dx"]), "dx differs when dw9 / dbias are NULL"
    buf = _glu_build(d, F32, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3_bwd_f32, d, buf)
    torch.cuda.synchronize()
    got, intact = _glu_windows(d, buf)
    assert intact, (case_id, "fp32 twin: sentinel")
    _glu_check(d, got, (case_id, "fp32"), True)


def test_glu_dwconv_bwd_replays_from_a_graph(gpu):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = G.glu_case("glu-2x5x7x40-pad24")
    buf = _glu_build(d, BF, gpu)
    _glu_launch(cdll.ug_glu_dwconv3x3_bwd, d, buf)
    torch.cuda.synchronize()
    direct = {n: buf[n].clone() for n in ("dx", "dw9", "db")}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _glu_launch(cdll.ug_glu_dwconv3x3_bwd, d, buf)
    torch.cuda.synchronize()
    for _ in range(2):
        for n in direct:
            buf[n].fill_(SENT)
        buf["ws"].fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(buf[n], direct[n]) for n in direct), "a graph replay differs from the direct launch"


def test_ops_glu_dwconv_bwd(gpu):
    from unigen_amd import ops
    d = G.glu_case("glu-2x5x7x40-pad24")
    B, H, W, C, pad = d["B"], d["H"], d["W"], d["C"], d["pad"]
    n = B * H * W
    for dtype in (BF, F32):
        x, w9, b = d["x"].reshape(n, 2 * C).to(gpu, dtype), d["w"].reshape(2 * C, 9).t().contiguous().to(gpu, dtype), d["b"].to(gpu, dtype)
        do = torch.full((n, C + pad), NAN, dtype=dtype, device=gpu)
        do[:, :C] = d["do"].reshape(n, C).to(gpu, dtype)
        dx, dw9, db = ops.glu_dwconv3x3_bwd(x, w9, b, do, torch.empty(n, 2 * C, dtype=dtype, device=gpu), B=B, H=H, W=W, C=C,
                                            dw9=torch.empty(9, 2 * C, dtype=F32, device=gpu), dbias=torch.empty(2 * C, dtype=F32, device=gpu))
        torch.cuda.synchronize()
        _glu_check(d, dict(dx=dx.cpu().reshape(B, H, W, 2 * C), dw=dw9.cpu(), db=db.cpu()), ("ops", dtype), dtype == F32)
    with pytest.raises(ValueError, match="both"):
        ops.glu_dwconv3x3_bwd(x, w9, b, do, dx, B=B, H=H, W=W, C=C, dw9=dw9)
    with pytest.raises(ValueError, match="workspace"):
        ops.glu_dwconv3x3_bwd(x, w9, b, do, dx, B=B, H=H, W=W, C=C, workspace=torch.empty(64, dtype=torch.uint8, device=gpu))
