"""ug_rmsnorm_bias_rows, ug_msconv_proj, ug_dc_shortcut_down / _up and ug_silu with their fp32 twins (csrc/dcae.hip) through the C ABI, against the
float64 references of tests/dcae_ref.py (checked on the host by tests/test_dcae_ref_cpu.py over the same case ids).

Every case: NaN rows before and behind each operand, NaN pad columns in every packed row (row stride > channels), outputs pre-filled with a sentinel
that must survive everywhere outside the written window, a second launch and a graph replay bit-identical to the first.
Bounds (docs/PARITY_TOLERANCES.md, "DC-AE"): bf16 rel-L2 over the tensor AND the worst row within 1.5 x err(O_v) against O, no floor; the fp32 twins
within 1e-5 / 1e-4; the pure copies (up without x, down with g = 1 without x) bit for bit.

The cases behind the first ones of each kernel are the sweep of docs/PARITY_TOLERANCES.md, "DC-AE": the second and later row and column tiles of
msconv_proj_kernel (k = 5 and 3), once in the model's layout - x and out column windows of one buffer; every lane group and chunk pass of
rmsnorm_bias_rows_kernel, and rows whose mean square lies below and near eps; the published channel pairs of the shortcuts over several workgroups.
The worst figures per kernel and path are printed at the end of the module (pytest -s)."""
import pytest
import torch

from tests import bwd_ref as BR
from tests import dcae_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
F32_TOTAL, F32_ROW = 1e-5, 1e-4
SENT = 3.0
GUARD = 3                                     # NaN rows before and behind an operand
PAD = 8                                       # NaN pad columns of a packed row
RECORD = {}                                   # (kernel, path) -> [cases, worst rel-L2, worst row, worst rel-L2 / bound, worst row / bound]


def teardown_module(module):
    for (k, path), (n, t, w, rt, rw) in sorted(RECORD.items()):
        print(f"[dcae-sweep] {k} {path}: {n} cases, rel-L2 {t:.2e}, worst row {w:.2e}, of the bound {rt:.2f} / {rw:.2f}")


def _kernel_of(tag):
    cid = tag[0] if isinstance(tag, tuple) else tag
    head = str(cid).split("-")[0]
    return {"ms5": "ug_msconv_proj k = 5", "ms3": "ug_msconv_proj k = 3", "norm": "ug_rmsnorm_bias_rows", "down": "ug_dc_shortcut_down",
            "up": "ug_dc_shortcut_up", "silu": "ug_silu"}.get(head, head)


def _operand(t2d, dtype, dev, pad=PAD):
    """[rows, C] -> (the guarded buffer, the view of the operand's rows: [rows, C + pad] with NaN everywhere but [:, :C])"""
    rows, C = t2d.shape
    pad += -(C + pad) % 8                      # row strides are multiples of 8 elements
    full = torch.full((GUARD + rows + GUARD, C + pad), float("nan"), dtype=dtype)
    full[GUARD:GUARD + rows, :C] = t2d.to(dtype)
    full = full.to(dev)
    return full, full[GUARD:GUARD + rows]


def _output(rows, C, dtype, dev, pad=PAD):
    return torch.full((rows + 1, C + pad), SENT, dtype=dtype, device=dev)


def _window(out, rows, C):
    """(the written window on the host, whether the sentinel is intact everywhere else)"""
    oc = out.detach().cpu()
    rest = oc.clone()
    rest[:rows, :C] = SENT
    return oc[:rows, :C], bool((rest == SENT).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _twice_and_replayed(launch, out, refill=None):
    """the launch again, then captured and replayed twice on a sentinel-filled output: the bits of the first launch each time"""
    first = out.clone()
    if refill is not None:
        refill()
    launch()
    torch.cuda.synchronize()
    assert torch.equal(out, first), "a second launch differs"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    for _ in range(2):
        out.fill_(SENT)
        if refill is not None:
            refill()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first), "a graph replay differs from the direct launch"


def _judge(tag, got, d, dtype, intact, record=RECORD):
    assert intact, ("the output sentinel outside the window was overwritten", tag)
    assert bool(torch.isfinite(got).all()), ("a NaN of the padding reached the output", tag)
    total, worst, _ = BR.err(got.reshape(d["O"].shape), d["O"])
    if dtype == BF:
        b_total, b_row = R.bounds(d["O"], d["O_v"])
    else:
        b_total, b_row = F32_TOTAL, F32_ROW
    print(f"{tag}: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
    rec = record.setdefault((_kernel_of(tag), "bf16" if dtype == BF else "fp32"), [0, 0.0, 0.0, 0.0, 0.0])
    rec[0] += 1
    for i, v in enumerate((total, worst, total / b_total if b_total else 0.0, worst / b_row if b_row else 0.0)):
        rec[1 + i] = max(rec[1 + i], v)
    assert total <= b_total and worst <= b_row, (tag, total, b_total, worst, b_row)


# ---------------------------------------------------------------- RMSNorm with weight and bias ------------------------------------------------------
@pytest.mark.parametrize("case_id", R.norm_old_case_ids() + R.norm_lane_case_ids() + R.norm_small_case_ids())
def test_rmsnorm_bias_rows_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.norm_case(case_id)
    rows, C, alias = d["rows"], d["C"], d["mode"] == "alias"
    for dtype, fn in ((BF, cdll.ug_rmsnorm_bias_rows), (F32, cdll.ug_rmsnorm_bias_rows_f32)):
        _, x = _operand(d["x"], dtype, gpu, PAD + d["pad"])
        w, b = d["w"].to(dtype).to(gpu), d["b"].to(dtype).to(gpu)
        out = _output(rows, C, dtype, gpu)
        r = None
        if d["r"] is not None and not alias:
            _, r = _operand(d["r"], dtype, gpu, 2 * PAD)

        def refill():
            if alias:                         # the residual sits in the output buffer and is overwritten by the sum
                out[:rows, :C] = d["r"].to(dtype).to(gpu)
        refill()
        rp, ldr = (out.data_ptr(), out.stride(0)) if alias else (r.data_ptr(), r.stride(0)) if r is not None else (None, 0)

        def launch():
            ULIB.check(fn(x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), rp, ldr, out.data_ptr(), out.stride(0), rows, C, R.EPS_NORM, d["act"],
                          _stream()), "rmsnorm_bias_rows")
        launch()
        torch.cuda.synchronize()
        got, intact = _window(out, rows, C)
        _judge((case_id, dtype), got, d, dtype, intact)
        if d["zero_row"] is not None:
            assert torch.equal(got[d["zero_row"]].double(), d["b"].double()), "a row of zeros: the output is the bias"
        if d["act"]:
            assert bool((got >= 0).all())
        _twice_and_replayed(launch, out, refill if alias else None)


# ---------------------------------------------------------------- multiscale projection ------------------------------------------------------------
def _ms_weights(d, dtype, dev):
    k, C = d["k"], d["G"] * R.DH
    return d["w_dw"].reshape(C, k * k).t().contiguous().to(dtype).to(dev), d["w_pw"].reshape(d["G"], R.DH, R.DH).contiguous().to(dtype).to(dev)


@pytest.mark.parametrize("case_id", R.ms_case_ids(5)[:R.MS_OLD] + R.ms_case_ids(3)[1:3] + R.MS_SEAM_IDS)
def test_msconv_proj_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.ms_case(case_id)
    B, H, W, G, k = d["B"], d["H"], d["W"], d["G"], d["k"]
    rows, C = B * H * W, G * R.DH
    for dtype, fn in ((BF, cdll.ug_msconv_proj), (F32, cdll.ug_msconv_proj_f32)):
        _, x = _operand(d["x"].reshape(rows, C), dtype, gpu)
        w_dw, w_pw = _ms_weights(d, dtype, gpu)
        out = _output(rows, C, dtype, gpu)

        def launch():
            ULIB.check(fn(x.data_ptr(), x.stride(0), w_dw.data_ptr(), w_pw.data_ptr(), out.data_ptr(), out.stride(0), B, H, W, G, k, _stream()), "msconv_proj")
        launch()
        torch.cuda.synchronize()
        got, intact = _window(out, rows, C)
        _judge((case_id, dtype), got, d, dtype, intact)
        _twice_and_replayed(launch, out)


def test_msconv_proj_in_the_models_layout(gpu):
    """x and out are column windows of ONE buffer with ldx == ldo == 6 G 32, out 3 G 32 columns behind x, as AutoencoderDC's attention block calls
    it: the input columns keep their bits, the columns between and behind the windows keep the sentinel, the guard rows stay NaN"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.ms_case(R.MS_MODEL_LAYOUT_ID)
    B, H, W, G, k = d["B"], d["H"], d["W"], d["G"], d["k"]
    rows, C = B * H * W, G * R.DH
    ld, off = 6 * C, 3 * C
    host = torch.full((GUARD + rows + GUARD, ld), float("nan"), dtype=BF)
    host[GUARD:GUARD + rows] = SENT
    host[GUARD:GUARD + rows, :C] = d["x"].reshape(rows, C)
    buf = host.to(gpu)
    x, out = buf[GUARD:GUARD + rows], buf[GUARD:GUARD + rows, off:]
    w_dw, w_pw = _ms_weights(d, BF, gpu)
    assert x.stride(0) == out.stride(0) == ld and out.data_ptr() == x.data_ptr() + 2 * off

    def launch():
        ULIB.check(cdll.ug_msconv_proj(x.data_ptr(), ld, w_dw.data_ptr(), w_pw.data_ptr(), out.data_ptr(), ld, B, H, W, G, k, _stream()), "msconv_proj")
    launch()
    torch.cuda.synchronize()
    after = buf.cpu()
    assert bool(after[:GUARD].isnan().all()) and bool(after[GUARD + rows:].isnan().all()), "a guard row was written"
    live = after[GUARD:GUARD + rows]
    assert torch.equal(live[:, :C].view(torch.int16), host[GUARD:GUARD + rows, :C].view(torch.int16)), "the input columns changed"
    intact = bool((live[:, C:off] == SENT).all()) and bool((live[:, off + C:] == SENT).all())
    _judge((R.MS_MODEL_LAYOUT_ID, "model layout"), live[:, off:off + C], d, BF, intact)
    window = out[:, :C]
    _twice_and_replayed(launch, window)
    again = buf.cpu()[GUARD:GUARD + rows]
    assert torch.equal(again[:, :C].view(torch.int16), host[GUARD:GUARD + rows, :C].view(torch.int16))
    assert bool((again[:, C:off] == SENT).all()) and bool((again[:, off + C:] == SENT).all())


# ---------------------------------------------------------------- shortcuts -------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", R.sc_case_ids(False)[:12] + R.sc_case_ids(True)[:12] + R.sc_published_case_ids(False) + R.sc_published_case_ids(True))
def test_dc_shortcut_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.sc_case(case_id)
    B, H, W, Cin, Cout, f = d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["f"]
    rows_o = B * H * W * f * f if d["up"] else B * (H // f) * (W // f)
    base = "ug_dc_shortcut_up" if d["up"] else "ug_dc_shortcut_down"
    for dtype, fn in ((BF, getattr(cdll, base)), (F32, getattr(cdll, base + "_f32"))):
        _, h = _operand(d["h"].reshape(-1, Cin), dtype, gpu)
        x = None
        if d["x"] is not None:
            _, x = _operand(d["x"].reshape(-1, d["x"].shape[-1]), dtype, gpu, 2 * PAD)
        out = _output(rows_o, Cout, dtype, gpu)

        def launch():
            ULIB.check(fn(h.data_ptr(), h.stride(0), x.data_ptr() if x is not None else None, x.stride(0) if x is not None else 0,
                          1 if d["mode"] == "xshuffle" else 0, out.data_ptr(), out.stride(0), B, H, W, Cin, Cout, f, _stream()), base)
        launch()
        torch.cuda.synchronize()
        got, intact = _window(out, rows_o, Cout)
        _judge((case_id, dtype), got, d, dtype, intact)
        if d["exact"]:
            assert torch.equal(got.double().reshape(d["O"].shape), d["O"]), ("a pure copy must be bit for bit", case_id, dtype)
        _twice_and_replayed(launch, out)


def test_dc_shortcut_x_may_be_the_output(gpu):
    """x with the output's layout may alias out: a thread reads its 8 elements of x before it stores them"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    for cid, base in (("down-2x4x6x16to16xf2-x", "ug_dc_shortcut_down"), ("up-2x3x5x32to8xf2-x", "ug_dc_shortcut_up")):
        d = R.sc_case(cid)
        B, H, W, Cin, Cout, f = d["B"], d["H"], d["W"], d["Cin"], d["Cout"], d["f"]
        rows_o = d["O"].numel() // Cout
        _, h = _operand(d["h"].reshape(-1, Cin), BF, gpu)
        out = _output(rows_o, Cout, BF, gpu)
        out[:rows_o, :Cout] = d["x"].reshape(rows_o, Cout).to(gpu)
        ULIB.check(getattr(cdll, base)(h.data_ptr(), h.stride(0), out.data_ptr(), out.stride(0), 0, out.data_ptr(), out.stride(0), B, H, W, Cin, Cout, f, _stream()), base)
        torch.cuda.synchronize()
        got, intact = _window(out, rows_o, Cout)
        _judge((cid, "aliased"), got, d, BF, intact)


# ---------------------------------------------------------------- SiLU ------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", R.silu_case_ids())
def test_silu_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    d = R.silu_case(case_id)
    n = d["n"]
    rows = dict(d, O=d["O"].reshape(-1, 8), O_v=d["O_v"].reshape(-1, 8))          # judged as rows of 8
    for dtype, fn in ((BF, cdll.ug_silu), (F32, cdll.ug_silu_f32)):
        full = torch.full((8 + n + 8,), float("nan"), dtype=dtype)
        full[8:8 + n] = d["x"].to(dtype)
        full = full.to(gpu)
        out = torch.full((n + 8,), SENT, dtype=dtype, device=gpu)

        def launch():
            ULIB.check(fn(full[8:].data_ptr(), out.data_ptr(), n, _stream()), "silu")
        launch()
        torch.cuda.synchronize()
        oc = out.detach().cpu()
        _judge((case_id, dtype), oc[:n].reshape(-1, 8), rows, dtype, bool((oc[n:] == SENT).all()))
        assert float(oc[1]) == 88.0 and float(oc[6]) == 0.0 and -1e-30 < float(oc[3]) <= 0.0
        _twice_and_replayed(launch, out)
        if dtype == BF:                                                           # in place: the same bits
            y = d["x"].to(gpu).clone()
            ULIB.check(fn(y.data_ptr(), y.data_ptr(), n, _stream()), "silu")
            torch.cuda.synchronize()
            assert torch.equal(y.cpu(), oc[:n])


def test_ops_wrappers(gpu):
    """unigen_amd.ops over the same cases: the wrappers pass the strides of the views they are given"""
    from unigen_amd import ops
    d = R.norm_case("norm-33x128-residual")
    _, x = _operand(d["x"], BF, gpu)
    _, r = _operand(d["r"], BF, gpu)
    out = _output(d["rows"], d["C"], BF, gpu)
    ops.rmsnorm_bias_rows(x, d["w"].to(gpu), d["b"].to(gpu), R.EPS_NORM, residual=r, out=out[:d["rows"]], C_=d["C"])
    torch.cuda.synchronize()
    _judge("ops.rmsnorm_bias_rows", _window(out, d["rows"], d["C"])[0], d, BF, _window(out, d["rows"], d["C"])[1])
    d = R.ms_case("ms5-2x5x7x6")
    rows, C = d["B"] * d["H"] * d["W"], d["G"] * R.DH
    _, x = _operand(d["x"].reshape(rows, C), BF, gpu)
    w_dw, w_pw = _ms_weights(d, BF, gpu)
    out = _output(rows, C, BF, gpu)
    ops.msconv_proj(x, w_dw, w_pw, out[:rows], B=d["B"], H=d["H"], W=d["W"], G=d["G"], k=5)
    torch.cuda.synchronize()
    _judge("ops.msconv_proj", _window(out, rows, C)[0], d, BF, _window(out, rows, C)[1])
    for cid in ("down-2x4x6x16to16xf2-xshuffle", "up-2x3x5x32to8xf2-xshuffle"):
        d = R.sc_case(cid)
        rows_o = d["O"].numel() // d["Cout"]
        _, h = _operand(d["h"].reshape(-1, d["Cin"]), BF, gpu)
        _, x = _operand(d["x"].reshape(-1, d["x"].shape[-1]), BF, gpu)
        out = _output(rows_o, d["Cout"], BF, gpu)
        ops.dc_shortcut(h, out[:rows_o], up=d["up"], B=d["B"], H=d["H"], W=d["W"], Cin=d["Cin"], Cout=d["Cout"], factor=d["f"], x=x, x_shuffle=True)
        torch.cuda.synchronize()
        _judge("ops.dc_shortcut " + cid, _window(out, rows_o, d["Cout"])[0], d, BF, _window(out, rows_o, d["Cout"])[1])
    d = R.silu_case("silu-1000")
    y = ops.silu(d["x"].to(gpu))
    torch.cuda.synchronize()
    assert BR.err(y.cpu().reshape(-1, 8), d["O"].reshape(-1, 8))[0] <= R.bounds(d["O"], d["O_v"])[0]
