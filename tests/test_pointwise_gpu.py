"""The entry points that launch pointwise_kernel (csrc/pointwise.h): ug_euler_step, ug_cfg_combine, ug_gelu_tanh(_bwd), ug_quick_gelu, ug_gelu_erf,
ug_relu and their fp32 twins, at the sizes where the one kernel's loop shapes turn: one chunk, exactly one block, one block and a chunk, and one chunk
past the 2048-block grid cap of the Euler / CFG launch (the grid-stride loop's second trip); for the GELU pair a length and a base that take the
element-wise path, for ReLU a base 8 bytes off (the guarded accesses), and out == x wherever an entry allows it. Each op is held to the float64
reference and the bound its own sweep applies (imported, not restated):
  euler_step, cfg_combine   bit equality             tests/test_fuzz_step_gpu.py (step_kernel_ref)
  gelu_tanh                 step_kernel_ref.gelu_bound
  gelu_tanh_bwd             tests/test_fuzz_backward_gpu.py
  quick_gelu, gelu_erf      text_ref.quick_gelu_bound, sd3_text_ref.gelu_erf_bound through text_ref.elementwise_excess
  relu                      one right answer, torch.relu: NaN and -0 pass
Outputs lie between guard elements that must come back untouched. The long case repeats a 4104-element pattern, so its reference costs nothing."""
import functools

import pytest
import torch

from tests import sd3_text_ref as S3
from tests import step_kernel_ref as SR
from tests import text_ref as TR
from tests.test_fuzz_backward_gpu import _check_elem, gelu_tanh_bwd_truth_and_tol

pytestmark = pytest.mark.gpu
BF, F32, F64 = SR.BF, SR.F32, SR.F64
G, SENT = SR.GUARD, SR.SENT
DTS = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
BLOCK = 8 * 256
SIZES = [8, BLOCK, BLOCK + 8, BLOCK * 2048 + 8]
PATTERN = 4104
OPS = ["euler_step", "cfg_combine", "gelu_tanh", "gelu_tanh_bwd", "quick_gelu", "gelu_erf", "relu"]
# (op, n, element offset of every base, in place) beside OPS x SIZES
EXTRA = [("gelu_tanh", 13, 1, False), ("gelu_tanh_bwd", 13, 1, False), ("gelu_tanh", 4099, 0, False), ("gelu_tanh_bwd", 4099, 0, False)] + \
        [(op, BLOCK + 8, 0, True) for op in OPS if op != "euler_step"]          # euler_step is in place by definition
CASES = [(op, n, 0, False) for op in OPS for n in SIZES] + EXTRA


@functools.lru_cache(maxsize=None)
def _pattern(op, dt):
    """two operands of PATTERN elements as stored in dt: magnitudes over 1e-3 .. 1e3, for the activations half of them over +-30, and the edge values"""
    if op == "gelu_tanh_bwd":                                          # the domain of tests/test_fuzz_backward_gpu.py: x over [-10, 10] with exact zeros
        g = torch.Generator().manual_seed(PATTERN)
        a, b = (torch.rand(PATTERN, generator=g) * 20 - 10).to(dt), torch.randn(PATTERN, generator=g).to(dt)
        a[::5], a[1], a[-1] = 0.0, 10.0, -10.0
        return a, b
    a, b = SR.flat_data(dict(n=PATTERN, seed=len(op)), dt, big=op not in ("euler_step", "cfg_combine"))
    a[:6] = torch.tensor([0.0, -0.0, 1.0, -1.0, 30.0, -30.0]).to(dt)
    if op == "relu":
        a[6], a[7] = float("nan"), float("-inf")
    return a, b


def _rep(t, n):
    return t.repeat(-(-n // PATTERN))[:n].clone()


@functools.lru_cache(maxsize=None)
def _want(op, dt):
    """for the pattern -> ("exact", tensor in dt) or ("bound", fp64 truth, fp64 bound); every op is pointwise, so a repeated pattern repeats these"""
    a, b = _pattern(op, dt)
    if op == "euler_step":
        return "exact", SR.euler_step(a, b, DT_STEP)
    if op == "cfg_combine":
        return "exact", SR.cfg_combine(a, b, GS)
    if op == "relu":
        return "exact", torch.relu(a)
    if op == "gelu_tanh":
        truth = SR.gelu64(a)
        return "bound", truth, SR.gelu_bound(a, truth, dt)
    if op == "gelu_tanh_bwd":
        return ("bound",) + gelu_tanh_bwd_truth_and_tol(a, b, dt)
    return ("bound",) + (TR.quick_gelu_bound if op == "quick_gelu" else S3.gelu_erf_bound)(a.to(F64), dt == BF)


DT_STEP, GS = 0.9741077 - 0.9873806, 3.5          # a step of SD3's shifted schedule (rounds in bf16); a guidance scale


def _guarded(n, off, dt, dev, values=None):
    """-> (device buffer of sentinels with `values` at [G + off, G + off + n), the address of that slice)"""
    buf = torch.full((G + off + n + G,), SENT, dtype=dt)
    if values is not None:
        buf[G + off:G + off + n] = values
    d = buf.to(dev)
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + (G + off) * d.element_size()


def _inside(buf, n, off):
    return buf[G + off:G + off + n]


def _guards_intact(buf, n, off):
    return bool((buf[:G + off] == SENT).all() and (buf[G + off + n:] == SENT).all())


def _same_bits(x, y):
    bits = torch.int16 if x.dtype == BF else torch.int32
    return torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op,n,off,inplace", CASES, ids=[f"{o}-n{n}" + (f"-off{f}" if f else "") + ("-inplace" if i else "") for o, n, f, i in CASES])
def test_pointwise_entry(gpu, op, n, off, inplace, dt):
    from unigen_amd import lib
    cdll = lib.load()
    fn = getattr(cdll, "ug_" + op + ("" if dt == BF else "_f32"))
    stream = torch.cuda.current_stream().cuda_stream
    if op == "relu" and off == 0 and not inplace and n == BLOCK + 8:
        off = 8 // (2 if dt == BF else 4)                              # this size doubles as the base 8 bytes off 16: the guarded accesses
    a, b = (_rep(t, n) for t in _pattern(op, dt))
    ab, ap = _guarded(n, off, dt, gpu, a)
    bb, bp = _guarded(n, off, dt, gpu, b)
    ob, op_ = (ab, ap) if inplace or op == "euler_step" else _guarded(n, off, dt, gpu)
    if inplace and op == "gelu_tanh_bwd":
        ob, op_ = bb, bp                                               # dx over dy
    if op == "euler_step":
        rc = fn(ap, bp, DT_STEP, n, stream)
    elif op == "cfg_combine":
        rc = fn(ap, bp, GS, op_, n, stream)
    elif op == "gelu_tanh_bwd":
        rc = fn(ap, bp, op_, n, stream)
    else:
        rc = fn(ap, op_, n, stream)
    assert rc == lib.UG_OK, (rc, cdll.ug_last_error())
    torch.cuda.synchronize()
    out = ob.cpu()
    assert _guards_intact(out, n, off), f"{op}: written outside the output"
    for name, buf, src in (("first", ab, a), ("second", bb, b)):       # operands that are not the output come back as they went in
        if buf is not ob:
            host = buf.cpu()
            assert _guards_intact(host, n, off) and _same_bits(_inside(host, n, off), src), f"{op}: the {name} operand was written"
    got = _inside(out, n, off)
    want = _want(op, dt)
    want = (want[0],) + tuple(_rep(t, n) for t in want[1:])
    if want[0] == "exact":
        nan, zero = torch.isnan(want[1]), torch.zeros_like(got)       # a NaN stays a NaN; every other element has the reference's bits (-0 included)
        assert torch.equal(torch.isnan(got), nan) and _same_bits(torch.where(nan, zero, got), torch.where(nan, zero, want[1])), \
            (op, n, "differing elements", ((got != want[1]) & ~nan).nonzero()[:4].flatten().tolist())
    elif op == "gelu_tanh_bwd":
        _check_elem(op, got, want[1], want[2], dict(n=n, off=off, dt=str(dt)))
    elif op == "gelu_tanh":
        mask = torch.zeros(out.shape, dtype=torch.bool)
        mask[G + off:G + off + n] = True
        SR.judge_bounded(f"{op} n{n}", out, want[1], want[2], mask)
    else:
        excess = TR.elementwise_excess(got, want[1], want[2], dt == BF)
        assert excess <= 1.0, (op, n, excess)
