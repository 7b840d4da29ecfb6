"""Seeded random geometries of the DC-AE kernels (csrc/dcae.hip: ug_msconv_proj, ug_rmsnorm_bias_rows, ug_dc_shortcut_down / _up and their fp32 twins)
through the C ABI, with the arenas and the bounds of tests/test_dcae_kernels_gpu.py (docs/PARITY_TOLERANCES.md, "DC-AE"): NaN guard rows and NaN
pad columns around every operand, a sentinel-filled output that must survive outside the window, finite output, a second launch and two graph replays
with the first launch's bits; bf16 rel-L2 over the tensor AND the worst row within 1.5 x err(O_v) against O, the fp32 twins within 1e-5 / 1e-4, the
pure copies bit for bit. The float64 reference and its rounding variant (tests/dcae_ref.py) are computed per draw.

    msconv      k in {3, 5}, B in 1..2, H in 1..40, W in 1..80, G in 1..9; row strides of G 32 plus 0, 8 or 24 pad columns, x and out drawn apart
    norm        rows in 1..300, C = 8 n with n in 1..576 - every other seed takes n from the edges of the lane groups and of the chunk passes -
                a random mode, pads of x, residual and out drawn apart
    shortcuts   direction, f in {1, 2}, Cin and Cout multiples of 8 up to 1024, B in 1..2, H, W in 1..12 (even for down at f = 2), a random mode
A draw that the entry point must refuse (the divisibility rule of dc_shortcut_impl: Cout | Cin f^2 down, Cin | Cout f^2 up) is redrawn on the host;
nothing is sent to the device to see what happens. The geometry of a draw is in every assertion message: a failure is reproducible from its seed."""
import math
import random

import pytest
import torch

from tests import dcae_ref as R
from tests import test_dcae_kernels_gpu as KT

pytestmark = pytest.mark.gpu

BF, F32 = KT.BF, KT.F32
SEEDS = 12
NORM_EDGES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 576)         # C / 8 at the edges of lpr and of the chunk passes
RECORD = {}


def teardown_module(module):
    for (k, path), (n, t, w, rt, rw) in sorted(RECORD.items()):
        print(f"[dcae-fuzz] {k} {path}: {n} draws, rel-L2 {t:.2e}, worst row {w:.2e}, of the bound {rt:.2f} / {rw:.2f}")


# ---------------------------------------------------------------- the draws: host arithmetic only, checked without a GPU by tests/test_dcae_ref_cpu.py ----
def draw_ms(seed):
    rng = random.Random(9100 + seed)
    return dict(k=rng.choice((3, 5)), B=rng.randint(1, 2), H=rng.randint(1, 40), W=rng.randint(1, 80), G=rng.randint(1, 9),
                pad_x=rng.choice((0, 8, 24)), pad_o=rng.choice((0, 8, 24)))


def draw_norm(seed):
    rng = random.Random(9200 + seed)
    n = rng.choice(NORM_EDGES) if seed % 2 == 0 else rng.randint(1, 576)
    return dict(rows=rng.randint(1, 300), C=8 * n, mode=rng.choice(R.NORM_MODES), pad_x=rng.choice((0, 8, 24, 40)), pad_r=rng.choice((0, 8, 24, 40)),
                pad_o=rng.choice((0, 8, 24, 40)))


def sc_accepted(up, Cin, Cout, f):
    """the documented rule of ug_dc_shortcut_down / _up for channel counts that are multiples of 8"""
    return (Cout * f * f) % Cin == 0 if up else (Cin * f * f) % Cout == 0


def draw_sc(seed):
    rng = random.Random(9300 + seed)
    up, f = rng.random() < 0.5, rng.choice((1, 2))
    for _ in range(100000):
        Cin, Cout = 8 * rng.randint(1, 128), 8 * rng.randint(1, 128)
        if sc_accepted(up, Cin, Cout, f):
            break
    else:
        raise AssertionError("no accepted channel pair drawn")
    even = not up and f == 2
    H, W = (2 * rng.randint(1, 6), 2 * rng.randint(1, 6)) if even else (rng.randint(1, 12), rng.randint(1, 12))
    return dict(up=up, f=f, Cin=Cin, Cout=Cout, B=rng.randint(1, 2), H=H, W=W, mode=rng.choice(R.SC_MODES))


def _geo(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


# ---------------------------------------------------------------- multiscale projection ------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
def test_msconv_proj_random_geometries(gpu, seed):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    c = draw_ms(seed)
    B, H, W, G, k = c["B"], c["H"], c["W"], c["G"], c["k"]
    rows, C = B * H * W, G * R.DH
    g = torch.Generator().manual_seed(9100 + seed)
    d = dict(G=G, k=k, x=(1.5 * torch.randn(B, H, W, C, generator=g)).to(BF), w_dw=(torch.randn(C, 1, k, k, generator=g) / k).to(BF),
             w_pw=(torch.randn(C, R.DH, 1, 1, generator=g) / math.sqrt(R.DH)).to(BF))
    d["O"], d["O_v"] = R.msconv(d["x"], d["w_dw"], d["w_pw"]), R.msconv_variant(d["x"], d["w_dw"], d["w_pw"])
    tag = f"ms{k}-fuzz seed {seed}: {_geo(c)}"
    for dtype, fn in ((BF, cdll.ug_msconv_proj), (F32, cdll.ug_msconv_proj_f32)):
        _, x = KT._operand(d["x"].reshape(rows, C), dtype, gpu, c["pad_x"])
        w_dw, w_pw = KT._ms_weights(d, dtype, gpu)
        out = KT._output(rows, C, dtype, gpu, c["pad_o"])
        assert x.stride(0) == C + c["pad_x"] and out.stride(0) == C + c["pad_o"]

        def launch():
            ULIB.check(fn(x.data_ptr(), x.stride(0), w_dw.data_ptr(), w_pw.data_ptr(), out.data_ptr(), out.stride(0), B, H, W, G, k, KT._stream()), tag)
        launch()
        torch.cuda.synchronize()
        got, intact = KT._window(out, rows, C)
        KT._judge((tag, dtype), got, d, dtype, intact, RECORD)
        KT._twice_and_replayed(launch, out)


# ---------------------------------------------------------------- RMSNorm with weight and bias ------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
def test_rmsnorm_bias_rows_random_geometries(gpu, seed):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    c = draw_norm(seed)
    rows, C, mode = c["rows"], c["C"], c["mode"]
    alias, act = mode == "alias", 1 if mode == "relu" else 0
    g = torch.Generator().manual_seed(9200 + seed)
    xh = (2.0 * torch.randn(rows, C, generator=g)).to(BF)
    wh, bh = (1 + 0.25 * torch.randn(C, generator=g)).to(BF), (0.3 * torch.randn(C, generator=g)).to(BF)
    rh = torch.randn(rows, C, generator=g).to(BF) if mode in ("residual", "alias") else None
    d = dict(O=R.rmsnorm_bias(xh, wh, bh, rh, act), O_v=R.rmsnorm_bias_variant(xh, wh, bh, rh, act))
    tag = f"norm-fuzz seed {seed}: {_geo(c)}"
    for dtype, fn in ((BF, cdll.ug_rmsnorm_bias_rows), (F32, cdll.ug_rmsnorm_bias_rows_f32)):
        _, x = KT._operand(xh, dtype, gpu, c["pad_x"])
        w, b = wh.to(dtype).to(gpu), bh.to(dtype).to(gpu)
        out = KT._output(rows, C, dtype, gpu, c["pad_o"])
        r = None
        if rh is not None and not alias:
            _, r = KT._operand(rh, dtype, gpu, c["pad_r"])

        def refill():
            if alias:                         # the residual sits in the output buffer and is overwritten by the sum
                out[:rows, :C] = rh.to(dtype).to(gpu)
        refill()
        rp, ldr = (out.data_ptr(), out.stride(0)) if alias else (r.data_ptr(), r.stride(0)) if r is not None else (None, 0)

        def launch():
            ULIB.check(fn(x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), rp, ldr, out.data_ptr(), out.stride(0), rows, C, R.EPS_NORM, act, KT._stream()),
                       tag)
        launch()
        torch.cuda.synchronize()
        got, intact = KT._window(out, rows, C)
        KT._judge((tag, dtype), got, d, dtype, intact, RECORD)
        if act:
            assert bool((got >= 0).all()), tag
        KT._twice_and_replayed(launch, out, refill if alias else None)


# ---------------------------------------------------------------- shortcuts -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
def test_dc_shortcut_random_geometries(gpu, seed):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    c = draw_sc(seed)
    up, f, Cin, Cout, B, H, W, mode = (c[k] for k in ("up", "f", "Cin", "Cout", "B", "H", "W", "mode"))
    assert sc_accepted(up, Cin, Cout, f) and (up or (H % f == 0 and W % f == 0))
    g = torch.Generator().manual_seed(9300 + seed)
    hh = torch.randn(B, H, W, Cin, generator=g).to(BF)
    xh = None
    if mode == "x":
        xh = torch.randn((B, H * f, W * f, Cout) if up else (B, H // f, W // f, Cout), generator=g).to(BF)
    elif mode == "xshuffle":                  # Cout / f^2 channels may be no multiple of 8: the row stride still is (_operand pads it)
        xh = torch.randn(B, H, W, Cout * f * f if up else Cout // (f * f), generator=g).to(BF)
    xs = mode == "xshuffle"
    fn64, fnv = (R.shortcut_up, R.shortcut_up_variant) if up else (R.shortcut_down, R.shortcut_down_variant)
    d = dict(O=fn64(hh, Cout, f, xh, xs), O_v=fnv(hh, Cout, f, xh, xs))
    exact = xh is None and (up or Cin * f * f == Cout)
    rows_o = B * H * W * f * f if up else B * (H // f) * (W // f)
    base = "ug_dc_shortcut_up" if up else "ug_dc_shortcut_down"
    tag = f"{'up' if up else 'down'}-fuzz seed {seed}: {_geo(c)}"
    for dtype, fn in ((BF, getattr(cdll, base)), (F32, getattr(cdll, base + "_f32"))):
        _, h = KT._operand(hh.reshape(-1, Cin), dtype, gpu)
        x = None
        if xh is not None:
            _, x = KT._operand(xh.reshape(-1, xh.shape[-1]), dtype, gpu, 2 * KT.PAD)
        out = KT._output(rows_o, Cout, dtype, gpu)

        def launch():
            ULIB.check(fn(h.data_ptr(), h.stride(0), x.data_ptr() if x is not None else None, x.stride(0) if x is not None else 0, 1 if xs else 0,
                          out.data_ptr(), out.stride(0), B, H, W, Cin, Cout, f, KT._stream()), tag)
        launch()
        torch.cuda.synchronize()
        got, intact = KT._window(out, rows_o, Cout)
        KT._judge((tag, dtype), got, d, dtype, intact, RECORD)
        if exact:
            assert torch.equal(got.double().reshape(d["O"].shape), d["O"]), ("a pure copy must be bit for bit", tag, dtype)
        KT._twice_and_replayed(launch, out)
