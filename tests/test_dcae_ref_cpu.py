"""tests/dcae_ref.py checked on the host against independent forms, and the proof that the GPU bounds of tests/test_dcae_kernels_gpu.py and
tests/test_dcae_gpu.py catch each plausible slip on a case those tests run.

Independent forms: the depthwise + grouped stage against F.conv2d(groups = ...); the shortcuts against F.pixel_unshuffle / F.pixel_shuffle /
repeat_interleave / unflatten().mean(); the linear attention against the O(N^2) form (also where H W <= 32, diffusers' quadratic branch); the
96-channel head reading against a literal reshape + chunk, and the load-time permutation of the weight rows against it."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import bwd_ref as BR
from tests import dcae_ref as R

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcae_tiny.safetensors")


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("case_id", R.ms_case_ids(5) + R.ms_case_ids(3)[:3])
def test_msconv_against_conv2d(case_id):
    d = R.ms_case(case_id)
    C, k = d["G"] * R.DH, d["k"]
    a = F.conv2d(_nchw(d["x"].to(F64)), d["w_dw"].to(F64), padding=k // 2, groups=C)
    want = _nhwc(F.conv2d(a, d["w_pw"].to(F64), groups=d["G"]))
    assert float((d["O"] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    assert BR.err(d["O_v"], d["O"])[0] > 0                   # the variant does round


@pytest.mark.parametrize("case_id", R.sc_case_ids(False) + R.sc_case_ids(True))
def test_shortcuts_against_torch(case_id):
    d = R.sc_case(case_id)
    h, f, Cout = _nchw(d["h"].to(F64)), d["f"], d["Cout"]
    if d["up"]:
        y = F.pixel_shuffle(h.repeat_interleave(Cout * f * f // d["Cin"], 1), f)
        x = None if d["x"] is None else F.pixel_shuffle(_nchw(d["x"].to(F64)), f) if d["mode"] == "xshuffle" else _nchw(d["x"].to(F64))
    else:
        y = F.pixel_unshuffle(h, f).unflatten(1, (-1, d["Cin"] * f * f // Cout)).mean(2)
        x = None if d["x"] is None else F.pixel_unshuffle(_nchw(d["x"].to(F64)), f) if d["mode"] == "xshuffle" else _nchw(d["x"].to(F64))
    want = _nhwc(y if x is None else x + y)
    assert d["O"].shape == want.shape and float((d["O"] - want).abs().max()) <= 1e-14
    if d["exact"]:
        assert torch.equal(d["O_v"], d["O"]) and torch.equal(d["O"], d["O"].to(R.BF).to(F64))          # a pure copy: bf16 values, untouched


@pytest.mark.parametrize("case_id", R.norm_case_ids())
def test_rmsnorm_against_layer_ops(case_id):
    d = R.norm_case(case_id)
    x = d["x"].to(F64)
    y = x / torch.sqrt(x.pow(2).sum(-1, keepdim=True) / d["C"] + R.EPS_NORM) * d["w"].to(F64) + d["b"].to(F64)
    want = y + d["r"].to(F64) if d["r"] is not None else y.clamp_min(0) if d["act"] else y
    assert float((d["O"] - want).abs().max()) <= 1e-13
    if d["zero_row"] is not None:
        assert torch.equal(d["O_v"][d["zero_row"]], d["b"].to(F64))                                    # a row of zeros: the output is b


def test_silu_reference():
    d = R.silu_case("silu-1000")
    x = d["x"].to(F64)
    assert float((d["O"] - x / (1 + torch.exp(-x))).abs().max()) <= 1e-14
    assert float(d["O"][1]) == 88.0 and float(d["O"][6]) == 0.0 and -1e-35 < float(d["O"][3]) < 0


@pytest.mark.parametrize("shape", [(1, 2, 300), (2, 3, 64), (1, 2, 32), (2, 4, 16), (1, 1, 1)])
def test_linear_form_equals_quadratic_form(shape):
    """the same function in exact arithmetic: to 1e-13 in float64, also at H W <= 32 where diffusers takes the quadratic branch"""
    B, H, N = shape
    g = torch.Generator().manual_seed(8600 + N)
    q, k, v = (torch.randn(B, H, R.DH, N, generator=g, dtype=F64) for _ in range(3))
    a, b = R.attn_linear(q, k, v), R.attn_quadratic(q, k, v)
    assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max()))
    # and against tests/sana_ref.py's form ([B, H, N, 32]), which is what pins ug_linear_attn
    from tests import sana_ref as SR
    c = SR.linear_attention(q.transpose(-1, -2), k.transpose(-1, -2), v.transpose(-1, -2)).transpose(-1, -2)
    assert float((a - c).abs().max()) <= 1e-13 * max(1.0, float(c.abs().max()))


def test_heads_are_96_channel_chunks_and_the_permutation_commutes():
    """head g of a scale = channels [96 g, 96 g + 96) of that scale's tensor; with the weight rows (and proj_in / proj_out alike) permuted in
    32-blocks, the GEMM writes [Q | K | V] with head g at columns [32 g, 32 g + 32) - equal to the literal reshape + chunk to 1e-13"""
    C, B, H, W, k = 128, 2, 3, 5, 5
    heads = C // R.DH
    g = torch.Generator().manual_seed(8700)
    x = torch.randn(B, H, W, C, generator=g, dtype=F64)
    wq, wk, wv = (torch.randn(C, C, generator=g, dtype=F64) / C ** 0.5 for _ in range(3))
    w_in = torch.randn(3 * C, 1, k, k, generator=g, dtype=F64) / k
    w_out = torch.randn(3 * C, R.DH, 1, 1, generator=g, dtype=F64) / R.DH ** 0.5
    # diffusers' order
    t0 = _nchw(torch.cat([x @ wq.t(), x @ wk.t(), x @ wv.t()], -1))
    t1 = F.conv2d(F.conv2d(t0, w_in, padding=k // 2, groups=3 * C), w_out, groups=3 * heads)
    t = torch.cat([t0, t1], 1)
    q, kk, v = R.heads96(t)                                                   # [B, 2 heads, 32, H W]
    lit = t.reshape(B, 2 * heads, 3, R.DH, H * W)                             # the literal reading, written out once more
    assert torch.equal(q, lit[:, :, 0]) and torch.equal(kk, lit[:, :, 1]) and torch.equal(v, lit[:, :, 2])
    # the package's layout
    stack = R.permute_blocks(torch.cat([wq, wk, wv], 0), heads)
    p0 = x @ stack.t()                                                        # [B, H, W, 3 C] = [Q | K | V]
    p1 = R.msconv(p0, R.permute_blocks(w_in, heads), R.permute_blocks(w_out, heads))
    for s, p in enumerate((p0, p1)):
        for part, want in enumerate((q, kk, v)):
            got = p[..., part * C:(part + 1) * C].reshape(B, H * W, heads, R.DH).permute(0, 2, 3, 1)
            ref = want[:, s * heads:(s + 1) * heads]
            assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max())), (s, part)
    # the slip reads other channels
    qs, _, _ = R.heads_qkv(t, C)
    assert float((qs - q).norm() / q.norm()) > 0.5


# ---------------------------------------------------------------- the slips against the GPU bounds -------------------------------------------------
def _caught(O, O_v, bad):
    b_total, b_row = R.bounds(O, O_v)
    total, worst, _ = BR.err(bad, O)
    return total > b_total or worst > b_row


@pytest.mark.parametrize("slip", R.NORM_SLIPS)
def test_norm_slips_exceed_the_bound(slip):
    for cid in ("norm-5x40-residual", "norm-33x128-residual", "norm-7x1024-alias"):
        d = R.norm_case(cid)
        assert _caught(d["O"], d["O_v"], R.rmsnorm_bias_variant(d["x"], d["w"], d["b"], d["r"], d["act"], slip=slip)), (slip, cid)


@pytest.mark.parametrize("slip", R.MS_SLIPS)
def test_msconv_slips_exceed_the_bound(slip):
    for cid in ("ms5-2x5x7x6", "ms5-1x16x16x24", "ms5-1x3x34x3"):
        d = R.ms_case(cid)
        assert _caught(d["O"], d["O_v"], R.msconv_variant(d["x"], d["w_dw"], d["w_pw"], slip=slip)), (slip, cid)


@pytest.mark.parametrize("slip", R.DOWN_SLIPS)
def test_down_slips_exceed_the_bound(slip):
    hit = 0
    for cid in R.sc_case_ids(False):
        d = R.sc_case(cid)
        g = d["Cin"] * d["f"] ** 2 // d["Cout"]
        if d["f"] == 1 and slip == "channel_order_dydxc" or g == 1 and slip == "sum_not_mean":
            continue                                          # the slip is no slip there: one pixel per patch / a group of one
        bad = R.shortcut_down_variant(d["h"], d["Cout"], d["f"], d["x"], d["mode"] == "xshuffle", slip=slip)
        if d["exact"]:
            assert not torch.equal(bad, d["O"]), (slip, cid)
        else:
            assert _caught(d["O"], d["O_v"], bad), (slip, cid)
        hit += 1
    assert hit >= 6


def test_up_slip_exceeds_the_bound():
    hit = 0
    for cid in R.sc_case_ids(True):
        d = R.sc_case(cid)
        if d["Cout"] * d["f"] ** 2 == d["Cin"]:
            continue                                          # r = 1: repeat and repeat_interleave are the same map
        bad = R.shortcut_up_variant(d["h"], d["Cout"], d["f"], d["x"], d["mode"] == "xshuffle", slip="repeat_not_interleave")
        if d["exact"]:
            assert not torch.equal(bad, d["O"]), cid
        else:
            assert _caught(d["O"], d["O_v"], bad), cid
        hit += 1
    assert hit >= 9


@pytest.fixture(scope="module")
def run0():
    return R.evaluate(0)


def test_head_slip_exceeds_the_model_bound(run0):
    """heads read as to_q / to_k / to_v heads: far above the fp32 path's 1e-3 on configuration "a" """
    lat, img = run0
    lat_s, img_s = R.evaluate(0, head_slip=True)
    assert float((lat_s - lat).norm() / lat.norm()) > 1e-2 and float((img_s - img).norm() / img.norm()) > 1e-2


def test_fixture_matches_the_generator(run0):
    from safetensors.torch import load_file
    fx = load_file(GOLDEN)
    assert torch.equal(fx["fingerprint"], R.fingerprint("a")) and [k for k in R.tiny_quantised("a")] == fx_keys(fx)
    for r in (0, 1):
        i = R.tiny_inputs(r)
        assert torch.equal(fx[f"run{r}.x"], i["x"]) and torch.equal(fx[f"run{r}.z"], i["z"])
    lat, img = run0
    assert float((fx["run0.latent"] - lat).abs().max()) <= 1e-12 * float(lat.abs().max())
    assert float((fx["run0.sample"] - img).abs().max()) <= 1e-12 * float(img.abs().max())


def fx_keys(fx):
    return bytes(fx["keys"].tolist()).decode().split("\n")


def test_tiny_weights_are_exact_in_bf16_and_ordinary():
    sd = R.tiny_state_dict("a")
    assert len(sd) == len(R.DCAERef(**R.TINY["a"]).state_dict())
    for k, v in sd.items():
        assert v.dtype == R.BF and bool(torch.isfinite(v).all()), k
    assert abs(float(sd["encoder.down_blocks.0.0.norm.weight"].float().mean()) - 1) < 0.1
