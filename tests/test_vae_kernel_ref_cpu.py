"""tests/vae_kernel_ref.py against torch and the oracle in float64 (no GPU): the references the AutoencoderKL kernel sweep
(tests/test_fuzz_vae_gpu.py) measures the kernels against are right to 1e-12, the sweep's cases cover what they claim, and its bounds - fp32
twins 1e-5 / 1e-4, bf16 max(1.5 x the rounding-point variant's own error, 2^-9) on every metric - lie at least 10 x below the error of each
plausible slip of a kernel, on the sweep's own data. Last, the arithmetic of the fp32 twin's GroupNorm statistics restated before and after
its fix (per-thread sums in fp32 / in fp64) against float64: the reason for that fix, checkable without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import vae_ref as V
from tests import vae_kernel_ref as VR

F64, F32 = torch.float64, torch.float32
TOL = 1e-12


def rel(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm())


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv_inputs(seed, B, H, W, Cin, Cout, KH, KW):
    g = _g(seed)
    return (torch.randn(B, H, W, Cin, generator=g, dtype=F64), torch.randn(Cout, KH, KW, Cin, generator=g, dtype=F64), torch.randn(Cout, generator=g, dtype=F64))


# ----------------------------------------------------------------------------------------------------------------------------------
# references against torch / the oracle
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["same", "down", "up"])
def test_conv_reference_vae_geometries(mode):
    B, H, W, Cin, Cout = 2, 7, 6, 5, 4
    x, w, b = _conv_inputs(1, B, H, W, Cin, Cout, 3, 3)
    xn, wn = _nchw(x), _nchw(w)
    st = {"c.weight": wn, "c.bias": b}
    if mode == "same":
        ref, ora = F.conv2d(xn, wn, b, padding=1), V._conv(st, "c", xn)
    elif mode == "down":         # Downsample2D as the oracle's encoder applies it
        ref = F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, b, stride=2)
        ora = V._conv(st, "c", F.pad(xn, (0, 1, 0, 1), mode="constant", value=0), stride=2, padding=0)
    else:                        # Upsample2D as the oracle's decoder applies it
        ref = F.conv2d(F.interpolate(xn, scale_factor=2.0, mode="nearest"), wn, b, padding=1)
        ora = V._conv(st, "c", F.interpolate(xn, scale_factor=2.0, mode="nearest"))
    Ho, Wo = ref.shape[-2:]
    R = torch.randn(B, Ho, Wo, Cout, generator=_g(2), dtype=F64)
    truth, var, border = VR.conv2d(x, w, b, R, Ho=Ho, Wo=Wo, **VR.VAE_GEOMETRIES[mode])
    assert rel(_nchw(truth), ref + _nchw(R)) <= TOL and rel(_nchw(truth), ora + _nchw(R)) <= TOL
    assert torch.equal(var, VR.bf16(truth - R) + R)
    # border pixels: exactly those whose value changes when the padding is filled with ones instead of zeros
    ones = torch.ones_like(xn)
    pad = dict(same=(1, 1, 1, 1), down=(0, 1, 0, 1), up=(1, 1, 1, 1))[mode]
    src = F.interpolate(ones, scale_factor=2.0, mode="nearest") if mode == "up" else ones
    full = F.conv2d(F.pad(src, pad, value=1.0), torch.ones(1, Cin, 3, 3, dtype=F64), stride=2 if mode == "down" else 1)
    zero = F.conv2d(F.pad(src, pad, value=0.0), torch.ones(1, Cin, 3, 3, dtype=F64), stride=2 if mode == "down" else 1)
    assert torch.equal(border, (full != zero)[:, 0])


@pytest.mark.parametrize("KH,KW,stride,pad", [(1, 1, 1, 0), (3, 3, 1, 1), (5, 3, 2, 1), (2, 7, 3, 0), (7, 2, 4, 1), (5, 5, 1, 2), (1, 3, 2, 0), (3, 1, 1, 0)])
def test_conv_reference_general(KH, KW, stride, pad):
    """symmetric padding `pad` on every side, any kernel / stride: F.conv2d's output size; no bias, no residual on the odd cases"""
    B, H, W, Cin, Cout = 2, 9, 11, 3, 5
    x, w, b = _conv_inputs(3, B, H, W, Cin, Cout, KH, KW)
    ref = F.conv2d(_nchw(x), _nchw(w), b if KH % 2 else None, stride=stride, padding=pad)
    Ho, Wo = ref.shape[-2:]
    truth, var, border = VR.conv2d(x, w, b if KH % 2 else None, None, Ho=Ho, Wo=Wo, stride=stride, pad_t=pad, pad_l=pad, up=0)
    assert rel(_nchw(truth), ref) <= TOL and torch.equal(var, VR.bf16(truth))
    assert bool(border.any()) == (pad > 0 or (Ho - 1) * stride + KH > H or (Wo - 1) * stride + KW > W)
    # fewer output rows / columns than the input allows: the leading block of the same result
    t2, _, _ = VR.conv2d(x, w, b if KH % 2 else None, None, Ho=max(1, Ho - 1), Wo=max(1, Wo - 2), stride=stride, pad_t=pad, pad_l=pad, up=0)
    assert rel(t2, truth[:, :max(1, Ho - 1), :max(1, Wo - 2)]) <= TOL
    # asymmetric (pad_t, pad_l) = torch with the top / left padding alone, cropped to the rows the kernel's bound admits
    t3, _, _ = VR.conv2d(x, w, None, None, Ho=Ho, Wo=Wo, stride=stride, pad_t=KH - 1, pad_l=0, up=0)
    ref3 = F.conv2d(F.pad(_nchw(x), (0, KW, KH - 1, KH)), _nchw(w), None, stride=stride)
    assert rel(_nchw(t3), ref3[:, :, :Ho, :Wo]) <= TOL


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_reference(silu):
    g = _g(4)
    B, HW, C, G = 2, 37, 24, 6
    x = torch.randn(B, HW, C, generator=g, dtype=F64) * 2 + 3
    ga, be = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    ref = F.group_norm(x.transpose(1, 2), G, ga, be, eps=VR.f32(1e-6)).transpose(1, 2)
    truth, var = VR.groupnorm(x, ga, be, G, 1e-6, silu)
    assert rel(truth, F.silu(ref) if silu else ref) <= TOL
    r16 = ref.to(torch.bfloat16).to(F64)
    exp = F.silu(r16).to(torch.bfloat16).to(F64) if silu else r16
    # the variant rounds where F.group_norm / F.silu on bf16 tensors round; its fp32 arithmetic moves isolated elements by one bf16 ulp
    assert ((var - exp).abs() <= VR.bf16_ulp(exp)).all() and float(((var - exp) != 0).double().mean()) < 0.02


def test_resnet_block_from_the_references():
    """the oracle's ResnetBlock2D (GroupNorm + SiLU, 3x3 convolution, twice, 1x1 shortcut, residual) composed from this module's references"""
    cfg = V.VAEConfig(block_out_channels=(8, 16), layers_per_block=1, norm_num_groups=4)
    g = _g(5)
    B, H, W, Ci, Co = 2, 5, 4, 8, 16
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    st = {"r.norm1.weight": rn(Ci), "r.norm1.bias": rn(Ci), "r.conv1.weight": rn(Co, Ci, 3, 3), "r.conv1.bias": rn(Co), "r.norm2.weight": rn(Co),
          "r.norm2.bias": rn(Co), "r.conv2.weight": rn(Co, Co, 3, 3), "r.conv2.bias": rn(Co), "r.conv_shortcut.weight": rn(Co, Ci, 1, 1), "r.conv_shortcut.bias": rn(Co)}
    x = rn(B, H, W, Ci)
    ref = V.resnet_block(st, "r", cfg, _nchw(x))
    nhwc = lambda k: st[k].permute(0, 2, 3, 1)
    same = dict(Ho=H, Wo=W, stride=1, pad_t=1, pad_l=1, up=0)
    h = VR.groupnorm(x.reshape(B, H * W, Ci), st["r.norm1.weight"], st["r.norm1.bias"], 4, 1e-6, True)[0].reshape(B, H, W, Ci)
    h = VR.conv2d(h, nhwc("r.conv1.weight"), st["r.conv1.bias"], None, **same)[0]
    h = VR.groupnorm(h.reshape(B, H * W, Co), st["r.norm2.weight"], st["r.norm2.bias"], 4, 1e-6, True)[0].reshape(B, H, W, Co)
    sc = VR.conv2d(x, nhwc("r.conv_shortcut.weight"), st["r.conv_shortcut.bias"], None, Ho=H, Wo=W, stride=1, pad_t=0, pad_l=0, up=0)[0]
    out = VR.conv2d(h, nhwc("r.conv2.weight"), st["r.conv2.bias"], sc, **same)[0]
    assert rel(_nchw(out), ref) <= 1e-11          # eps as fp32 (the C ABI's argument) against the oracle's Python float: 1e-13 of the statistics


@pytest.mark.parametrize("c", [c for c in VR.softmax_cases() if c["cols"] <= 2048][:12])
def test_softmax_reference(c):
    S, s0 = VR.softmax_data(c, _g(c["seed"]))
    truth, var, arg = VR.softmax_rows(S, c["cols"], c["scale"])
    ref = F.softmax(VR.f32(c["scale"]) * S[:, :c["cols"]].to(F64), dim=1)
    assert truth.shape == (c["rows"], c["cols"]) and rel(truth, ref) <= TOL
    assert rel(VR.softmax_rows(s0, c["cols"], c["scale"])[0], truth) <= 1e-9          # data "offset": S0 + 1e4 is exact, the common offset cancels
    assert ((var - truth).abs() <= VR.softmax_elem_bound(truth, arg)).all()


def test_layout_and_sample_references():
    g = _g(6)
    x = torch.randn(2, 5, 3, 4, generator=g).to(torch.bfloat16)
    t, v = VR.nchw_to_nhwc(x, 8)
    assert torch.equal(t[..., :5], x.to(F64).permute(0, 2, 3, 1).reshape(2, 12, 5)) and not t[..., 5:].any() and torch.equal(t, v)
    assert torch.equal(VR.nhwc_to_nchw(t.reshape(24, 8), 2, 5, 3, 4), x.to(F64))
    t, v = VR.nchw_to_nhwc(x, 8, 0.3611, 0.1159)
    assert rel(t[..., :5], (x.to(F64) / VR.f32(0.3611) + VR.f32(0.1159)).permute(0, 2, 3, 1).reshape(2, 12, 5)) <= TOL
    assert ((v - t).abs()[..., :5] <= VR.bf16_ulp(t[..., :5]) + VR.bf16_ulp(t[..., :5] - VR.f32(0.1159))).all() and not v[..., 5:].any()      # two roundings
    for c in VR.SAMPLE_CASES:
        mom, noise = VR.sample_data(c, g)
        L, HW = c["L"], c["H"] * c["W"]
        lv = mom[..., L:2 * L]
        assert float(lv.min()) < -30 and float(lv.max()) > 20
        sh, sc = (0.1159, 0.3611) if c["affine"] else (0.0, 1.0)
        truth, var = VR.vae_sample(mom, noise, L, sh, sc)
        mo = mom.to(F64).reshape(c["B"], c["H"], c["W"], c["Cp"])[..., :2 * L].permute(0, 3, 1, 2)
        ref = (V.gaussian_sample(mo, noise.to(F64).reshape(c["B"], L, c["H"], c["W"])) - VR.f32(sh)) * VR.f32(sc)
        assert rel(truth.reshape(ref.shape), ref) <= TOL
        mo16 = mo.to(torch.bfloat16)
        ref16 = (V.gaussian_sample(mo16, noise.to(torch.bfloat16).reshape(c["B"], L, c["H"], c["W"])) - sh) * sc          # the oracle's bf16 evaluation
        d = (var.reshape(ref.shape) - ref16.to(F64)).abs()
        # torch's CPU kernels round a Python scalar to bf16 first (tests/test_vae_gpu.py), which `- shift` turns into several ulps where it cancels
        far = d > 2 * VR.bf16_ulp(ref16.to(F64))
        assert float(far.double().mean()) <= (0.03 if c["affine"] else 0.0), c


# ----------------------------------------------------------------------------------------------------------------------------------
# the sweep's cases
# ----------------------------------------------------------------------------------------------------------------------------------
def test_sweep_cases_cover_what_they_claim():
    cs = [VR.conv_case(s) for s in range(VR.CONV_SEEDS)]
    refused = [c for c in cs if VR.conv_check(c, True) != VR.OK or VR.conv_check(dict(c, Cin=c["Cin32"], Cout=c["Cout32"]), False) != VR.OK]
    assert VR.CONV_SEEDS >= 64 and len(refused) <= VR.CONV_SEEDS // 4 and all(c["refuse"] for c in refused) and len(refused) == sum(c["refuse"] is not None for c in cs)
    assert {c["refuse"] for c in refused} == set(VR.CONV_REFUSALS)
    run = [c for c in cs if not c["refuse"]]
    M = [c["B"] * c["Ho"] * c["Wo"] for c in run]
    assert any(m < 128 and c["Cout"] < 128 for m, c in zip(M, run)) and any(m > 128 and 0 < m % 128 <= 40 for m in M) and any(m > 128 and m % 128 >= 88 for m in M)
    for key, vals in (("KH", [1, 2, 3, 5, 7]), ("KW", [1, 2, 3, 5, 7]), ("stride", [1, 2, 3, 4]), ("up", [0, 1]), ("B", [1, 2, 3]), ("Cin", [64, 128, 192, 256, 320]),
                      ("res", ["none", "separate", "alias"]), ("bias", [False, True]), ("Cin32", [3, 16, 100])):
        assert set(vals) <= {c[key] for c in run}, key
    assert any(c["Ho"] < VR.conv_max_out(c["H"], c["stride"], c["pad_t"], c["up"]) for c in run) and any(c["Cout32"] % 2 for c in run)
    assert all(0 <= c["pad_t"] < c["KH"] and 0 <= c["pad_l"] < c["KW"] for c in run)
    for c in VR.CONV256_CASES:
        assert VR.conv_takes_256(c) and not VR.conv_takes_256(dict(c, Cin=192)), c
    assert any(c["B"] > 1 and (c["Ho"] * c["Wo"]) % 256 and (c["B"] * c["Ho"] * c["Wo"]) % 256 == 0 for c in VR.CONV256_CASES)
    assert {c["Cin"] // 64 for c in VR.CONV256_CASES} == {2, 4, 8} and {c["stride"] for c in VR.CONV256_CASES} == {1, 2, 3, 4}
    assert {(1, 1), (1, 3), (3, 1), (2, 2), (5, 5)} <= {(c["KH"], c["KW"]) for c in VR.CONV256_CASES}
    for cin, cout in VR.VAE_CHANNELS:
        for mode in VR.VAE_GEOMETRIES:
            assert VR.conv_check(VR.vae_conv_case(cin, cout, mode), True) == VR.OK
    gs = [VR.gn_case(s) for s in range(VR.GN_SEEDS)]
    assert {c["C"] for c in gs} == set(VR.GN_C) and {c["HW"] for c in gs} == set(VR.GN_HW) and {c["C"] // c["G"] for c in gs} == set(VR.GN_CG)
    assert {c["ratio"] for c in gs if c["data"] == "offset"} == set(VR.GN_RATIOS) and {c["data"] for c in gs} == set(VR.GN_DATA)
    assert sum(VR.gn_fast(c) for c in gs) >= 10 and {c["B"] for c in gs} == {1, 2, 3} and {c["eps"] for c in gs} == {1e-6, 1e-5}
    sm = VR.softmax_cases()
    assert {c["cols"] for c in sm} == set(VR.SOFTMAX_COLS) and {c["rows"] for c in sm} >= {1, 37}
    assert sum(VR.softmax_fast(c["cols"], c["scale"], c["ld_s"], c["ld_p"]) for c in sm) >= 8
    assert any(c["scale"] < 0 and c["cols"] % 1024 == 0 for c in sm) and any(c["ld_s"] > c["cols"] for c in sm)


# ----------------------------------------------------------------------------------------------------------------------------------
# sensitivity: each slip exceeds the bound it is judged by at least 10 x
# ----------------------------------------------------------------------------------------------------------------------------------
def _conv_excess(c, slip, border_only):
    g = _g(5000 + c["seed"])
    x, w, b, R = VR.conv_data(c, g, c["Cin"], c["Cout"])
    geo = {k: c[k] for k in ("Ho", "Wo", "stride", "pad_t", "pad_l", "up")}
    truth, var, border = VR.conv2d(x, w, b, R, **geo)
    _, bad, _ = VR.conv2d(x, w, b, R, slip=slip, **geo)
    if torch.equal(VR.bf16(bad), VR.bf16(var)):
        return None                                   # the slip does not touch this geometry
    m, bd = VR.conv_metrics(VR.bf16(bad), truth, border), VR.bounds(VR.conv_metrics(VR.bf16(var), truth, border), True)
    return m["border_row"] / bd["border_row"] if border_only else VR.excess(m, bd)


@pytest.mark.parametrize("slip,border_only", [("clamp", True), ("pad_tl", False), ("up_round", False), ("kykx", False), ("pad_t_for_x", False),
                                              ("res_before_round", False), ("next_sample", True)])
def test_conv_slips_break_the_bounds(slip, border_only):
    cases = [VR.conv_case(s) for s in range(0, VR.CONV_SEEDS, 2)]
    cases = [c for c in cases if not c["refuse"]] + [VR.vae_conv_case(64, 128, m) for m in VR.VAE_GEOMETRIES]
    if slip == "res_before_round":
        # bf16(acc + bias + R) is one rounding CLOSER to the truth than the documented bf16(acc + bias) + R: no distance to the truth can reject
        # it. The sweep rejects it by the share of elements that differ from the rounded variant (VR.MISMATCH_MAX, on outputs of at least
        # VR.MISMATCH_MIN elements with a residual): a kernel with the documented rounding differs only where fp32 accumulation crosses a tie.
        n = 0
        for c in (VR.conv_case(s) for s in range(VR.CONV_SEEDS)):
            if c["refuse"] or c["B"] * c["Ho"] * c["Wo"] * c["Cout"] < VR.MISMATCH_MIN:
                continue
            c = dict(c, res="separate")
            x, w, b, R = VR.conv_data(c, _g(5000 + c["seed"]), c["Cin"], c["Cout"])
            geo = {k: c[k] for k in ("Ho", "Wo", "stride", "pad_t", "pad_l", "up")}
            var, bad = VR.conv2d(x, w, b, R, **geo)[1], VR.conv2d(x, w, b, R, slip=slip, **geo)[1]
            assert VR.mismatch(VR.bf16(bad), var) >= 10 * VR.MISMATCH_MAX, c
            n += 1
        assert n >= 5
        return
    ex = [(e, c) for c in cases for e in [_conv_excess(c, slip, border_only)] if e is not None]
    assert len(ex) >= 5, (slip, len(ex))
    worst = min(ex, key=lambda t: t[0])
    assert worst[0] >= 10.0, (slip, worst)
    if slip == "pad_tl":                  # Downsample2D's padding on the top / left instead of the bottom / right, on its own geometry
        assert _conv_excess(VR.vae_conv_case(128, 128, "down"), slip, True) >= 10.0


def _gn_excess(c, bad_fn, is_bf16):
    x, ga, be = VR.gn_data(c, _g(6000 + c["seed"]))
    if is_bf16:
        x = x.to(torch.bfloat16).to(F32)
    truth, var = VR.groupnorm(x, ga, be, c["G"], c["eps"], c["silu"])
    bad = bad_fn(x.to(F64), ga.to(F64), be.to(F64), c)
    slab = 256 if is_bf16 and VR.gn_fast(c) else 64
    m = VR.gn_metrics(VR.bf16(bad) if is_bf16 else bad, truth, c["G"], slab)
    return VR.excess(m, VR.bounds(VR.gn_metrics(var, truth, c["G"], slab), is_bf16))


def _gn_with(x, ga, be, c, G=None, unbiased=False, roll=False, silu_first=False):
    G = c["G"] if G is None else G
    B, HW, C = x.shape
    mean, var = VR.group_stats(x, G)
    if unbiased:
        n = HW * C // G
        var = var * n / max(n - 1, 1)
    if roll:
        mean, var = mean.roll(1, 0), var.roll(1, 0)
    y = ((x.reshape(B, HW, G, C // G) - mean) * torch.rsqrt(var + VR.f32(c["eps"]))).reshape(B, HW, C)
    if silu_first:
        y = F.silu(y) * ga + be
        return y
    y = y * ga + be
    return F.silu(y) if c["silu"] else y


def test_groupnorm_slips_break_the_bounds():
    cases = [VR.gn_case(s) for s in range(VR.GN_SEEDS)]
    live = [c for c in cases if c["data"] != "constant" and c["B"] * c["HW"] * c["C"] <= 4e5]
    for c in live:
        for G2 in (c["G"] * 2, c["G"] // 2):            # group width off by a factor 2
            if G2 >= 1 and c["C"] % G2 == 0 and G2 <= c["C"] and c["HW"] * c["C"] // c["G"] > 2:
                assert _gn_excess(c, lambda x, ga, be, c, G2=G2: _gn_with(x, ga, be, c, G=G2), True) >= 10.0, ("group width", G2, c)
        if c["B"] > 1 and c["data"] in ("offset", "samples") and c["HW"] * c["C"] // c["G"] > 2:
            assert _gn_excess(c, lambda x, ga, be, c: _gn_with(x, ga, be, c, roll=True), True) >= 10.0, ("statistics of the other sample", c)
        if c["silu"] and c["HW"] * c["C"] // c["G"] > 2:
            assert _gn_excess(c, lambda x, ga, be, c: _gn_with(x, ga, be, c, silu_first=True), True) >= 10.0, ("SiLU before the affine", c)
    # unbiased variance: a factor sqrt(1 - 1 / n) on a group's output, n = HW C / G elements. At the VAE's 16 K elements per group that is 3e-5,
    # which no bf16 bound can see (floor 2^-9); it is judged on the sweep's small groups (n <= 64) and by the fp32 twin's bound, which sees
    # it up to n ~ 5e4 (1 / (2 n) >= 1e-5).
    small = [c for c in live if 2 < c["HW"] * c["C"] // c["G"] <= 64]
    assert len(small) >= 3
    for c in small:
        assert _gn_excess(c, lambda x, ga, be, c: _gn_with(x, ga, be, c, unbiased=True), False) >= 10.0, ("unbiased variance", c)
    mid = [c for c in live if 64 < c["HW"] * c["C"] // c["G"] <= 4000]
    for c in mid[:6]:
        assert _gn_excess(c, lambda x, ga, be, c: _gn_with(x, ga, be, c, unbiased=True), False) >= 10.0, ("unbiased variance, fp32 bound", c)


def test_softmax_slips_break_the_bounds():
    n = 0
    for c in VR.softmax_cases():
        if c["cols"] > 5120 or c["data"] == "equal" or c["cols"] < 2:
            continue
        S, _ = VR.softmax_data(c, _g(c["seed"]))
        truth, var, arg = VR.softmax_rows(S, c["cols"], c["scale"])
        bd = VR.bounds(dict(zip(("rel_l2", "worst_row"), VR.err(var, truth)[:2])), True)
        tw = dict(rel_l2=VR.F32_TOTAL, worst_row=VR.F32_ROW)
        met = lambda t: dict(zip(("rel_l2", "worst_row"), VR.err(t, truth)[:2]))
        if c["scale"] != 1.0:                                          # scale dropped
            bad = F.softmax(S[:, :c["cols"]].to(F64), 1)
            assert VR.excess(met(VR.bf16(bad)), bd) >= 10.0 and VR.excess(met(bad), tw) >= 10.0, c
            assert ((VR.bf16(bad) - truth).abs() > VR.softmax_elem_bound(truth, arg)).any(), c
            n += 1
        if c["cols"] % 256 and c["cols"] > 256:                        # the last cols % 256 columns left out of the sum
            t = VR.f32(c["scale"]) * S[:, :c["cols"]].to(F64)
            e = torch.exp(t - t.amax(1, keepdim=True))
            bad = e / e[:, :c["cols"] // 256 * 256].sum(1, keepdim=True)
            # one column of 257 or 1025 is 0.4 % / 0.1 % of the sum, below half a bf16 ulp: the fp32 twin (the same kernel template) is what
            # sees it; the bf16 bounds see it where the tail is at least a sixteenth of the row
            assert VR.excess(met(bad), tw) >= 10.0, c
            if c["cols"] % 256 >= c["cols"] // 16:
                assert VR.excess(met(VR.bf16(bad)), bd) >= 10.0, c
                assert ((VR.bf16(bad) - truth).abs() > VR.softmax_elem_bound(truth, arg)).any(), c
            n += 1
    assert n >= 12


def test_sample_and_layout_slips_break_the_bounds():
    g = _g(7)
    for c in VR.SAMPLE_CASES:
        mom, noise = VR.sample_data(c, g)
        sh, sc = (0.1159, 0.3611) if c["affine"] else (0.0, 1.0)
        truth, var = VR.vae_sample(mom, noise, c["L"], sh, sc)
        for slip in ("no_clamp", "no_half") + (("affine_order",) if c["affine"] else ()):
            bad = VR.vae_sample(mom, noise, c["L"], sh, sc, slip=slip)[1]
            far = ((bad - var).abs() > 10 * VR.bf16_ulp(var)) | ~torch.isfinite(bad)
            assert far.any(), (slip, c)                      # the sweep allows one bf16 ulp of the variant per element
            assert VR.err(bad.nan_to_num(posinf=1e300), truth)[0] >= 10 * 1e-6, (slip, c)        # and the twin 1e-6 relative
    for (B, C, H, W, Cp) in VR.LAYOUT_CASES:
        x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
        t, v = VR.nchw_to_nhwc(x, Cp, 0.3611, 0.1159)
        bad = VR.bf16(x.to(F64).permute(0, 2, 3, 1).reshape(B, H * W, C) * VR.f32(0.3611) + VR.f32(0.1159))       # "/ div" as "* div"
        assert ((bad - v[..., :C]).abs() > 10 * VR.bf16_ulp(v[..., :C])).any() and VR.err(bad, t[..., :C])[0] >= 10 * 1e-6
        if Cp > C:                                            # padding channels not zeroed: the sweep compares them with 0 bit for bit
            junk = torch.cat([v[..., :C], torch.full((B, H * W, Cp - C), 1e-30, dtype=F64)], 2)
            assert junk[..., C:].any() and not v[..., C:].any()


# ----------------------------------------------------------------------------------------------------------------------------------
# the fp32 twin's GroupNorm statistics, before and after the fix
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [200, 4096])
def test_twin_groupnorm_statistics_before_and_after_the_fix(HW):
    """gn_partial_kernel<float> summed v and v v of 64 rows in fp32 before the fp64 combine. The error is in the statistics - a uniform scale
    (and shift) error of each group's normalised output - so the normalised output (gamma = 1, beta = 0) is compared, rel-L2 against float64,
    at a channel offset of 0 ... 64 standard deviations. Before: inside 1e-5 up to 16, 1.2e-4 at 64 (HW = 200). After (fp64 sums): inside
    1e-5 everywhere, and no worse than torch's fp32 F.group_norm on the same input."""
    B, C, G = 2, 128, 32
    out = {}
    for ratio in VR.GN_RATIOS:
        x = (torch.randn(B, HW, C, generator=_g(8)) + float(ratio)).to(F32)
        mean, var = VR.group_stats(x, G)
        truth = ((x.to(F64).reshape(B, HW, G, C // G) - mean) * torch.rsqrt(var + VR.f32(1e-6))).reshape(B, HW, C)
        e = [VR.err(VR.normalise_with(x, G, *VR.twin_group_stats(x, G, 1e-6, fixed)), truth)[0] for fixed in (False, True)]
        ones, zeros = torch.ones(C), torch.zeros(C)
        e.append(VR.err(F.group_norm(x.transpose(1, 2), G, ones, zeros, eps=1e-6).transpose(1, 2), truth)[0])
        out[ratio] = e
        print(f"HW {HW} offset / std {ratio}: twin before {e[0]:.2e}, after {e[1]:.2e}, torch fp32 {e[2]:.2e}")
        assert e[1] <= VR.F32_TOTAL and e[1] <= max(2 * e[2], 5e-6), (ratio, e)
    assert out[64][0] > VR.F32_TOTAL, out          # the defect: the pre-fix arithmetic misses the twin's own bound at offset / std = 64
    assert all(out[r][0] <= VR.F32_TOTAL for r in (0, 1, 4)), out
