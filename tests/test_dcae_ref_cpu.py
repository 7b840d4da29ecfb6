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


@pytest.mark.parametrize("case_id", R.ms_case_ids(5)[:R.MS_OLD] + R.ms_case_ids(3)[:3] + R.MS_SEAM_IDS)
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
    """what tests/test_dcae_kernels_gpu.py's _judge would refuse: an output that is not finite, or one above either bound"""
    b_total, b_row = R.bounds(O, O_v)
    total, worst, _ = BR.err(bad, O)
    return not bool(torch.isfinite(bad).all()) or total > b_total or worst > b_row


def test_the_new_case_ids_are_the_appended_ones():
    """ids and seeds go by position: the cases that shipped with the kernels keep theirs"""
    assert R.ms_case_ids(5)[R.MS_OLD:] + R.ms_case_ids(3)[R.MS_OLD:] == R.MS_SEAM_IDS and R.MS_MODEL_LAYOUT_ID in R.MS_SEAM_IDS
    assert R.norm_case_ids()[:22] == R.norm_old_case_ids() and R.norm_case_ids()[21] == "norm-6x128-zero_row"
    assert R.norm_lane_case_ids()[0] == "norm-129x16-plain" and R.norm_lane_case_ids()[-1] == "norm-2x4608-relu" and len(R.norm_case_ids()) == 48
    assert R.sc_case_ids(False)[:12][-1] == "down-2x3x5x64to8xf1-xshuffle" and R.sc_case_ids(True)[:12][-1] == "up-2x3x5x8to64xf1-xshuffle"
    assert R.sc_published_case_ids(False)[0] == "down-2x6x10x512to1024xf2-nox" and R.sc_published_case_ids(True)[-1] == "up-1x3x5x32to1024xf1-xshuffle"
    assert R.TINY_RUNS[R.RUN_W] == ("w", 24, 40) and len(R.TINY_RUNS) == 5


def test_lane_cases_reach_the_lane_groups_they_name():
    """lpr as rmsnorm_bias_rows_impl picks it, and the chunk passes (ceil of C / 8 over 64 lanes) of the whole-wave widths"""
    def lpr(C):
        n = 1
        while n < 64 and n < C // 8:
            n *= 2
        return n
    assert [(lpr(C), -(-(C // 8) // 64)) for _, C in R.NORM_LANE_SHAPES] == [(2, 1), (4, 1), (32, 1), (64, 1), (64, 2), (64, 9)]
    assert {lpr(C) for _, C in R.NORM_SHAPES} == {1, 8, 16, 64}                     # what the first cases ran
    rows, C = R.NORM_LANE_SHAPES[0]
    assert rows == 256 // lpr(C) + 1                                                # one row in a second workgroup


def _norm_slipped(cid, slip):
    d = R.norm_case(cid)
    return _caught(d["O"], d["O_v"], R.rmsnorm_bias_variant(d["x"], d["w"], d["b"], d["r"], d["act"], slip=slip))


def _ms_slipped(cid, slip):
    d = R.ms_case(cid)
    return _caught(d["O"], d["O_v"], R.msconv_variant(d["x"], d["w_dw"], d["w_pw"], slip=slip))


@pytest.mark.parametrize("slip", R.NORM_SLIPS[:2])
def test_norm_slips_exceed_the_bound(slip):
    for cid in ["norm-5x40-residual", "norm-33x128-residual", "norm-7x1024-alias"] + [c for c in R.norm_lane_case_ids() + R.norm_small_case_ids()
                                                                                       if "residual" in c or "alias" in c]:
        assert _norm_slipped(cid, slip), (slip, cid)
    if slip == "no_bias":
        for cid in R.norm_lane_case_ids() + R.norm_small_case_ids():
            assert _norm_slipped(cid, slip), (slip, cid)


@pytest.mark.parametrize("slip", R.NORM_EPS_SLIPS)
def test_eps_slips_pass_the_first_cases_and_exceed_the_bound_on_small_rows(slip):
    """THE GAP: at x ~ N(0, 4) the mean square is 4e5 x eps, and an eps that is missing or added after the square root stays inside every bound -
    on all the cases the kernel shipped with and on the lane-group cases alike. The one exception is no_eps on the row of zeros, where rsqrt(0)
    gives a NaN that the finite check refuses: the only place the first suite saw eps at all, and eps_after_sqrt passes it too."""
    for cid in R.norm_old_case_ids() + R.norm_lane_case_ids():
        assert _norm_slipped(cid, slip) == (slip == "no_eps" and cid == "norm-6x128-zero_row"), (slip, cid)
    for cid in R.norm_small_case_ids():
        assert _norm_slipped(cid, slip), (slip, cid)


def test_small_rows_are_below_and_near_eps():
    for cid in R.norm_small_case_ids():
        ms = R.norm_case(cid)["x"].double().pow(2).mean(-1)
        assert bool((ms[0::2] < R.EPS_NORM / 2).all()) and bool((ms[1::2] > 4 * R.EPS_NORM).all()) and bool((ms[1::2] < 400 * R.EPS_NORM).all()), ms


@pytest.mark.parametrize("slip", R.MS_SLIPS[:3])
def test_msconv_slips_exceed_the_bound(slip):
    for cid in ["ms5-2x5x7x6", "ms5-1x16x16x24", "ms5-1x3x34x3"] + R.MS_SEAM_IDS:
        assert _ms_slipped(cid, slip), (slip, cid)


def test_seam_rows_slip_passes_the_first_cases_and_exceeds_the_bound_past_16_rows():
    """THE GAP: no case the kernel shipped with has more than MS_TILE_H rows, so a second row tile whose halo is missing changes nothing there"""
    for cid in R.ms_old_case_ids() + R.ms_case_ids(3)[:R.MS_OLD]:
        assert R.ms_case(cid)["H"] <= R.MS_TILE_H and not _ms_slipped(cid, "seam_rows_zero"), cid
    for cid in R.MS_SEAM_IDS:
        assert _ms_slipped(cid, "seam_rows_zero"), cid


def test_seam_cols_slip_passes_single_column_tiles_and_exceeds_the_bound_past_32_columns():
    """the first cases caught it at W = 34 and k = 5 only (two pixels in the second tile); every new case wider than the tile catches it at both k"""
    for cid in R.ms_case_ids(5) + R.ms_case_ids(3):
        assert _ms_slipped(cid, "seam_cols_zero") == (R.ms_case(cid)["W"] > R.MS_TILE_W), cid
    assert [c for c in R.ms_old_case_ids() if R.ms_case(c)["W"] > R.MS_TILE_W] == ["ms5-1x3x34x3"]
    assert sum(R.ms_case(c)["W"] > 2 * R.MS_TILE_W for c in R.MS_SEAM_IDS) == 4          # an interior column tile, at k = 5 and k = 3


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
    assert hit >= 6 + (6 if slip == "channel_order_dydxc" else 9)


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
    assert hit >= 9 + 9


@pytest.fixture(scope="module")
def run0():
    return R.evaluate(0)


def test_head_slip_exceeds_the_model_bound(run0):
    """heads read as to_q / to_k / to_v heads: far above the fp32 path's 1e-3 on configuration "a" """
    lat, img = run0
    lat_s, img_s = R.evaluate(0, head_slip=True)
    assert float((lat_s - lat).norm() / lat.norm()) > 1e-2 and float((img_s - img).norm() / img.norm()) > 1e-2


def test_head_slip_exceeds_the_model_bound_at_published_widths():
    """the same at 16 and 32 heads (configuration "w", widths 512 and 1024)"""
    assert R.TINY["w"]["encoder_block_out_channels"] == (512, 1024) and R.TINY["w"]["latent_channels"] == 32
    lat, img = R.evaluate(R.RUN_W)
    assert lat.shape == (2, 32, 12, 20) and img.shape == (2, 3, 24, 40)
    from safetensors.torch import load_file
    fx = load_file(GOLDEN)                                                    # the fixture's pair of this run is this evaluation
    assert torch.equal(fx["fingerprint.w"], R.fingerprint("w"))
    i = R.tiny_inputs(R.RUN_W)
    assert torch.equal(fx[f"run{R.RUN_W}.x"], i["x"]) and torch.equal(fx[f"run{R.RUN_W}.z"], i["z"])
    assert float((fx[f"run{R.RUN_W}.latent"] - lat).abs().max()) <= 1e-12 * float(lat.abs().max())
    assert float((fx[f"run{R.RUN_W}.sample"] - img).abs().max()) <= 1e-12 * float(img.abs().max())
    lat_s, img_s = R.evaluate(R.RUN_W, head_slip=True)
    e = float((lat_s - lat).norm() / lat.norm()), float((img_s - img).norm() / img.norm())
    print("head slip at published widths: encode %.3g decode %.3g" % e)
    assert min(e) > 1e-2


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


def test_fuzz_draws_are_inside_what_the_entry_points_accept():
    """tests/test_fuzz_dcae_gpu.py redraws on the host what an entry point must refuse: every draw it sends obeys the documented rules, the norm's
    forced draws are the lane-group edges, and the draws reach second tiles, several workgroups and both directions"""
    from tests import test_fuzz_dcae_gpu as Z
    ms = [Z.draw_ms(s) for s in range(Z.SEEDS)]
    for c in ms:
        assert c["k"] in (3, 5) and 1 <= c["B"] <= 2 and 1 <= c["H"] <= 40 and 1 <= c["W"] <= 80 and 1 <= c["G"] <= 9 and {c["pad_x"], c["pad_o"]} <= {0, 8, 24}
    assert {c["k"] for c in ms} == {3, 5} and any(c["H"] > R.MS_TILE_H for c in ms) and any(c["W"] > 2 * R.MS_TILE_W for c in ms)
    no = [Z.draw_norm(s) for s in range(Z.SEEDS)]
    for s, c in enumerate(no):
        assert 1 <= c["rows"] <= 300 and c["C"] % 8 == 0 and 8 <= c["C"] <= 4608 and c["mode"] in R.NORM_MODES
        assert s % 2 or c["C"] // 8 in Z.NORM_EDGES
    sc = [Z.draw_sc(s) for s in range(Z.SEEDS)]
    for c in sc:
        assert c["Cin"] % 8 == 0 and c["Cout"] % 8 == 0 and max(c["Cin"], c["Cout"]) <= 1024 and c["f"] in (1, 2) and c["mode"] in R.SC_MODES
        num, den = (c["Cout"] * c["f"] ** 2, c["Cin"]) if c["up"] else (c["Cin"] * c["f"] ** 2, c["Cout"])
        assert num % den == 0 and (c["up"] or (c["H"] % c["f"] == 0 and c["W"] % c["f"] == 0)) and 1 <= c["H"] <= 12 and 1 <= c["W"] <= 12
    assert {c["up"] for c in sc} == {False, True} and {c["f"] for c in sc} == {1, 2}
