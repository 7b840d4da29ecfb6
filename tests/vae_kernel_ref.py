"""CPU float64 references of the AutoencoderKL kernels (csrc/vae.hip and the CONV mode of gemm256_kernel): the implicit-GEMM convolution,
GroupNorm (+ SiLU), the row softmax, the two layout changes and the latent sampling; plus the seeded case generators of the GPU sweep
(tests/test_fuzz_vae_gpu.py), kept here so that tests/test_vae_kernel_ref_cpu.py can draw the same cases without a GPU.

Every function takes the operands exactly as the kernel sees them (bf16 or fp32 values, widened to float64 here; fp32 scalars as their fp32
values) and returns `truth` - the exact result, nothing rounded - and a rounding-point `variant`: the same formula in fp32 with a bf16 rounding
wherever include/unigen_hip.h or the kernel's comment states one. The GPU sweep bounds a bf16 kernel by 1.5 x that variant's own error against
the truth. The convolution is written from the index formula of `ug_conv_desc`'s comment as a gather over (ky, kx), not on F.conv2d: it is an
independent restatement of the coordinate arithmetic. tests/test_vae_kernel_ref_cpu.py checks everything here against torch in float64."""
import random

import torch

from tests.bwd_ref import F64, bf16, bf16_ulp, err  # noqa: F401  (re-exported for the sweeps)

F32 = torch.float32
OK, BAD_SHAPE, BAD_ALIGN, UNSUPPORTED = 0, -1, -2, -3        # include/unigen_hip.h


def f32(v: float) -> float:
    """a Python scalar as the fp32 value the C ABI receives"""
    return float(torch.tensor(v, dtype=F32))


def rows_of(t: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """the rows (last dimension) of t selected by a boolean mask over its leading dimensions, as a tensor of their own for `err`"""
    return t[mask]


def group_blocks(t: torch.Tensor, G: int) -> torch.Tensor:
    """[B, HW, C] -> [B, G, HW * C / G]: every (sample, group) block as one row for `err`"""
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)


# ----------------------------------------------------------------------------------------------------------------------------------
# metrics and bounds (docs/PARITY_TOLERANCES.md, "AutoencoderKL kernel sweep"): fp32 twins rel-L2 <= 1e-5, every row metric <= 1e-4; bf16
# max(1.5 x the variant's own value of the same metric, 2^-9)
# ----------------------------------------------------------------------------------------------------------------------------------
FLOOR = 2.0 ** -9
F32_TOTAL, F32_ROW = 1e-5, 1e-4


def conv_metrics(got, truth, border) -> dict:
    """[B, Ho, Wo, Cout] (or [M, Cout]) -> rel-L2, worst pixel row, worst row of the last partial 128-row tile, worst border pixel row"""
    n = truth.shape[-1]
    g2, t2, b = got.reshape(-1, n), truth.reshape(-1, n), border.reshape(-1)
    M = t2.shape[0]
    total, worst, tail = err(g2, t2, rows_from=None if M % 128 == 0 else M // 128 * 128)
    return dict(rel_l2=total, worst_row=worst, tail_row=tail, border_row=err(rows_of(g2.cpu(), b), rows_of(t2, b))[1] if bool(b.any()) else 0.0)


def gn_metrics(got, truth, G, slab) -> dict:
    """[B, HW, C] -> rel-L2, worst pixel row, worst row of a sample's last partial slab (64 rows generic, 256 fast), worst (sample, group) block"""
    HW = truth.shape[1]
    total, worst, tail = err(got, truth, rows_from=None if HW % slab == 0 else HW // slab * slab)
    return dict(rel_l2=total, worst_row=worst, tail_row=tail, block=err(group_blocks(got.cpu(), G), group_blocks(truth, G))[1])


def bounds(truth_metrics_of_variant, is_bf16: bool) -> dict:
    if not is_bf16:
        return {k: F32_TOTAL if k == "rel_l2" else F32_ROW for k in truth_metrics_of_variant}
    return {k: max(1.5 * v, FLOOR) for k, v in truth_metrics_of_variant.items()}


def judge(name, m: dict, b: dict, case) -> None:
    """print every metric with its bound, then assert"""
    print(name + ": " + ", ".join(f"{k} {m[k]:.3e} ({b[k]:.3e})" for k in m))
    for k in m:
        assert m[k] <= b[k], (name, k, m[k], b[k], case)


# Share of a bf16 convolution output's elements that may differ from the ROUNDED variant bf16(bf16(acc + bias) + R). A kernel with the documented
# rounding points differs from it only where its fp32 accumulation error carries acc + bias across a bf16 rounding boundary: about
# 2 e / ulp of the elements, e ~ sqrt(K) 2^-24 relative for K <= 49 x 320 products and ulp >= 2^-8 relative, i.e. sqrt(K) 2^-15 <= 0.4 %; five
# times that is allowed. Rounding once, bf16(acc + bias + R), differs on a quarter of the elements. Counted on outputs large enough for a share.
MISMATCH_MAX, MISMATCH_MIN = 0.02, 2048


def mismatch(got, var) -> float:
    """share of elements of `got` (bf16 values) that differ from the variant rounded once more (the kernel's store)"""
    return float((got.to(F64).cpu() != bf16(var)).double().mean())


def excess(m: dict, b: dict) -> float:
    """the largest metric / bound ratio: a wrong result is rejected when this exceeds 1"""
    return max(m[k] / b[k] for k in m)


# ----------------------------------------------------------------------------------------------------------------------------------
# convolution: out[b][oy][ox][n] = R + bf16(bias[n] + sum_{ky,kx,c} x[b][(oy stride + ky - pad_t) >> up][(ox stride + kx - pad_l) >> up][c] w[n][ky][kx][c]),
# taps whose virtual coordinate falls outside [0, H << up) x [0, W << up) contribute zero
# ----------------------------------------------------------------------------------------------------------------------------------
def conv_max_out(size: int, stride: int, pad: int, up: int) -> int:
    """the largest Ho (Wo) conv_check admits: the FIRST tap of the last output pixel still lies inside the (upsampled) input,
    (Ho - 1) stride - pad <= (size << up) - 1"""
    return ((size << up) - 1 + pad) // stride + 1


def conv_check(c: dict, is_bf16: bool) -> int:
    """conv_check of csrc/vae.hip restated: the code ug_conv2d_nhwc[_f32] returns for this geometry (pointers and alignment aside)"""
    if min(c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["Ho"], c["Wo"]) <= 0:
        return BAD_SHAPE
    if not (1 <= c["KH"] <= 7 and 1 <= c["KW"] <= 7 and 1 <= c["stride"] <= 4 and c["pad_t"] >= 0 and c["pad_l"] >= 0 and c["up"] in (0, 1)):
        return UNSUPPORTED
    if (c["Ho"] - 1) * c["stride"] - c["pad_t"] > (c["H"] << c["up"]) - 1 or (c["Wo"] - 1) * c["stride"] - c["pad_l"] > (c["W"] << c["up"]) - 1:
        return BAD_SHAPE
    if is_bf16 and (c["Cin"] % 64 or c["Cout"] % 4):
        return UNSUPPORTED
    return OK


def conv_takes_256(c: dict, zero_page_bytes: int = 4096, min_tiles: int = 1) -> bool:
    """the dispatch condition of ug_conv2d_nhwc for the 256^2 GEMM kernel (gemm_plan's conditions of the convolution route, K >= 3 K-tiles among them), pointers aside"""
    M, ktp = c["B"] * c["Ho"] * c["Wo"], c["Cin"] // 64
    return (conv_check(c, True) == OK and M % 256 == 0 and c["Cout"] % 256 == 0 and c["Cin"] % 64 == 0 and ktp >= 2 and ktp & (ktp - 1) == 0 and
            zero_page_bytes >= 2 * (c["Cin"] + 64) and c["B"] < 256 and c["H"] < 2048 and c["W"] < 2048 and c["Ho"] < 4096 and c["Wo"] < 4096 and
            (M // 256) * (c["Cout"] // 256) >= min_tiles and c["KH"] * c["KW"] * ktp >= 3)


def conv2d(x, w, bias, R, *, Ho, Wo, stride, pad_t, pad_l, up, slip=None):
    """x [B, H, W, Cin], w [Cout, KH, KW, Cin], bias [Cout] or None, R [B, Ho, Wo, Cout] or None ->
    (truth, variant, border): truth = R + bias + conv in float64; variant = bf16(acc + bias) + R, NOT rounded after the residual (the kernel's
    store rounds once: round it when comparing); border [B, Ho, Wo]: output pixels with at least one padding tap.
    slip: one of the wrong gathers / epilogues tests/test_vae_kernel_ref_cpu.py shows the sweep's bounds reject (applies to truth AND variant)."""
    x, w = x.to(F64), w.to(F64)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Hv, Wv = H << up, W << up
    oy, ox = torch.arange(Ho), torch.arange(Wo)
    acc = torch.zeros(B, Ho, Wo, Cout, dtype=F64)
    border = torch.zeros(Ho, Wo, dtype=torch.bool)
    xrows = torch.cat([x.reshape(B * H, W, Cin), torch.zeros(1, W, Cin, dtype=F64)])        # "next_sample": sample b + 1 follows b in memory
    for tap in range(KH * KW):
        ky, kx = divmod(tap, KH if slip == "kykx" else KW)
        py, px = (pad_t + 1, pad_l + 1) if slip == "pad_tl" else (pad_t, pad_t if slip == "pad_t_for_x" else pad_l)
        yv, xv = oy * stride + ky - py, ox * stride + kx - px
        oky, okx = (yv >= 0) & (yv < Hv), (xv >= 0) & (xv < Wv)
        ok = oky[:, None] & okx[None, :]
        border |= ~ok
        if slip == "up_round":
            sy, sx = ((yv.clamp(0, Hv - 1) + 1) >> up).clamp_max(H - 1), ((xv.clamp(0, Wv - 1) + 1) >> up).clamp_max(W - 1)
        else:
            sy, sx = yv.clamp(0, Hv - 1) >> up, xv.clamp(0, Wv - 1) >> up
        if slip == "next_sample":            # no bound on the bottom edge: the row below the last one is the next sample's first
            r = (torch.arange(B)[:, None] * H + (yv.clamp_min(0) >> up)[None, :]).clamp_max(B * H)
            g = xrows[r][:, :, sx] * ((yv >= 0)[:, None] & okx[None, :])[None, :, :, None]
        else:
            g = x[:, sy][:, :, sx]
            if slip != "clamp":
                g = g * ok[None, :, :, None]
        acc += g @ w[:, tap // KW, tap % KW, :].transpose(0, 1)
    if bias is not None:
        acc = acc + bias.to(F64)
    truth, var = acc, bf16(acc)
    if R is not None:
        truth = acc + R.to(F64)
        var = bf16(truth) if slip == "res_before_round" else var + R.to(F64)
    return truth, var, border[None].expand(B, Ho, Wo)


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU): x [B, HW, C], statistics per (sample, group) over HW x C / G, biased variance
# ----------------------------------------------------------------------------------------------------------------------------------
def group_stats(x, G):
    """two-pass mean and biased variance in float64 -> ([B, 1, G, 1], [B, 1, G, 1])"""
    B, HW, C = x.shape
    xg = x.to(F64).reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    return mean, ((xg - mean) ** 2).mean((1, 3), keepdim=True)


def groupnorm(x, gamma, beta, G, eps, silu):
    """-> (truth, variant). variant: the statistics exact, then gn_apply_kernel's fp32 arithmetic on (mean, rstd) as fp32: one bf16 rounding
    after the affine (F.group_norm's output tensor), SiLU in fp32 rounded by the store."""
    B, HW, C = x.shape
    mean, var = group_stats(x, G)
    rstd = torch.rsqrt(var + f32(eps))
    xg = x.to(F64).reshape(B, HW, G, C // G)
    y = ((xg - mean) * rstd).reshape(B, HW, C) * gamma.to(F64) + beta.to(F64)
    truth = y * torch.sigmoid(y) if silu else y
    v = ((xg.to(F32) - mean.to(F32)) * rstd.to(F32)).reshape(B, HW, C) * gamma.to(F32) + beta.to(F32)
    v = v.to(torch.bfloat16).to(F32)
    if silu:
        v = (v / (1.0 + torch.exp(-v))).to(torch.bfloat16).to(F32)
    return truth, v.to(F64)


# ----------------------------------------------------------------------------------------------------------------------------------
# row softmax: P[r][:cols] = softmax(scale S[r][:cols]), S fp32 [rows][ld_s], P [rows][ld_p]; the buffers' columns >= cols are not touched
# ----------------------------------------------------------------------------------------------------------------------------------
def softmax_rows(S, cols, scale):
    """S [rows, ld_s] fp32 -> (truth [rows, cols], variant, arg): variant = fp32 arithmetic as the kernel's (the product scale s rounded to
    fp32, expf of the difference to the row maximum, one division) with the bf16 store; arg = |scale s - max|, the argument of the
    exponential, for the per-element bound."""
    sc = f32(scale)
    t = sc * S[:, :cols].to(F64)
    mx = t.amax(1, keepdim=True)
    truth = torch.softmax(t, 1)
    tf = torch.tensor(sc, dtype=F32) * S[:, :cols].to(F32)
    e = torch.exp(tf - tf.amax(1, keepdim=True))
    var = (e * (1.0 / e.sum(1, keepdim=True))).to(torch.bfloat16)
    return truth, var.to(F64), (t - mx).abs()


def softmax_elem_bound(truth, arg):
    """bf16 per element: one bf16 ulp of the float64 value plus 2^-20 (1 + |scale s - max|) relative (the attn_prob bound of the backward sweep);
    plus 2^-126, the smallest normal number of fp32 and bf16, below which the exponential is flushed to zero"""
    return bf16_ulp(truth) + 2.0 ** -20 * (1.0 + arg) * truth + 2.0 ** -126


# ----------------------------------------------------------------------------------------------------------------------------------
# layouts and sampling
# ----------------------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, Cp, div=0.0, add=0.0):
    """x [B, C, H, W] -> (truth, variant) [B, H W, Cp]: channels >= C zero; div != 0: v / div + add, variant bf16(bf16(v (1 / div)) + add) with
    the reciprocal and both operations in fp32 (torch divides by a Python scalar as a multiplication by the fp32 reciprocal)"""
    B, C, H, W = x.shape
    t = x.to(F64).permute(0, 2, 3, 1).reshape(B, H * W, C)
    v = t.clone()
    if div != 0.0:
        t = t / f32(div) + f32(add)
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(div, dtype=F32)
        v = ((v.to(F32) * inv).to(torch.bfloat16).to(F32) + torch.tensor(add, dtype=F32)).to(torch.bfloat16).to(F64)
    pad = torch.zeros(B, H * W, Cp - C, dtype=F64)
    return torch.cat([t, pad], 2), torch.cat([v, pad], 2)


def nhwc_to_nchw(x, B, C, H, W):
    """x [B H W, Cp] -> [B, C, H, W]: the first C channels"""
    return x.to(F64).reshape(B, H, W, -1)[..., :C].permute(0, 3, 1, 2).contiguous()


def vae_sample(mom, noise, L, shift, scale, slip=None):
    """mom [B, HW, Cp] (mean = channels [0, L), log-variance = [L, 2L)), noise [B, L, HW] -> (truth, variant) [B, L, HW]:
    ((mean + exp(0.5 clamp(logvar, -30, 20)) noise) - shift) scale; variant: every step of vae_sample_kernel rounded to bf16 as it documents -
    bf16(0.5 lv), bf16(exp), bf16(sd noise), bf16(mean + .), bf16(. - shift), bf16(. scale) - in fp32 arithmetic."""
    sh, sc = f32(shift), f32(scale)
    m = mom.to(F64)
    mean, lv = m[..., :L].transpose(1, 2), m[..., L:2 * L].transpose(1, 2)
    if slip != "no_clamp":
        lv = lv.clamp(-30.0, 20.0)
    half = 1.0 if slip == "no_half" else 0.5
    z = mean + torch.exp(half * lv) * noise.to(F64)
    truth = z * sc - sh if slip == "affine_order" else (z - sh) * sc
    r = lambda t: t.to(torch.bfloat16).to(F32)
    sd = r(torch.exp(r(half * lv.to(F32))))
    v = r(mean.to(F32) + r(sd * noise.to(F32)))
    if slip == "affine_order":
        v = r(r(v * torch.tensor(sc, dtype=F32)) - torch.tensor(sh, dtype=F32))
    else:
        v = r(r(v - torch.tensor(sh, dtype=F32)) * torch.tensor(sc, dtype=F32))
    return truth, v.to(F64)


# ----------------------------------------------------------------------------------------------------------------------------------
# the twin's GroupNorm statistics, restated (gn_partial_kernel<float> + gn_finalize_kernel): per channel and 64-row chunk a sequential sum of
# v and v v - in fp32 before the fix, in fp64 after it -, a float64 combine, var = q / n - mean^2, (mean, rstd) stored as fp32
# ----------------------------------------------------------------------------------------------------------------------------------
def twin_group_stats(x, G, eps, fixed):
    """x [B, HW, C] fp32 -> (mean, rstd) as fp32 [B, 1, G, 1], by the twin's arithmetic (fixed: per-thread sums in fp64)"""
    B, HW, C = x.shape
    acc = F64 if fixed else F32
    xa = x.to(F32).to(acc)
    s = torch.zeros(B, C, dtype=F64)
    q = torch.zeros(B, C, dtype=F64)
    for r0 in range(0, HW, 64):
        cs, cq = torch.zeros(B, C, dtype=acc), torch.zeros(B, C, dtype=acc)
        for r in range(r0, min(r0 + 64, HW)):            # sequential, as one thread's loop
            v = xa[:, r]
            cs, cq = cs + v, cq + v * v
        s, q = s + cs.to(F64), q + cq.to(F64)
    n = HW * (C // G)
    mean = s.reshape(B, G, -1).sum(-1) / n
    var = (q.reshape(B, G, -1).sum(-1) / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    return mean.to(F32).reshape(B, 1, G, 1), rstd.to(F32).reshape(B, 1, G, 1)


def normalise_with(x, G, mean, rstd):
    """(x - mean) rstd in fp32 with the given per-(sample, group) statistics: the normalised output before any affine"""
    B, HW, C = x.shape
    return ((x.to(F32).reshape(B, HW, G, C // G) - mean) * rstd).reshape(B, HW, C)


# ----------------------------------------------------------------------------------------------------------------------------------
# the sweep's cases (seeded; drawn identically on the CPU and on the GPU box)
# ----------------------------------------------------------------------------------------------------------------------------------
CONV_SEEDS = 64
CONV_WORK = 1.2e8            # B Ho Wo Cin Cout KH KW of one case: keeps the float64 reference on the host to a fraction of a second
_SIZES = [1, 2, 3, 7, 8, 9, 16, 17, 31]
_COUT = [4 * v for v in (1, 2, 3, 16, 31, 32, 33, 48, 64, 65)]
CONV_REFUSALS = ("Ho", "Wo", "stride", "KH", "KW", "up")


def conv_case(seed: int) -> dict:
    """One convolution case of the sweep. `refuse`: None, or the field that makes conv_check refuse the call (every eighth seed).
    Cin32 / Cout32: the fp32 twin's channel counts (the bf16 kernel's, or values only the twin accepts)."""
    rng = random.Random(seed)
    while True:
        KH, KW = rng.choice([1, 2, 3, 5, 7]), rng.choice([1, 2, 3, 5, 7])
        stride, up = rng.choice([1, 2, 3, 4]), rng.choice([0, 1])
        pad_t, pad_l = rng.randint(0, KH - 1), rng.randint(0, KW - 1)
        H, W, B = rng.choice(_SIZES), rng.choice(_SIZES), rng.choice([1, 2, 3])
        Cin, Cout = rng.choice([64, 128, 192, 256, 320]), rng.choice(_COUT)
        Cin32 = rng.choice([Cin, Cin, 3, 16, 100])
        Cout32 = rng.choice([Cout, Cout, 1, 5, 37, 129])
        Ho, Wo = conv_max_out(H, stride, pad_t, up), conv_max_out(W, stride, pad_l, up)
        if rng.random() < 0.3:
            Ho, Wo = rng.randint(1, Ho), rng.randint(1, Wo)
        c = dict(seed=seed, B=B, H=H, W=W, Cin=Cin, Cout=Cout, Cin32=Cin32, Cout32=Cout32, Ho=Ho, Wo=Wo, KH=KH, KW=KW, stride=stride, pad_t=pad_t, pad_l=pad_l,
                 up=up, bias=rng.random() < 0.7, res=rng.choice(["none", "separate", "alias"]), refuse=None)
        if B * Ho * Wo * max(Cin, Cin32) * max(Cout, Cout32) * KH * KW <= CONV_WORK:
            break
    if seed % 8 == 5:
        f = CONV_REFUSALS[(seed // 8) % len(CONV_REFUSALS)]
        c["refuse"] = f
        c[f] = dict(Ho=conv_max_out(H, stride, pad_t, up) + 1, Wo=conv_max_out(W, stride, pad_l, up) + 1, stride=5, KH=8, KW=8, up=2)[f]
    return c


# the VAE's real call shapes (Cin, Cout) at a small spatial size, each in the three geometries unigen_amd/vae.py uses
VAE_GEOMETRIES = dict(same=dict(stride=1, pad_t=1, pad_l=1, up=0), down=dict(stride=2, pad_t=0, pad_l=0, up=0), up=dict(stride=1, pad_t=1, pad_l=1, up=1))
VAE_CHANNELS = [(64, 128), (128, 128), (128, 256), (512, 512), (128, 8), (512, 32)]


def vae_conv_case(cin: int, cout: int, mode: str) -> dict:
    B, H, W = 2, 6, 5
    g = VAE_GEOMETRIES[mode]
    Ho, Wo = (((H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1) if mode == "down" else (H << g["up"], W << g["up"]))
    return dict(seed=1000 + cin + cout, B=B, H=H, W=W, Cin=cin, Cout=cout, Cin32=cin, Cout32=cout, Ho=Ho, Wo=Wo, KH=3, KW=3, bias=True,
                res="separate" if mode == "same" else "none", refuse=None, **g)


# 256^2 route: every case satisfies conv_takes_256 (asserted by both tests). M = B Ho Wo a multiple of 256, Cout = 256.
def _c256(B, H, W, Cin, KH, KW, stride, pad_t, pad_l, up, Ho, Wo, bias=True, res="none", Cout=256):
    return dict(seed=2000 + 31 * KH + 7 * KW + stride + Cin + B, B=B, H=H, W=W, Cin=Cin, Cout=Cout, Ho=Ho, Wo=Wo, KH=KH, KW=KW, stride=stride, pad_t=pad_t,
                pad_l=pad_l, up=up, bias=bias, res=res, refuse=None)


CONV256_CASES = [
    _c256(1, 16, 16, 256, 1, 1, 1, 0, 0, 0, 16, 16),                              # 1x1, one tap of four K-tiles
    _c256(1, 16, 16, 512, 1, 1, 1, 0, 0, 0, 16, 16, res="separate"),            # 1x1, Cin / 64 = 8
    _c256(1, 16, 16, 128, 1, 3, 1, 0, 1, 0, 16, 16, bias=False),                  # 1x3
    _c256(1, 16, 16, 128, 3, 1, 1, 1, 0, 0, 16, 16, res="alias"),               # 3x1
    _c256(2, 8, 16, 128, 2, 2, 1, 0, 1, 0, 8, 16),                                # 2x2, one-sided padding; 128 pixels per sample: a tile spans both samples
    _c256(1, 16, 16, 128, 5, 5, 1, 2, 2, 0, 16, 16, res="separate"),            # 5x5: 25 taps
    _c256(1, 31, 31, 128, 3, 3, 2, 1, 1, 0, 16, 16),                              # stride 2
    _c256(1, 46, 46, 256, 3, 3, 3, 1, 1, 0, 16, 16),                              # stride 3
    _c256(4, 31, 31, 128, 3, 2, 4, 1, 0, 0, 8, 8),                                # stride 4, 3x2, 64 pixels per sample: a tile spans four samples
    _c256(1, 16, 16, 128, 3, 3, 2, 1, 1, 1, 16, 16, res="alias"),               # up with stride 2
    _c256(3, 16, 16, 128, 3, 3, 1, 1, 1, 0, 16, 16, bias=False, res="separate", Cout=512),   # several tiles in M and N
    _c256(2, 8, 8, 256, 3, 3, 1, 1, 1, 1, 16, 8, res="separate"),               # Upsample2D geometry, Ho Wo = 128: a tile straddles the sample boundary
    _c256(2, 17, 31, 512, 3, 3, 2, 0, 0, 0, 8, 16),                               # Downsample2D geometry (smaller than the input allows), Cin / 64 = 8
    # the high bits of the packed output pixel b << 24 | oy << 12 | ox and of the input coordinates (tests/index_range_cases.py: the last five rows)
    _c256(1, 8, 2016, 128, 3, 3, 1, 1, 1, 1, 16, 4032),                           # Wo = 4032 through the folded upsampling: bits 5-11 of ox
    _c256(1, 2016, 8, 128, 3, 3, 1, 1, 1, 1, 4032, 16),                           # Ho = 4032 the same way: bits 5-11 of oy
    _c256(1, 32, 2040, 128, 3, 3, 1, 1, 1, 0, 32, 2040),                          # W = 2040, no upsampling
    _c256(1, 33, 2047, 128, 3, 3, 2, 1, 1, 0, 16, 1024),                          # stride 2 from W = 2047 to Wo = 1024
    _c256(252, 8, 8, 128, 3, 3, 1, 1, 1, 0, 8, 8),                                # batch indices up to 251 in the top byte
]

GN_SEEDS = 40
GN_C = [8, 32, 64, 128, 192, 256, 320, 512, 1024]
GN_CG = [1, 2, 4, 8, 16, 32]
GN_HW = [1, 3, 63, 64, 65, 255, 256, 257, 1000, 4099]
GN_RATIOS = [0, 1, 4, 16, 64]
GN_DATA = ["offset", "offset", "offset", "magnitudes", "constant", "samples"]
GN_WORK = 2.2e6              # B HW C of one case


def gn_fast(c: dict) -> bool:
    """groupnorm_impl's dispatch to the 16-byte kernels (bf16 only; UG_GN_FAST=0 keeps the generic pair)"""
    return c["C"] in (128, 256, 512) and c["G"] <= 256 and c["C"] // c["G"] in (4, 8, 16)


def gn_case(seed: int) -> dict:
    """One GroupNorm case. Every third seed is drawn from the shapes the fast kernels take. data: how the input is drawn (see gn_data)."""
    rng = random.Random(seed)
    HW = GN_HW[seed % len(GN_HW)]
    while True:
        C = rng.choice([128, 256, 512] if seed % 3 == 0 else GN_C)
        cg = rng.choice([c for c in ([4, 8, 16] if seed % 3 == 0 else GN_CG) if C % c == 0])
        B = rng.choice([1, 2, 3])
        c = dict(seed=seed, B=B, HW=HW, C=C, G=C // cg, silu=rng.random() < 0.5, eps=rng.choice([1e-6, 1e-5]), data=GN_DATA[seed % len(GN_DATA)],
                 ratio=GN_RATIOS[(seed // 2) % len(GN_RATIOS)])
        if c["data"] == "samples":
            c["B"] = B = max(B, 2)
        if B * HW * C <= GN_WORK:
            return c


def gn_data(c: dict, g: torch.Generator):
    """-> (x fp32 [B, HW, C], gamma, beta as bf16 values in fp32).
    offset:     every group has its own standard deviation (0.05 ... 5) and a mean of +-ratio standard deviations
    magnitudes: the channels of one group are 100 x apart in magnitude
    constant:   every sample is one constant (variance 0: the output must be beta, finite)
    samples:    consecutive samples differ by a factor 1000 in scale and in offset, which a cross-sample mix of statistics cannot survive"""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    cg = C // G
    x = torch.randn(B, HW, G, cg, generator=g)
    if cg > 1:               # the two halves of a group differ in spread (0.75 : 1.25; rms 1.03), so that half a group's statistics are not the group's
        x = x * torch.where(torch.arange(cg) < cg // 2, 0.75, 1.25)
    if c["data"] == "offset":
        std = torch.exp(torch.rand(B, 1, G, 1, generator=g) * 4.6 - 3.0)
        sign = torch.where(torch.rand(B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)
        x = std * (x + sign * c["ratio"] * (1.0625 ** 0.5 if cg > 1 else 1.0))
    elif c["data"] == "magnitudes":
        x = x * (100.0 ** (torch.arange(cg) % 2))[None, None, None, :] + 0.5
    elif c["data"] == "constant":
        x = torch.zeros_like(x) + (torch.arange(B, dtype=F32)[:, None, None, None] * 1.7 + 0.3)
    else:
        x = (x + 2.0) * (1000.0 ** (torch.arange(B) % 2).float())[:, None, None, None]
    if c["data"] != "constant":          # neighbouring groups differ 1 : 3 in scale, so that two groups' joint statistics are neither's
        x = x * (1.0 + 2.0 * (torch.arange(G) % 2).float())[None, None, :, None]
    rb = lambda t: t.to(torch.bfloat16).to(F32)
    return x.reshape(B, HW, C).contiguous(), rb(1 + 0.2 * torch.randn(C, generator=g)), rb(0.2 * torch.randn(C, generator=g))


GN_REFUSALS = [dict(B=1, HW=5, C=24, G=1, code=UNSUPPORTED), dict(B=2, HW=9, C=12, G=3, code=UNSUPPORTED), dict(B=1, HW=4, C=96, G=2, code=UNSUPPORTED),
               dict(B=1, HW=7, C=32, G=5, code=BAD_SHAPE)]      # cg = 24 / 48 does not divide 256; C % 8 != 0; G does not divide C

SOFTMAX_COLS = [1, 2, 255, 256, 257, 1000, 1023, 1024, 1025, 2048, 5120, 16384, 17408]
SOFTMAX_SCALES = [512 ** -0.5, 1.0, -0.3]
SOFTMAX_DATA = ["randn", "randn30", "dominant", "equal", "offset"]


def softmax_fast(cols: int, scale: float, ld_s: int, ld_p: int) -> bool:
    """softmax_impl's dispatch to the single-read kernel (bf16 only; UG_SOFTMAX_FAST=0 keeps the generic one; pointers 16-byte aligned)"""
    return cols % 1024 == 0 and cols <= 16384 and scale > 0 and ld_s % 4 == 0 and ld_p % 4 == 0


def softmax_cases():
    """every column count once per row count, cycling scales, data and leading dimensions; plus the fast kernel's column counts with a
    positive scale and every data kind"""
    out, i = [], 0
    for rows in (1, 37):
        for cols in SOFTMAX_COLS:
            wide = i % 2 == 1
            out.append(dict(rows=rows, cols=cols, scale=SOFTMAX_SCALES[i % 3], data=SOFTMAX_DATA[i % 5], ld_s=cols + (12 if wide else 0),
                            ld_p=cols + (8 if wide else 0), seed=i))
            i += 1
    for cols in (1024, 2048, 5120, 16384):
        for data in SOFTMAX_DATA:
            wide = i % 2 == 1
            out.append(dict(rows=5, cols=cols, scale=SOFTMAX_SCALES[i % 2], data=data, ld_s=cols + (12 if wide else 0), ld_p=cols + (8 if wide else 0), seed=i))
            i += 1
    out.append(dict(rows=3, cols=1000, scale=1.0, data="randn", ld_s=1003, ld_p=1001, seed=i))        # odd leading dimensions
    return out


def softmax_data(c: dict, g: torch.Generator):
    """-> (S fp32 [rows, ld_s] with junk beyond cols, S0): S0 is the un-offset score matrix whose softmax the result must equal (data "offset":
    S = S0 + 1e4 exactly - S0 is a multiple of 2^-8 - so the truth of S0 is the truth of S)"""
    rows, cols = c["rows"], c["cols"]
    s = torch.randn(rows, cols, generator=g)
    if c["data"] == "randn30":
        s = s * 30
    elif c["data"] == "dominant":
        s = s * 4
        s[rows // 2, cols // 3] = 60.0
    elif c["data"] == "equal":
        s = torch.full((rows, cols), 1.25)
    s = torch.round(s * 256) / 256
    S = torch.randn(rows, c["ld_s"], generator=g) * 50
    S[:, :cols] = s + 1e4 if c["data"] == "offset" else s
    return S, s


LAYOUT_CASES = [(1, 3, 5, 7, 64), (2, 16, 6, 5, 64), (3, 16, 1, 1, 16), (2, 8, 3, 4, 8), (1, 4, 9, 2, 6)]        # (B, C, H, W, Cp)
SAMPLE_CASES = [dict(B=2, L=16, H=6, W=5, Cp=32, affine=True), dict(B=2, L=16, H=6, W=5, Cp=64, affine=True), dict(B=1, L=16, H=9, W=3, Cp=64, affine=False),
                dict(B=3, L=4, H=1, W=1, Cp=8, affine=False), dict(B=1, L=3, H=4, W=4, Cp=64, affine=True)]


def sample_data(c: dict, g: torch.Generator):
    """moments [B, HW, Cp] with log-variances spread over [-40, 30] (both clamps are reached), noise [B, L, HW]; bf16 values in fp32"""
    B, L, HW, Cp = c["B"], c["L"], c["H"] * c["W"], c["Cp"]
    mom = torch.randn(B, HW, Cp, generator=g)
    mom[..., L:2 * L] = torch.rand(B, HW, L, generator=g) * 70 - 40
    mom[0, 0, L], mom[0, 0, 2 * L - 1] = -40.0, 30.0
    rb = lambda t: t.to(torch.bfloat16).to(F32)
    return rb(mom), rb(torch.randn(B, L, HW, generator=g))


def conv_data(c: dict, g: torch.Generator, cin: int, cout: int):
    """x [B, H, W, cin], w [cout, KH, KW, cin], bias, R [B, Ho, Wo, cout]: bf16 values in float64. Samples differ in scale (1, 3, 9, 27, 81, then
    again from 1: 3^b leaves bf16 beyond b = 80, and a period of five shares no factor with a batch field cut to a power of two) so that a pixel
    read from the wrong sample shows."""
    B, H, W, KH, KW = c["B"], c["H"], c["W"], c["KH"], c["KW"]
    x = torch.randn(B, H, W, cin, generator=g, dtype=F64) * (3.0 ** (torch.arange(B) % 5).to(F64))[:, None, None, None] + 0.25
    w = torch.randn(cout, KH, KW, cin, generator=g, dtype=F64) * (KH * KW * cin) ** -0.5
    b = 0.3 * torch.randn(cout, generator=g, dtype=F64)
    R = torch.randn(B, c["Ho"], c["Wo"], cout, generator=g, dtype=F64)
    return bf16(x), bf16(w), bf16(b) if c["bias"] else None, bf16(R) if c["res"] != "none" else None
