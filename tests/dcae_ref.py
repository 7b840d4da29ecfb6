"""CPU references of the DC-AE kernels (csrc/dcae.hip) and of AutoencoderDC (unigen_amd/dcae.py), and the case lists that
tests/test_dcae_kernels_gpu.py runs and tests/test_dcae_ref_cpu.py checks on the host.

diffusers is not a dependency: the arithmetic is restated from its published semantics (autoencoder_dc.py; SanaMultiscaleLinearAttention and
SanaMultiscaleAttnProcessor2_0; GLUMBConv; RMSNorm with weight and bias), so parity with diffusers is unpinned.

    rmsnorm_bias, msconv, shortcut_down, shortcut_up, silu      float64 (O), written as explicit sums and index maps
    *_variant                                                   the kernels' rounding points (O_v): what include/unigen_hip.h states
    *_slipped                                                   the variant with one deliberate mistake: the host test shows the GPU bounds catch each
    DCAERef                                                     a plain torch module with diffusers' parameter names (float64: the truth; bf16: "the
                                                                reference's own bf16 evaluation")
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from tests import bwd_ref as BR

F64 = torch.float64
BF = torch.bfloat16
DH = 32
EPS_ATTN = 1e-15
EPS_NORM = 1e-5
MARGIN = 1.5                 # the project's standing margin for a kernel that follows its variant's rounding points
MS_TILE_W = 32               # image columns per workgroup of msconv_proj_kernel (MS_W)
MS_TILE_H = 16               # image rows per workgroup (MS_ROWS)


def bounds(O, O_v):
    """(total, worst row) bounds of a bf16 kernel against O: MARGIN x the variant's own error, each"""
    e = BR.err(O_v, O)
    return MARGIN * e[0], MARGIN * e[1]


def _silu(t):
    return t * torch.sigmoid(t)


# ---------------------------------------------------------------- RMSNorm with weight and bias ------------------------------------------------------
# (rows, C, mode, ld pad); mode: plain | residual | alias (the residual is the output buffer) | relu
NORM_SHAPES = [(1, 8), (5, 40), (33, 128), (7, 1024), (3, 4096)]
# the lane groups of rmsnorm_bias_rows_kernel (lpr lanes per row, C / 8 chunks): lpr 2 with a row in a second workgroup; lpr 4 with 3 live chunks;
# lpr 32, the last width below a whole wave; 33 chunks, the first whole-wave width; one chunk in the second pass; all nine passes full
NORM_LANE_SHAPES = [(129, 16), (65, 24), (9, 256), (5, 264), (5, 520), (2, 4608)]
NORM_MODES = ("plain", "residual", "alias", "relu")
NORM_SLIPS = ("no_bias", "residual_before_norm", "no_eps", "eps_after_sqrt")
NORM_EPS_SLIPS = NORM_SLIPS[2:]
NORM_SMALL_SCALES = (2.0 ** -10, 2.0 ** -6)      # rows whose mean square (2^-20, 2^-12) lies below and near eps = 1e-5


def norm_old_case_ids():
    """the cases the kernel shipped with: every x ~ N(0, 4), where eps does not matter"""
    return ["norm-%dx%d-%s" % (r, c, m) for (r, c) in NORM_SHAPES for m in NORM_MODES] + ["norm-5x40-plain-ld56", "norm-6x128-zero_row"]


def norm_lane_case_ids():
    return ["norm-%dx%d-%s" % (r, c, m) for (r, c) in NORM_LANE_SHAPES for m in NORM_MODES]


def norm_small_case_ids():
    return ["norm-6x128-plain-small", "norm-6x128-residual-small"]


def norm_case_ids():
    """ids and seeds go by position: new cases are appended"""
    return norm_old_case_ids() + norm_lane_case_ids() + norm_small_case_ids()


_CACHE = {}


def _once(case_id, make):
    if case_id not in _CACHE:
        _CACHE[case_id] = make()
    return _CACHE[case_id]


def norm_case(case_id):
    """-> dict(x [rows, C], w, b [C], r [rows, C] or None, mode, pad, zero_row, O, O_v); computed once per process, read-only"""
    def make():
        parts = case_id.split("-")
        rows, C = (int(t) for t in parts[1].split("x"))
        mode = parts[2] if parts[2] in NORM_MODES else "plain"
        pad = 16 if case_id.endswith("ld56") else 0
        g = torch.Generator().manual_seed(8100 + norm_case_ids().index(case_id))
        x = (2.0 * torch.randn(rows, C, generator=g)).to(BF)
        if case_id.endswith("small"):               # rows 0, 2, 4 at the first scale, 1, 3, 5 at the second
            x = (x.float() * torch.tensor(NORM_SMALL_SCALES).repeat(rows // 2)[:, None]).to(BF)
        zero_row = None
        if case_id.endswith("zero_row"):
            zero_row = 3
            x[zero_row] = 0
        w = (1 + 0.25 * torch.randn(C, generator=g)).to(BF)
        b = (0.3 * torch.randn(C, generator=g)).to(BF)
        r = torch.randn(rows, C, generator=g).to(BF) if mode in ("residual", "alias") else None
        act = 1 if mode == "relu" else 0
        return dict(id=case_id, rows=rows, C=C, mode=mode, pad=pad, zero_row=zero_row, x=x, w=w, b=b, r=r, act=act,
                    O=rmsnorm_bias(x, w, b, r, act), O_v=rmsnorm_bias_variant(x, w, b, r, act))
    return _once(case_id, make)


def rmsnorm_bias(x, w, b, r=None, act=0, eps=EPS_NORM):
    x = x.to(F64)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.to(F64) + b.to(F64)
    if r is not None:
        return y + r.to(F64)
    return F.relu(y) if act else y


def rmsnorm_bias_variant(x, w, b, r=None, act=0, slip=None, eps=EPS_NORM):
    """y rounded once, then the sum with the residual rounded once. slips - no_bias: the bias is dropped; residual_before_norm: x + r is normalised;
    no_eps: rsqrt(mean) without eps; eps_after_sqrt: 1 / (sqrt(mean) + eps)"""
    assert slip is None or slip in NORM_SLIPS
    x = x.to(F64)
    if slip == "residual_before_norm" and r is not None:
        x = x + r.to(F64)
    ms = (x * x).mean(-1, keepdim=True)
    rs = torch.rsqrt(ms) if slip == "no_eps" else 1 / (torch.sqrt(ms) + eps) if slip == "eps_after_sqrt" else torch.rsqrt(ms + eps)
    y = x * rs * w.to(F64)
    if slip != "no_bias":
        y = y + b.to(F64)
    y = BR.bf16(y)
    if r is not None and slip != "residual_before_norm":
        return BR.bf16(y + r.to(F64))
    return F.relu(y) if act else y


# ---------------------------------------------------------------- multiscale projection ------------------------------------------------------------
# (B, H, W, G); the last is two pixels wider than the kernel's tile: a halo from the neighbouring tile and a ragged last tile
# Then the seams of the 16-row x 32-column tile: one row in a second row tile (its lower halo wholly outside the image); second tiles both ways,
# each narrower than halo + tile; three tiles each way (an interior tile with real halo on all four sides, B = 2, and G = 5: a partial group block
# at NG = 4 and at NG = 2); whole tiles only
MS_SHAPES = [(1, 1, 1, 3), (1, 2, 9, 3), (2, 5, 7, 6), (1, 16, 16, 24), (1, 3, MS_TILE_W + 2, 3),
             (1, 17, 5, 3), (1, 20, 33, 4), (2, 35, 70, 5), (1, 48, 96, 8)]
MS_OLD = 5                   # MS_SHAPES[:MS_OLD] at k = 5 and [1:3] at k = 3 are the cases the kernel shipped with: none has H > MS_TILE_H
MS_SLIPS = ("clamp_padding", "matrix_transposed", "missing_halo_row", "seam_rows_zero", "seam_cols_zero")
MS_SEAM_IDS = ["ms%d-%s" % (k, s) for k in (5, 3) for s in ("1x17x5x3", "1x20x33x4", "2x35x70x5", "1x48x96x8")]
MS_MODEL_LAYOUT_ID = "ms5-2x35x70x5"             # run once more with x and out as column windows of one buffer, as AutoencoderDC calls it


def ms_old_case_ids():
    return ms_case_ids(5)[:MS_OLD] + ms_case_ids(3)[1:3]


def ms_case_ids(k=5):
    return ["ms%d-%dx%dx%dx%d" % ((k,) + s) for s in MS_SHAPES]


def ms_case(case_id):
    """-> dict(x [B, H, W, G 32], w_dw [G 32, 1, k, k], w_pw [G 32, 32, 1, 1] bf16, O, O_v [B, H, W, G 32])"""
    def make():
        head, shape = case_id.split("-")
        k = int(head[2:])
        B, H, W, G = (int(t) for t in shape.split("x"))
        g = torch.Generator().manual_seed(8200 + 10 * k + MS_SHAPES.index((B, H, W, G)))
        x = (1.5 * torch.randn(B, H, W, G * DH, generator=g)).to(BF)
        w_dw = (torch.randn(G * DH, 1, k, k, generator=g) / k).to(BF)
        w_pw = (torch.randn(G * DH, DH, 1, 1, generator=g) / math.sqrt(DH)).to(BF)
        return dict(id=case_id, B=B, H=H, W=W, G=G, k=k, x=x, w_dw=w_dw, w_pw=w_pw, O=msconv(x, w_dw, w_pw), O_v=msconv_variant(x, w_dw, w_pw))
    return _once(case_id, make)


def _same_tile(n, shift, tile):
    """float64 [n]: 1 where position i + shift lies in the tile of i, else 0"""
    i = torch.arange(n)
    return (torch.div(i + shift, tile, rounding_mode="floor") == torch.div(i, tile, rounding_mode="floor")).to(F64)


def _dw(x, w_dw, clamp=False, drop_row=None, seam=None):
    """x [B, H, W, C] float64, w_dw [C, 1, k, k]: depthwise k x k with zero padding k / 2 (clamp: replicated borders), as shifted sums.
    drop_row: the taps of that kernel row are left out (a ring one row short); seam = "rows" / "cols": a tap outside the output pixel's own
    MS_TILE_H-row / MS_TILE_W-column tile reads zero (the neighbouring tile's halo is missing)"""
    B, H, W, C = x.shape
    k = w_dw.shape[-1]
    r = k // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (r, r, r, r), mode="replicate" if clamp else "constant").permute(0, 2, 3, 1)
    y = torch.zeros_like(x)
    for ky in range(k):
        if ky == drop_row:
            continue
        for kx in range(k):
            t = xp[:, ky:ky + H, kx:kx + W, :] * w_dw[:, 0, ky, kx].to(F64)
            if seam == "rows":
                t = t * _same_tile(H, ky - r, MS_TILE_H)[None, :, None, None]
            elif seam == "cols":
                t = t * _same_tile(W, kx - r, MS_TILE_W)[None, None, :, None]
            y = y + t
    return y


def _pw(a, w_pw, transposed=False):
    """a [B, H, W, G 32], w_pw [G 32, 32, 1, 1]: out[.., g 32 + o] = sum_i a[.., g 32 + i] w[g 32 + o][i]"""
    G = a.shape[-1] // DH
    w = w_pw.to(F64).reshape(G, DH, DH)
    if transposed:
        w = w.transpose(1, 2)
    return torch.einsum("bhwgi,goi->bhwgo", a.unflatten(-1, (G, DH)), w).flatten(-2)


def msconv(x, w_dw, w_pw):
    return _pw(_dw(x.to(F64), w_dw), w_pw)


def msconv_variant(x, w_dw, w_pw, slip=None):
    """a = bf16(dwconv), out = bf16(grouped 1x1). slips - clamp_padding: replicated borders; matrix_transposed: w[g][i][o] read as w[g][o][i];
    missing_halo_row: the last kernel row never enters the sum; seam_rows_zero / seam_cols_zero: rows / columns of the neighbouring tile read as zeros"""
    assert slip is None or slip in MS_SLIPS
    a = BR.bf16(_dw(x.to(F64), w_dw, clamp=slip == "clamp_padding", drop_row=w_dw.shape[-1] - 1 if slip == "missing_halo_row" else None,
                    seam={"seam_rows_zero": "rows", "seam_cols_zero": "cols"}.get(slip)))
    return BR.bf16(_pw(a, w_pw, transposed=slip == "matrix_transposed"))


# ---------------------------------------------------------------- shortcuts -------------------------------------------------------------------------
# (B, H, W, Cin, Cout, f): H, W are the input's
# Then the published stage pairs (512 <-> 1024, 512 <-> 512) and the two latent shortcuts (1024 -> 32: a group of 32; 32 -> 1024: 32 repeats), each
# over several workgroups of dc_shortcut_kernel
DOWN_SHAPES = [(1, 2, 2, 8, 16, 2), (2, 4, 6, 16, 16, 2), (1, 2, 2, 64, 256, 2), (2, 3, 5, 64, 8, 1),
               (2, 6, 10, 512, 1024, 2), (1, 4, 6, 512, 512, 2), (2, 9, 11, 1024, 32, 1)]
UP_SHAPES = [(1, 1, 1, 16, 8, 2), (2, 3, 5, 32, 8, 2), (1, 2, 2, 8, 8, 2), (2, 3, 5, 8, 64, 1),
             (2, 3, 5, 1024, 512, 2), (1, 2, 3, 512, 512, 2), (1, 3, 5, 32, 1024, 1)]
SC_OLD = 4                   # the first SC_OLD shapes of each list shipped with the kernel: fewer than 256 threads of work each
SC_MODES = ("nox", "x", "xshuffle")
DOWN_SLIPS = ("channel_order_dydxc", "sum_not_mean")
UP_SLIPS = ("repeat_not_interleave",)


def sc_published_case_ids(up):
    return sc_case_ids(up)[SC_OLD * len(SC_MODES):]


def sc_case_ids(up):
    return ["%s-%dx%dx%dx%dto%dxf%d-%s" % (("up" if up else "down",) + s + (m,)) for s in (UP_SHAPES if up else DOWN_SHAPES) for m in SC_MODES]


def sc_case(case_id):
    """-> dict(h [B, H, W, Cin] bf16, x (layout of the output, or of h's grid under xshuffle) or None, O, O_v, exact: the call is a pure copy)"""
    def make():
        kind, shape, mode = case_id.split("-")
        up = kind == "up"
        dims, rest = shape.split("to")
        B, H, W, Cin = (int(t) for t in dims.split("x"))
        Cout, f = (int(t) for t in rest.split("xf"))
        g = torch.Generator().manual_seed(8300 + sc_case_ids(up).index(case_id) + (100 if up else 0))
        h = torch.randn(B, H, W, Cin, generator=g).to(BF)
        x = None
        if mode == "x":
            x = torch.randn((B, H * f, W * f, Cout) if up else (B, H // f, W // f, Cout), generator=g).to(BF)
        elif mode == "xshuffle":
            x = torch.randn(B, H, W, Cout * f * f if up else Cout // (f * f), generator=g).to(BF)
        fn, fv = (shortcut_up, shortcut_up_variant) if up else (shortcut_down, shortcut_down_variant)
        exact = x is None and (up or Cin * f * f == Cout)
        return dict(id=case_id, up=up, B=B, H=H, W=W, Cin=Cin, Cout=Cout, f=f, mode=mode, h=h, x=x, exact=exact,
                    O=fn(h, Cout, f, x, mode == "xshuffle"), O_v=fv(h, Cout, f, x, mode == "xshuffle"))
    return _once(case_id, make)


def unshuffle(t, f, order="cdydx"):
    """NHWC pixel_unshuffle as an index map: out[.., y, x, c f^2 + dy f + dx] = t[.., f y + dy, f x + dx, c] (order dydxc: (dy f + dx) C + c)"""
    B, H, W, C = t.shape
    out = torch.zeros(B, H // f, W // f, C * f * f, dtype=t.dtype)
    for c in range(C):
        for dy in range(f):
            for dx in range(f):
                m = c * f * f + dy * f + dx if order == "cdydx" else (dy * f + dx) * C + c
                out[..., m] = t[:, dy::f, dx::f, c]
    return out


def shuffle(t, f):
    """NHWC pixel_shuffle: out[.., f y + dy, f x + dx, c] = t[.., y, x, c f^2 + dy f + dx]"""
    B, H, W, C = t.shape
    Co = C // (f * f)
    out = torch.zeros(B, H * f, W * f, Co, dtype=t.dtype)
    for c in range(Co):
        for dy in range(f):
            for dx in range(f):
                out[:, dy::f, dx::f, c] = t[..., c * f * f + dy * f + dx]
    return out


def _down_y(h, Cout, f, slip=None):
    u = unshuffle(h.to(F64), f, "dydxc" if slip == "channel_order_dydxc" else "cdydx")
    g = u.shape[-1] // Cout
    assert g * Cout == u.shape[-1] and g >= 1
    y = torch.zeros(u.shape[:-1] + (Cout,), dtype=F64)
    for j in range(g):
        y = y + u[..., j::g]
    return y if slip == "sum_not_mean" else y / g


def shortcut_down(h, Cout, f, x=None, x_shuffle=False):
    y = _down_y(h, Cout, f)
    if x is None:
        return y
    return y + (unshuffle(x.to(F64), f) if x_shuffle else x.to(F64))


def shortcut_down_variant(h, Cout, f, x=None, x_shuffle=False, slip=None):
    assert slip is None or slip in DOWN_SLIPS
    y = BR.bf16(_down_y(h, Cout, f, slip))
    if x is None:
        return y
    return BR.bf16(y + (unshuffle(x.to(F64), f) if x_shuffle else x.to(F64)))


def _up_y(h, Cout, f, slip=None):
    h = h.to(F64)
    Cin = h.shape[-1]
    r = Cout * f * f // Cin
    assert r * Cin == Cout * f * f and r >= 1
    idx = torch.arange(Cout * f * f) % Cin if slip == "repeat_not_interleave" else torch.arange(Cout * f * f) // r
    return shuffle(h[..., idx], f)


def shortcut_up(h, Cout, f, x=None, x_shuffle=False):
    y = _up_y(h, Cout, f)
    if x is None:
        return y
    return y + (shuffle(x.to(F64), f) if x_shuffle else x.to(F64))


def shortcut_up_variant(h, Cout, f, x=None, x_shuffle=False, slip=None):
    assert slip is None or slip in UP_SLIPS
    y = _up_y(h, Cout, f, slip)
    if x is None:
        return y
    return BR.bf16(y + (shuffle(x.to(F64), f) if x_shuffle else x.to(F64)))


# ---------------------------------------------------------------- SiLU ------------------------------------------------------------------------------
SILU_SIZES = [8, 1000, 1 << 20]


def silu_case_ids():
    return ["silu-%d" % n for n in SILU_SIZES]


def silu_case(case_id):
    """-> dict(x [n] bf16 with +-88 and 0 among N(0, 2) values, O, O_v), judged as rows of 8"""
    def make():
        n = int(case_id.split("-")[1])
        g = torch.Generator().manual_seed(8400 + SILU_SIZES.index(n))
        x = (2.0 * torch.randn(n, generator=g)).to(BF)
        x[1], x[3], x[6] = 88.0, -88.0, 0.0
        O = _silu(x.to(F64))
        return dict(id=case_id, n=n, x=x, O=O, O_v=BR.bf16(O))
    return _once(case_id, make)


# ---------------------------------------------------------------- attention: the two forms and the 96-channel heads --------------------------------
def attn_linear(q, k, v):
    """q, k, v [B, heads, 32, N] float64 (diffusers' layout after the chunk): the padded-value form of apply_linear_attention"""
    q, k = F.relu(q), F.relu(k)
    v1 = F.pad(v, (0, 0, 0, 1), value=1.0)
    o = (v1 @ k.transpose(-1, -2)) @ q
    return o[:, :, :-1] / (o[:, :, -1:] + EPS_ATTN)


def attn_quadratic(q, k, v):
    """apply_quadratic_attention: the branch diffusers takes when H W <= 32"""
    q, k = F.relu(q), F.relu(k)
    s = k.transpose(-1, -2) @ q
    s = s / (s.sum(2, keepdim=True) + EPS_ATTN)
    return v @ s


def heads96(t):
    """[B, 3 C (1 + S), H, W] -> q, k, v [B, heads, 32, H W]: the processor's reshape to [B, -1, 96, H W] and chunk"""
    B, _, H, W = t.shape
    return t.reshape(B, -1, 3 * DH, H * W).chunk(3, 2)


def heads_qkv(t, C):
    """THE SLIP: head g of to_q, to_k and to_v per scale - [B, 3 C (1 + S), H, W] read as (scale, part, head, 32)"""
    B, _, H, W = t.shape
    u = t.reshape(B, -1, 3, C // DH, DH, H * W)
    return tuple(u[:, :, i].reshape(B, -1, DH, H * W) for i in range(3))


def permute_blocks(t, heads):
    """first axis = 3 C channels in diffusers' order: 32-block 3 g + part -> part * heads + g (unigen_amd/dcae.py's load-time permutation)"""
    return t.reshape(heads, 3, DH, -1).permute(1, 0, 2, 3).reshape((3 * heads * DH,) + tuple(t.shape[1:]))


# ---------------------------------------------------------------- the model -------------------------------------------------------------------------
def _up(t):
    """the modules' `.float()` / `.to(torch.float32)`: at least fp32, float64 stays"""
    return t if t.dtype == F64 else t.float()


class _RMSNorm(nn.Module):
    """diffusers' RMSNorm(C, eps, elementwise_affine = True, bias = True) over the last axis"""

    def __init__(self, C):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(C)), nn.Parameter(torch.zeros(C))

    def forward(self, x):
        y = x * torch.rsqrt(_up(x).pow(2).mean(-1, keepdim=True) + EPS_NORM)
        return y.to(self.weight.dtype) * self.weight + self.bias


def _cl(norm, x):
    return norm(x.movedim(1, -1)).movedim(-1, 1)


class _ResBlock(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv1, self.conv2, self.norm = nn.Conv2d(C, C, 3, 1, 1), nn.Conv2d(C, C, 3, 1, 1, bias=False), _RMSNorm(C)

    def forward(self, x):
        return _cl(self.norm, self.conv2(F.silu(self.conv1(x)))) + x


class _MSProj(nn.Module):
    def __init__(self, C, heads, k):
        super().__init__()
        self.proj_in = nn.Conv2d(3 * C, 3 * C, k, padding=k // 2, groups=3 * C, bias=False)
        self.proj_out = nn.Conv2d(3 * C, 3 * C, 1, groups=3 * heads, bias=False)

    def forward(self, x):
        return self.proj_out(self.proj_in(x))


class _MSAttn(nn.Module):
    def __init__(self, C, scales, head_slip=False):
        super().__init__()
        self.C, self.head_slip = C, head_slip
        self.to_q, self.to_k, self.to_v = (nn.Linear(C, C, bias=False) for _ in range(3))
        self.to_qkv_multiscale = nn.ModuleList([_MSProj(C, C // DH, k) for k in scales])
        self.to_out = nn.Linear(C * (1 + len(scales)), C, bias=False)
        self.norm_out = _RMSNorm(C)

    def forward(self, x):
        B, _, H, W = x.shape
        h = x.movedim(1, -1)
        t = torch.cat([self.to_q(h), self.to_k(h), self.to_v(h)], 3).movedim(-1, 1)
        t = torch.cat([t] + [m(t) for m in self.to_qkv_multiscale], 1)
        linear = H * W > DH
        if linear:
            t = _up(t)
        q, k, v = heads_qkv(t, self.C) if self.head_slip else heads96(t)
        o = attn_linear(q, k, v).to(x.dtype) if linear else _quadratic_typed(q, k, v)
        o = self.to_out(o.reshape(B, -1, H, W).movedim(1, -1))
        return self.norm_out(o).movedim(-1, 1) + x


def _quadratic_typed(q, k, v):
    """apply_quadratic_attention with its casts: the scores in fp32, cast back to the value's dtype for the product"""
    q, k = F.relu(q), F.relu(k)
    s = _up(k.transpose(-1, -2) @ q)
    s = s / (s.sum(2, keepdim=True) + EPS_ATTN)
    return v @ s.to(v.dtype)


class _GLUMBConv(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv_inverted = nn.Conv2d(C, 8 * C, 1)
        self.conv_depth = nn.Conv2d(8 * C, 8 * C, 3, 1, 1, groups=8 * C)
        self.conv_point = nn.Conv2d(4 * C, C, 1, bias=False)
        self.norm = _RMSNorm(C)

    def forward(self, x):
        h, gate = self.conv_depth(F.silu(self.conv_inverted(x))).chunk(2, 1)
        return _cl(self.norm, self.conv_point(h * F.silu(gate))) + x


class _EViT(nn.Module):
    def __init__(self, C, scales, head_slip=False):
        super().__init__()
        self.attn, self.conv_out = _MSAttn(C, scales, head_slip), _GLUMBConv(C)

    def forward(self, x):
        return self.conv_out(self.attn(x))


class _Down(nn.Module):
    def __init__(self, cin, cout, unshuffle_):
        super().__init__()
        self.unshuffle, self.group = unshuffle_, cin * 4 // cout
        self.conv = nn.Conv2d(cin, cout // 4 if unshuffle_ else cout, 3, 1 if unshuffle_ else 2, 1)

    def forward(self, h):
        x = self.conv(h)
        if self.unshuffle:
            x = F.pixel_unshuffle(x, 2)
        return x + F.pixel_unshuffle(h, 2).unflatten(1, (-1, self.group)).mean(2)


class _Up(nn.Module):
    def __init__(self, cin, cout, interpolate):
        super().__init__()
        self.interpolate, self.repeats = interpolate, cout * 4 // cin
        self.conv = nn.Conv2d(cin, cout if interpolate else cout * 4, 3, 1, 1)

    def forward(self, h):
        x = self.conv(F.interpolate(h, scale_factor=2, mode="nearest")) if self.interpolate else F.pixel_shuffle(self.conv(h), 2)
        return x + F.pixel_shuffle(h.repeat_interleave(self.repeats, 1), 2)


def _block(kind, C, scales, head_slip):
    return _ResBlock(C) if kind == "ResBlock" else _EViT(C, scales, head_slip)


class _Encoder(nn.Module):
    def __init__(self, c, head_slip):
        super().__init__()
        ch, layers, types, ms = c["encoder_block_out_channels"], c["encoder_layers_per_block"], c["encoder_block_types"], c["encoder_qkv_multiscales"]
        self.conv_in = nn.Conv2d(c["in_channels"], ch[0], 3, 1, 1)
        stages = []
        for i in range(len(ch)):
            mods = [_block(types[i], ch[i], ms[i], head_slip) for _ in range(layers[i])]
            if i < len(ch) - 1:
                mods.append(_Down(ch[i], ch[i + 1], c["downsample_block_type"] == "pixel_unshuffle"))
            stages.append(nn.Sequential(*mods))
        self.down_blocks = nn.ModuleList(stages)
        self.conv_out = nn.Conv2d(ch[-1], c["latent_channels"], 3, 1, 1)
        self.group = ch[-1] // c["latent_channels"]

    def forward(self, x):
        x = self.conv_in(x)
        for s in self.down_blocks:
            x = s(x)
        return self.conv_out(x) + x.unflatten(1, (-1, self.group)).mean(2)


class _Decoder(nn.Module):
    def __init__(self, c, head_slip):
        super().__init__()
        ch, layers, types, ms = c["decoder_block_out_channels"], c["decoder_layers_per_block"], c["decoder_block_types"], c["decoder_qkv_multiscales"]
        self.conv_in = nn.Conv2d(c["latent_channels"], ch[-1], 3, 1, 1)
        self.repeats = ch[-1] // c["latent_channels"]
        stages = []
        for i in range(len(ch)):
            mods = [_Up(ch[i + 1], ch[i], c["upsample_block_type"] == "interpolate")] if i < len(ch) - 1 else []
            mods += [_block(types[i], ch[i], ms[i], head_slip) for _ in range(layers[i])]
            stages.append(nn.Sequential(*mods))
        self.up_blocks = nn.ModuleList(stages)
        self.norm_out = _RMSNorm(ch[0])
        self.conv_out = nn.Conv2d(ch[0], c["in_channels"], 3, 1, 1)

    def forward(self, z):
        x = self.conv_in(z) + z.repeat_interleave(self.repeats, 1)
        for s in reversed(self.up_blocks):
            x = s(x)
        return self.conv_out(F.relu(_cl(self.norm_out, x)))


class DCAERef(nn.Module):
    def __init__(self, head_slip=False, **c):
        super().__init__()
        self.encoder, self.decoder = _Encoder(c, head_slip), _Decoder(c, head_slip)

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z):
        return self.decoder(z)


# ---------------------------------------------------------------- the tiny configurations ----------------------------------------------------------
def _cfg(widths, layers, types, ms, down, up, latent=8):
    n = len(widths)
    return dict(in_channels=3, latent_channels=latent, attention_head_dim=32, encoder_block_types=types, decoder_block_types=types,
                encoder_block_out_channels=widths, decoder_block_out_channels=widths, encoder_layers_per_block=(layers,) * n,
                decoder_layers_per_block=(layers,) * n, encoder_qkv_multiscales=ms, decoder_qkv_multiscales=ms, upsample_block_type=up,
                downsample_block_type=down, decoder_norm_types="rms_norm", decoder_act_fns="silu", scaling_factor=0.41407)


_TYPES = ("ResBlock", "EfficientViTBlock", "EfficientViTBlock")
TINY = {
    "a": _cfg((64, 128, 128), 1, _TYPES, ((), (5,), ()), "Conv", "interpolate"),
    "b": _cfg((64, 128, 256), 2, _TYPES, ((), (5,), (5,)), "pixel_unshuffle", "pixel_shuffle"),
    # the published widths of the attention stages: 16 and 32 heads, G = 48 and 96, GLU at 2048 and 4096 channels, 32 latent channels. 66 M values
    "w": _cfg((512, 1024), 1, ("EfficientViTBlock",) * 2, ((5,), (5,)), "pixel_unshuffle", "pixel_shuffle", latent=32),
}
# (config, image H, W); B = 2 everywhere. "a": 64 and 256 tokens at the attention stages of the 32 x 32 image; "b" at 16 x 16: 16 tokens at the last
# stage, where diffusers takes its quadratic branch
# "w" at 24 x 40: two row and two column tiles of the multiscale projection and N = 960 (four chunks of the linear attention) at width 512, then
# 12 x 20 at width 1024; down 512 -> 1024 (a group of 2), up 1024 -> 512, and the latent shortcuts with a group and a repeat of 32
TINY_RUNS = [("a", 32, 32), ("a", 24, 40), ("b", 16, 16), ("b", 32, 24), ("w", 24, 40)]
RUN_W = 4


def tiny_quantised(name):
    """seeded weights of a tiny model on an 8-bit grid: {key: (int8 tensor, exponent e)}, value = q * 2^e, exact in bf16 (tests/sana_ref.py);
    computed once per process, read-only"""
    def make():
        g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
        out = {}
        for k, t in DCAERef(**TINY[name]).state_dict().items():
            small = k.endswith("bias") or ".norm" in k
            std = 0.2 if small else 1.0 / math.sqrt(t[0].numel())
            e = int(round(math.log2(std * math.sqrt(3.0) / 127.0)))
            out[k] = (torch.randint(-127, 128, t.shape, generator=g, dtype=torch.int8), e)
        return out
    return _once("grid-" + name, make)


def dequantise(k, q, e):
    if ".norm" in k and k.endswith(".weight"):
        v = 1 + torch.div(q.to(torch.int32), 8, rounding_mode="trunc").to(torch.float32) * 2.0 ** -6       # 1 +- 0.25 in steps of 2^-6: exact in bf16
    else:
        v = q.to(torch.float32) * 2.0 ** e
    assert bool((v.to(BF).float() == v).all())
    return v.to(BF)


def tiny_state_dict(name):
    """computed once per process, read-only"""
    return _once("state-" + name, lambda: {k: dequantise(k, q, e) for k, (q, e) in tiny_quantised(name).items()})


def fingerprint(name):
    """int64 [keys, 2]: the sum and the sum of squares of every tensor's grid values in key order - what the fixture pins of the seeded generator"""
    return torch.tensor([[int(q.to(torch.int64).sum()), int((q.to(torch.int64) ** 2).sum())] for q, _ in tiny_quantised(name).values()], dtype=torch.int64)


def tiny_inputs(run):
    """-> dict(x [2, 3, H, W], z [2, latent channels, H / f, W / f]) bf16: the image for encode, latents of their own for decode"""
    name, H, W = TINY_RUNS[run]
    g = torch.Generator().manual_seed(8500 + run)
    f = 2 ** (len(TINY[name]["encoder_block_out_channels"]) - 1)
    return dict(x=torch.randn(2, 3, H, W, generator=g).to(BF), z=torch.randn(2, TINY[name]["latent_channels"], H // f, W // f, generator=g).to(BF))


def build_ref(name, sd, dtype, head_slip=False):
    m = DCAERef(head_slip=head_slip, **TINY[name])
    m.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()})
    return m.to(dtype).eval()


def evaluate(run, dtype=F64, sd=None, head_slip=False):
    """-> (latent of x, image of z) of a run, evaluated in `dtype` on the CPU"""
    name = TINY_RUNS[run][0]
    with torch.no_grad():
        m = build_ref(name, sd if sd is not None else tiny_state_dict(name), dtype, head_slip)
        i = tiny_inputs(run)
        return m.encode(i["x"].to(dtype)), m.decode(i["z"].to(dtype))
