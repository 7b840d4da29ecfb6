"""CPU references of the Sana kernels (csrc/sana.hip) and of the Sana block / base transformer (unigen_amd/sana.py), and the case lists that
tests/test_sana_kernels_gpu.py runs and tests/test_sana_ref_cpu.py checks on the host.

diffusers is not a dependency: the arithmetic is restated from its published semantics (SanaLinearAttnProcessor2_0, GLUMBConv, SanaTransformerBlock,
SanaTransformer2DModel, PatchEmbed's 2-D sin-cos table, AdaLayerNormSingle, PixArtAlphaTextProjection, RMSNorm), so parity with diffusers is unpinned.

    linear_attention(q, k, v)            float64, the two-matmul form of the kernel (state S, z first)
    linear_attention_quadratic(q, k, v)  float64, the independent O(N^2) form
    linear_attention_variant(q, k, v)    the kernel's rounding points: everything exact, the output rounded once to bf16
    glu_dwconv(x, w, b)                  float64, explicit shifted sums (checked against F.conv2d(groups = 2C) by the host test)
    glu_dwconv_variant(x, w, b)          the kernel's rounding points: bf16(silu), bf16(conv + bias), bf16(silu(gate)), bf16(product)
    *_slipped(..., slip)                 the variant with one deliberate mistake: the host tests show that the GPU bounds catch each
    SanaBlockRef, SanaModelRef           plain torch modules with diffusers' parameter names (evaluated in float64 for the truth, in bf16 for "the
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
EPS = 1e-15
MARGIN = 1.5                 # the project's standing margin for a kernel that follows its variant's rounding points
CHUNK = 256                  # tokens per partial state of linattn_state_kernel (LA_CHUNK)

# ---------------------------------------------------------------- linear attention -----------------------------------------------------------------
# (B, H, N): N(0, 1) operands
ATTN_SHAPES = [(1, 1, 1), (1, 2, 33), (2, 3, 64), (1, 4, 257), (2, 8, 1024)]
ATTN_SLIPS = ("no_relu_k", "no_ones_row", "state_bf16", "drop_partial_chunk")


def attn_case_ids():
    return ["gaussian-%dx%dx%d" % s for s in ATTN_SHAPES] + ["scaled8-1x2x4096", "negative_query_row-1x2x33", "negative_key_head-2x3x64", "cancelling-1x2x300"]


_ATTN = {}


def attn_case(case_id):
    """-> dict(q, k, v [B, H, N, 32] bf16, zero: a boolean [B, H, N] of the rows whose output is exactly 0, O, O_v); computed once per process, read-only"""
    if case_id not in _ATTN:
        kind, shape = case_id.split("-")
        B, H, N = (int(x) for x in shape.split("x"))
        g = torch.Generator().manual_seed(7300 + attn_case_ids().index(case_id))
        q, k, v = (torch.randn(B, H, N, DH, generator=g) for _ in range(3))
        zero = torch.zeros(B, H, N, dtype=torch.bool)
        if kind == "scaled8":
            q, k, v = 8 * q, 8 * k, 8 * v
        elif kind == "negative_query_row":
            q[0, 1, 17] = -q[0, 1, 17].abs() - 0.125
            zero[0, 1, 17] = True
        elif kind == "negative_key_head":
            k[1, 2] = -k[1, 2].abs() - 0.125
            zero[1, 2] = True
        elif kind == "cancelling":
            # even tokens: keys live on the even columns, values near +1; odd tokens: keys on the odd columns, values near -0.9; queries near +1. The
            # numerator is a difference of two sums of the denominator's size, so an error made on the STATE (relative to its entries) is about ten
            # times larger relative to the output, while the output's own rounding is not: this is where a state rounded to bf16 shows
            even_n, even_j = (torch.arange(N) % 2 == 0)[:, None], (torch.arange(DH) % 2 == 0)[None, :]
            k = torch.where(even_n == even_j, k.abs() + 0.125, -k.abs() - 0.125)
            v = torch.where(even_n, 1.0, -0.9) * (1 + 0.01 * v)
            q = 1 + 0.05 * q
        q, k, v = q.to(BF), k.to(BF), v.to(BF)
        _ATTN[case_id] = dict(id=case_id, B=B, H=H, N=N, q=q, k=k, v=v, zero=zero, O=linear_attention(q, k, v), O_v=linear_attention_variant(q, k, v))
    return _ATTN[case_id]


def _state(q, k, v):
    q, k, v = F.relu(q.to(F64)), F.relu(k.to(F64)), v.to(F64)
    S = torch.einsum("bhnd,bhnj->bhdj", v, k)
    z = k.sum(-2)
    return q, S, z


def _apply(q, S, z):
    return torch.einsum("bhdj,bhnj->bhnd", S, q) / (torch.einsum("bhj,bhnj->bhn", z, q)[..., None] + EPS)


def linear_attention(q, k, v):
    return _apply(*_state(q, k, v))


def linear_attention_quadratic(q, k, v):
    q, k, v = F.relu(q.to(F64)), F.relu(k.to(F64)), v.to(F64)
    a = q @ k.transpose(-1, -2)                                   # [.., n, m] = q'_n . k'_m
    return (a @ v) / (a.sum(-1, keepdim=True) + EPS)


def linear_attention_variant(q, k, v):
    return BR.bf16(linear_attention(q, k, v))


def linear_attention_slipped(q, k, v, slip):
    """no_relu_k: k enters unrectified;  no_ones_row: the denominator's row of ones is missing from v, the division is by 1;
    state_bf16: S and z rounded to bf16 (the MFMA shortcut);  drop_partial_chunk: the last, partial chunk of CHUNK tokens never reaches the state"""
    assert slip in ATTN_SLIPS
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    if slip == "no_relu_k":
        qq = F.relu(q)
        S, z = torch.einsum("bhnd,bhnj->bhdj", v, k), k.sum(-2)
        return BR.bf16(_apply(qq, S, z))
    if slip == "drop_partial_chunk":
        N = k.shape[-2]
        keep = N // CHUNK * CHUNK if N % CHUNK else N
        qq, S, z = _state(q, k[..., :keep, :], v[..., :keep, :])
        return BR.bf16(_apply(qq, S, z))
    qq, S, z = _state(q, k, v)
    if slip == "no_ones_row":
        return BR.bf16(torch.einsum("bhdj,bhnj->bhnd", S, qq))
    return BR.bf16(_apply(qq, BR.bf16(S), BR.bf16(z)))


def bounds(O, O_v):
    """(total, worst row) bounds of a bf16 kernel against O: MARGIN x the variant's own error, each"""
    e = BR.err(O_v, O)
    return MARGIN * e[0], MARGIN * e[1]


# ---------------------------------------------------------------- GLU depthwise convolution --------------------------------------------------------
# (B, H, W, C, ldo - C)
# the last one is wider than a workgroup's 32-column tile: three tile columns, halo pixels read from the neighbouring tile, a ragged last tile
GLU_SHAPES = [(1, 1, 1, 8, 0), (1, 1, 5, 16, 0), (1, 6, 1, 16, 0), (2, 5, 7, 40, 0), (1, 32, 32, 320, 0), (2, 5, 7, 40, 24), (1, 3, 70, 16, 0)]
GLU_SLIPS = ("silu_after", "halves_swapped", "clamp_padding")


def glu_case_ids():
    return ["glu-%dx%dx%dx%d-pad%d" % s for s in GLU_SHAPES]


_GLU = {}


def glu_case(case_id):
    """-> dict(x [B, H, W, 2C], w [2C, 1, 3, 3], b [2C] bf16, pad, O, O_v [B, H, W, C]); computed once per process, read-only"""
    if case_id not in _GLU:
        _, shape, pad = case_id.split("-")
        B, H, W, C = (int(t) for t in shape.split("x"))
        g = torch.Generator().manual_seed(7400 + glu_case_ids().index(case_id))
        x = (1.5 * torch.randn(B, H, W, 2 * C, generator=g)).to(BF)
        w = (torch.randn(2 * C, 1, 3, 3, generator=g) / 3).to(BF)
        b = (0.2 * torch.randn(2 * C, generator=g)).to(BF)
        _GLU[case_id] = dict(id=case_id, B=B, H=H, W=W, C=C, pad=int(pad[3:]), x=x, w=w, b=b, O=glu_dwconv(x, w, b), O_v=glu_dwconv_variant(x, w, b))
    return _GLU[case_id]


def _silu(t):
    return t * torch.sigmoid(t)


def _dwconv(a, w, b, clamp=False):
    """a [B, H, W, 2C] float64, w [2C, 1, 3, 3], b [2C]: depthwise 3x3, zero padding 1 (clamp: replicated borders instead), as shifted sums"""
    B, H, W, C2 = a.shape
    ap = F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if clamp else "constant").permute(0, 2, 3, 1)
    y = torch.zeros_like(a)
    for ky in range(3):
        for kx in range(3):
            y = y + ap[:, ky:ky + H, kx:kx + W, :] * w[:, 0, ky, kx].to(F64)
    return y + b.to(F64)


def glu_dwconv(x, w, b):
    y = _dwconv(_silu(x.to(F64)), w, b)
    C = y.shape[-1] // 2
    return y[..., :C] * _silu(y[..., C:])


def glu_dwconv_variant(x, w, b, slip=None):
    """the kernel's rounding points. slips - silu_after: the first SiLU moves behind the convolution; halves_swapped: the gate half is taken for the
    value half and the other way round; clamp_padding: the borders are replicated where the convolution pads with zeros"""
    assert slip is None or slip in GLU_SLIPS
    x = x.to(F64)
    if slip == "silu_after":
        y = BR.bf16(_silu(BR.bf16(_dwconv(x, w, b))))
    else:
        y = BR.bf16(_dwconv(BR.bf16(_silu(x)), w, b, clamp=slip == "clamp_padding"))
    C = y.shape[-1] // 2
    val, gate = (y[..., C:], y[..., :C]) if slip == "halves_swapped" else (y[..., :C], y[..., C:])
    return BR.bf16(val * BR.bf16(_silu(gate)))


# ---------------------------------------------------------------- cross attention and the padded head ---------------------------------------------
def softmax_attention(q, k, v, scale, lengths=None):
    """q [B, H, Lq, dh], k, v [B, H, Lkv, dh] float64; lengths[b]: only the first lengths[b] keys of sample b count (a prefix mask)"""
    s = scale * (q.to(F64) @ k.to(F64).transpose(-1, -2))
    if lengths is not None:
        dead = torch.arange(k.shape[-2])[None, :] >= torch.as_tensor(lengths)[:, None]                # [B, Lkv]
        s = s.masked_fill(dead[:, None, None, :], -math.inf)
    return torch.softmax(s, -1) @ v.to(F64)


def pad_width(dh):
    """the slot a cross-attention head of width dh is packed into: the flash kernel has 64 and 128"""
    if dh > 128:
        raise ValueError(dh)
    return 64 if dh <= 64 else 128


# ---------------------------------------------------------------- position table -------------------------------------------------------------------
def sincos_pos_embed(D, H, W, base_size, interpolation_scale):
    """diffusers' get_2d_sincos_pos_embed for an [H, W] token grid, float64 [H * W, D]. Token (y, x) is row y W + x. The meshgrid takes the width grid
    first, so the FIRST half of the channels (diffusers calls it emb_h) is built from the x coordinate and the second half from the y coordinate;
    each half is [sin | cos] of pos * 10000^(-i / (D / 4)), i < D / 4."""
    gy = torch.arange(H, dtype=F64) / (H / base_size) / interpolation_scale
    gx = torch.arange(W, dtype=F64) / (W / base_size) / interpolation_scale
    omega = 10000.0 ** (-torch.arange(D // 4, dtype=F64) / (D / 4))

    def one(pos):
        a = pos[:, None] * omega[None, :]
        return torch.cat([a.sin(), a.cos()], 1)
    X = gx[None, :].expand(H, W).reshape(-1)
    Y = gy[:, None].expand(H, W).reshape(-1)
    return torch.cat([one(X), one(Y)], 1)


# ---------------------------------------------------------------- block and model ------------------------------------------------------------------
def _up(t):
    """the processor's `.float()`: at least fp32, float64 stays"""
    return t if t.dtype == F64 else t.float()


class _Attn(nn.Module):
    def __init__(self, dim, kv_dim, heads, dh, bias):
        super().__init__()
        self.heads, self.dh = heads, dh
        self.to_q = nn.Linear(dim, heads * dh, bias=bias)
        self.to_k = nn.Linear(kv_dim, heads * dh, bias=bias)
        self.to_v = nn.Linear(kv_dim, heads * dh, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(heads * dh, dim, bias=True)])

    def _split(self, t):
        return t.unflatten(-1, (self.heads, self.dh)).transpose(1, 2)

    def linear(self, h):
        q, k, v = (self._split(f(h)) for f in (self.to_q, self.to_k, self.to_v))
        q, k, v = _up(F.relu(q)), _up(F.relu(k)), _up(v)
        v1 = F.pad(v, (0, 1), value=1.0)                                                   # the row of ones
        s = v1.transpose(-1, -2) @ k                                                       # [B, H, dh + 1, dh]
        o = s @ q.transpose(-1, -2)                                                        # [B, H, dh + 1, N]
        o = (o[:, :, :-1] / (o[:, :, -1:] + EPS)).transpose(-1, -2)
        return self.to_out[0](o.transpose(1, 2).flatten(2).to(h.dtype))

    def softmax(self, h, enc, mask, scale=None):
        q, k, v = self._split(self.to_q(h)), self._split(self.to_k(enc)), self._split(self.to_v(enc))
        bias = None
        if mask is not None:
            bias = ((1 - mask.to(h.dtype)) * -10000.0)[:, None, None, :]
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=scale)
        return self.to_out[0](o.transpose(1, 2).flatten(2))


class _GLUMBConv(nn.Module):
    def __init__(self, dim, ratio):
        super().__init__()
        C = int(ratio * dim)
        self.conv_inverted = nn.Conv2d(dim, 2 * C, 1)
        self.conv_depth = nn.Conv2d(2 * C, 2 * C, 3, 1, 1, groups=2 * C)
        self.conv_point = nn.Conv2d(C, dim, 1, bias=False)

    def forward(self, x):
        x = self.conv_depth(F.silu(self.conv_inverted(x)))
        x, gate = x.chunk(2, 1)
        return self.conv_point(x * F.silu(gate))


class SanaBlockRef(nn.Module):
    def __init__(self, dim, num_attention_heads, attention_head_dim, num_cross_attention_heads, cross_attention_head_dim, cross_attention_dim,
                 attention_bias=False, norm_eps=1e-6, mlp_ratio=2.5, cross_scale=None):
        super().__init__()
        self.eps, self.cross_scale = norm_eps, cross_scale
        self.attn1 = _Attn(dim, dim, num_attention_heads, attention_head_dim, attention_bias)
        self.attn2 = _Attn(dim, cross_attention_dim, num_cross_attention_heads, cross_attention_head_dim, True)
        self.ff = _GLUMBConv(dim, mlp_ratio)
        self.scale_shift_table = nn.Parameter(torch.randn(6, dim) / dim ** 0.5)

    def forward(self, h, attention_mask, enc, enc_mask, timestep, height, width):
        B, N, D = h.shape
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = (self.scale_shift_table[None] + timestep.reshape(B, 6, -1)).chunk(6, 1)
        n = F.layer_norm(h, (D,), eps=self.eps) * (1 + sc_a) + sh_a
        h = h + g_a * self.attn1.linear(n.to(h.dtype))
        h = self.attn2.softmax(h, enc, enc_mask, self.cross_scale) + h
        n = F.layer_norm(h, (D,), eps=self.eps) * (1 + sc_m) + sh_m
        f = self.ff(n.unflatten(1, (height, width)).permute(0, 3, 1, 2)).flatten(2, 3).permute(0, 2, 1)
        return h + g_m * f


class _RMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.eps, self.weight = eps, nn.Parameter(torch.ones(dim))

    def forward(self, x):
        y = x * torch.rsqrt(_up(x).pow(2).mean(-1, keepdim=True) + self.eps)
        return y.to(self.weight.dtype) * self.weight


class _Named(nn.Module):
    """a holder that gives its children diffusers' dotted names"""


def timestep_proj(t, dim=256):
    """Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin], in the dtype of t"""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=t.dtype) / half)
    a = t[:, None] * f[None]
    return torch.cat([a.cos(), a.sin()], -1)


class SanaModelRef(nn.Module):
    def __init__(self, in_channels=32, out_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                 cross_attention_head_dim=112, cross_attention_dim=2240, caption_channels=2304, mlp_ratio=2.5, attention_bias=False, sample_size=32,
                 patch_size=1, norm_eps=1e-6, interpolation_scale=None, **ignored):
        super().__init__()
        D = num_attention_heads * attention_head_dim
        self.D, self.p, self.out_channels = D, patch_size, out_channels
        self.base, self.interp, self.eps = sample_size // patch_size, interpolation_scale, norm_eps
        self.patch_embed = _Named()
        self.patch_embed.proj = nn.Conv2d(in_channels, D, patch_size, patch_size)
        self.time_embed = _Named()
        self.time_embed.emb = _Named()
        self.time_embed.emb.timestep_embedder = _Named()
        self.time_embed.emb.timestep_embedder.linear_1 = nn.Linear(256, D)
        self.time_embed.emb.timestep_embedder.linear_2 = nn.Linear(D, D)
        self.time_embed.linear = nn.Linear(D, 6 * D)
        self.caption_projection = _Named()
        self.caption_projection.linear_1 = nn.Linear(caption_channels, D)
        self.caption_projection.linear_2 = nn.Linear(D, D)
        self.caption_norm = _RMSNorm(D, 1e-5)
        self.transformer_blocks = nn.ModuleList([SanaBlockRef(D, num_attention_heads, attention_head_dim, num_cross_attention_heads, cross_attention_head_dim,
                                                              cross_attention_dim, attention_bias, norm_eps, mlp_ratio) for _ in range(num_layers)])
        self.scale_shift_table = nn.Parameter(torch.randn(2, D) / D ** 0.5)
        self.proj_out = nn.Linear(D, patch_size * patch_size * out_channels)

    def forward(self, x, enc, timestep, encoder_attention_mask=None):
        B, _, Hh, Ww = x.shape
        dt = x.dtype
        H, W = Hh // self.p, Ww // self.p
        h = self.patch_embed.proj(x).flatten(2).transpose(1, 2)
        if self.interp is not None:
            pos = sincos_pos_embed(self.D, H, W, self.base, self.interp)
            h = (_up(h) + (pos if dt == F64 else pos.float())[None]).to(dt)
        te = self.time_embed.emb.timestep_embedder
        et = te.linear_2(F.silu(te.linear_1(timestep_proj(_up(timestep)).to(dt))))
        mod = self.time_embed.linear(F.silu(et))
        enc = self.caption_projection.linear_2(F.gelu(self.caption_projection.linear_1(enc), approximate="tanh"))
        enc = self.caption_norm(enc)
        for blk in self.transformer_blocks:
            h = blk(h, None, enc, encoder_attention_mask, mod, H, W)
        shift, scale = (self.scale_shift_table[None] + et[:, None]).chunk(2, 1)
        h = F.layer_norm(h, (self.D,), eps=self.eps) * (1 + scale) + shift
        h = self.proj_out(h)
        p = self.p
        return h.reshape(B, H, W, p, p, self.out_channels).permute(0, 5, 1, 3, 2, 4).reshape(B, self.out_channels, H * p, W * p)


# ---------------------------------------------------------------- the tiny configurations of the fixture -------------------------------------------
TINY = {
    # 4 heads of 32; cross heads of 48 pad to 64; C = 320
    "a": dict(in_channels=8, out_channels=8, num_attention_heads=4, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2, cross_attention_head_dim=48,
              cross_attention_dim=128, caption_channels=64, mlp_ratio=2.5, attention_bias=False, sample_size=8, patch_size=1, norm_eps=1e-6,
              interpolation_scale=1.0),
    # 10 heads of 32; 2 cross heads of 112 pad to 128 (cross width 224 != dim); C = 800 pads to 832; attention_bias on; no position table
    "b": dict(in_channels=4, out_channels=4, num_attention_heads=10, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2, cross_attention_head_dim=112,
              cross_attention_dim=320, caption_channels=64, mlp_ratio=2.5, attention_bias=True, sample_size=8, patch_size=1, norm_eps=1e-6,
              interpolation_scale=None),
}
# (config, H, W, text tokens, prefix lengths or None); B = 2 everywhere
TINY_RUNS = [("a", 4, 6, 5, None), ("a", 8, 8, 12, (12, 1)), ("b", 4, 6, 12, (7, 12)), ("b", 8, 8, 5, None)]


def tiny_quantised(name):
    """seeded weights of a tiny model on an 8-bit grid: {key: (int8 tensor, exponent e)}, value = q * 2^e. Every value is exact in bf16 (8 significant
    bits), so each evaluation - float64, bf16, the GPU's - reads the same numbers, and the fixture stores one byte per weight. The spread is that of
    N(0, 1 / fan_in) for weights (uniform on the grid) and about 0.2 for biases, tables and the norm weight's offset from 1."""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    out = {}
    for k, t in SanaModelRef(**TINY[name]).state_dict().items():
        small = k.endswith("bias") or "scale_shift_table" in k or k.endswith("caption_norm.weight")
        std = 0.2 if small else 1.0 / math.sqrt(t[0].numel())
        e = int(round(math.log2(std * math.sqrt(3.0) / 127.0)))
        out[k] = (torch.randint(-127, 128, t.shape, generator=g, dtype=torch.int8), e)
    return out


def dequantise(k, q, e):
    if k.endswith("caption_norm.weight"):
        v = 1 + torch.div(q.to(torch.int32), 8, rounding_mode="trunc").to(torch.float32) * 2.0 ** -6       # 1 +- 0.25 in steps of 2^-6: exact in bf16
    else:
        v = q.to(torch.float32) * 2.0 ** e
    assert bool((v.to(BF).float() == v).all())
    return v.to(BF)


def tiny_state_dict(name):
    return {k: dequantise(k, q, e) for k, (q, e) in tiny_quantised(name).items()}


def tiny_inputs(run):
    name, H, W, T, lengths = TINY_RUNS[run]
    c = TINY[name]
    g = torch.Generator().manual_seed(7500 + run)
    x = torch.randn(2, c["in_channels"], H, W, generator=g).to(BF)
    enc = torch.randn(2, T, c["caption_channels"], generator=g).to(BF)
    t = torch.tensor([999.0, 37.0])
    mask = None if lengths is None else (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64)
    return dict(x=x, enc=enc, t=t, mask=mask)


def build_ref(name, sd, dtype):
    m = SanaModelRef(**TINY[name])
    m.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()})
    return m.to(dtype).eval()


def block_inputs(run):
    """inputs of block 0 of the run's model: (hidden [2, N, D], enc [2, T, D], timestep [2, 6 D], mask) in bf16"""
    name, H, W, T, lengths = TINY_RUNS[run]
    D = TINY[name]["num_attention_heads"] * 32
    g = torch.Generator().manual_seed(7600 + run)
    mask = None if lengths is None else (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64)
    return dict(h=torch.randn(2, H * W, D, generator=g).to(BF), enc=torch.randn(2, T, TINY[name]["cross_attention_dim"], generator=g).to(BF),
                t=(0.5 * torch.randn(2, 6 * D, generator=g)).to(BF), mask=mask)
