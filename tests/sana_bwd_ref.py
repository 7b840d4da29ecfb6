"""CPU references of the Sana backward kernels (csrc/sana_bwd.hip): the gradients of tests/sana_ref.linear_attention and glu_dwconv as closed forms in
float64, their rounding variants G_v (what a kernel that follows the stated rounding points computes with exact arithmetic in between), and the
variants with one deliberate mistake each. tests/test_sana_bwd_ref_cpu.py checks all of this on the host over the case lists below;
tests/test_sana_bwd_kernels_gpu.py runs the same cases on the device.

    linear_attention_bwd(q, k, v, do)              -> dict(dq, dk, dv [B, H, N, 32], mag: per tensor the magnitude of the terms that cancel in it)
    glu_dwconv_bwd(x, w, b, do)                    -> dict(dx [B, H, W, 2C], dw [2C, 1, 3, 3], db [2C])
    variant=True                                   the kernels' rounding points: attention - dq, dk, dv rounded once (dS, dz never); convolution -
                                                   a, y, s as the forward rounds them, dy once, dx once, dw / db left exact (they leave the kernel as fp32)
    slip=...                                       the variant with one mistake (ATTN_SLIPS, GLU_SLIPS)
"""
import torch
import torch.nn.functional as F

from tests import bwd_ref as BR
from tests import sana_ref as R

F64 = torch.float64
BF = torch.bfloat16
BWD_CHUNK = 128              # query rows per partial dS of linattn_bwd_q_kernel (LB_ROWS)
SLAB = 256                   # pixels per partial dw9 / dbias of glu_bwd_dw_kernel (GB_SLAB)

ATTN_SLIPS = ("no_q_mask", "no_cz_term", "dstate_bf16", "drop_partial_chunk")
GLU_SLIPS = ("unflipped_taps", "clamp_padding", "halves_swapped", "dbias_one_sample")
# the forward's shapes and (1, 17, 33, 8): ragged against every tile there is (561 pixels: three slabs of 256 that end mid-row; 1-D launches of 256 items)
GLU_SHAPES = R.GLU_SHAPES + [(1, 17, 33, 8, 0)]


def attn_case_ids():
    return R.attn_case_ids()


def glu_case_ids():
    return ["glu-%dx%dx%dx%d-pad%d" % s for s in GLU_SHAPES]


_ATTN, _GLU = {}, {}


def attn_case(case_id):
    """the forward's case plus do ~ N(0, 1) in bf16 and G, G_v: computed once per process, read-only"""
    if case_id not in _ATTN:
        d = dict(R.attn_case(case_id))
        g = torch.Generator().manual_seed(8300 + attn_case_ids().index(case_id))
        d["do"] = torch.randn(d["B"], d["H"], d["N"], R.DH, generator=g).to(BF)
        d["G"] = linear_attention_bwd(d["q"], d["k"], d["v"], d["do"])
        d["G_v"] = linear_attention_bwd(d["q"], d["k"], d["v"], d["do"], variant=True)
        _ATTN[case_id] = d
    return _ATTN[case_id]


def glu_case(case_id):
    if case_id not in _GLU:
        if case_id in R.glu_case_ids():
            d = dict(R.glu_case(case_id))
        else:
            _, shape, pad = case_id.split("-")
            B, H, W, C = (int(t) for t in shape.split("x"))
            g = torch.Generator().manual_seed(8400 + glu_case_ids().index(case_id))
            d = dict(id=case_id, B=B, H=H, W=W, C=C, pad=int(pad[3:]), x=(1.5 * torch.randn(B, H, W, 2 * C, generator=g)).to(BF),
                     w=(torch.randn(2 * C, 1, 3, 3, generator=g) / 3).to(BF), b=(0.2 * torch.randn(2 * C, generator=g)).to(BF))
        g = torch.Generator().manual_seed(8500 + glu_case_ids().index(case_id))
        d["do"] = torch.randn(d["B"], d["H"], d["W"], d["C"], generator=g).to(BF)
        d["G"] = glu_dwconv_bwd(d["x"], d["w"], d["b"], d["do"])
        d["G_v"] = glu_dwconv_bwd(d["x"], d["w"], d["b"], d["do"], variant=True)
        _GLU[case_id] = d
    return _GLU[case_id]


def bounds(G, G_v, mag=None):
    """(total, worst row) of a bf16 kernel against G: the standing margin x the variant's own error, each"""
    e = BR.err(G_v, G, mag)
    return R.MARGIN * e[0], R.MARGIN * e[1]


# ---------------------------------------------------------------- linear attention -----------------------------------------------------------------
def linear_attention_bwd(q, k, v, do, variant=False, slip=None):
    assert slip is None or slip in ATTN_SLIPS
    rnd = BR.bf16 if (variant or slip) else (lambda t: t)
    q, k, v, do = q.to(F64), k.to(F64), v.to(F64), do.to(F64)
    qq, S, z = R._state(q, k, v)                                         # relu(q) [.., n, j], S [.., d, j], z [.., j]
    kk = F.relu(k)
    den = torch.einsum("bhj,bhnj->bhn", z, qq) + R.EPS
    o = torch.einsum("bhdj,bhnj->bhnd", S, qq) / den[..., None]
    g = do / den[..., None]
    c = -(do * o).sum(-1) / den
    dqp = torch.einsum("bhnd,bhdj->bhnj", g, S)
    if slip != "no_cz_term":
        dqp = dqp + c[..., None] * z[..., None, :]
    dq = dqp if slip == "no_q_mask" else dqp * (q > 0)
    N = q.shape[-2]
    keep = N // BWD_CHUNK * BWD_CHUNK if (slip == "drop_partial_chunk" and N % BWD_CHUNK) else N
    dS = torch.einsum("bhnd,bhnj->bhdj", g[..., :keep, :], qq[..., :keep, :])
    dz = torch.einsum("bhn,bhnj->bhj", c[..., :keep], qq[..., :keep, :])
    if slip == "dstate_bf16":
        dS, dz = BR.bf16(dS), BR.bf16(dz)
    dk = (torch.einsum("bhnd,bhdj->bhnj", v, dS) + dz[..., None, :]) * (k > 0)
    dv = torch.einsum("bhdj,bhnj->bhnd", dS, kk)
    # the magnitudes of what cancels in each gradient (BR.err's `mag`): dq' = g S + c z is orthogonal to q' (the output does not change when q' is
    # scaled), and with one token the output is v whatever q and k are, so dq and dk are exact zeros reached as differences; no fp32 evaluation gets
    # closer to them than a few ulps of the terms
    dSa = torch.einsum("bhnd,bhnj->bhdj", g.abs(), qq)
    dza = torch.einsum("bhn,bhnj->bhj", c.abs(), qq)
    mag = dict(dq=(torch.einsum("bhnd,bhdj->bhnj", g.abs(), S.abs()) + c.abs()[..., None] * z[..., None, :]) * (q > 0),
               dk=(torch.einsum("bhnd,bhdj->bhnj", v.abs(), dSa) + dza[..., None, :]) * (k > 0), dv=torch.einsum("bhdj,bhnj->bhnd", dSa, kk))
    return dict(dq=rnd(dq), dk=rnd(dk), dv=rnd(dv), mag=mag)


# ---------------------------------------------------------------- GLU depthwise convolution --------------------------------------------------------
def _dsilu(t):
    s = torch.sigmoid(t)
    return s * (1 + t * (1 - s))


def _pad1(t, clamp=False):
    """[B, H, W, K] -> [B, H + 2, W + 2, K]: zeros round the image (clamp: replicated borders)"""
    return F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if clamp else "constant").permute(0, 2, 3, 1)


def glu_dwconv_bwd(x, w, b, do, variant=False, slip=None):
    assert slip is None or slip in GLU_SLIPS
    rnd = BR.bf16 if (variant or slip) else (lambda t: t)
    x, w64, do = x.to(F64), w.to(F64), do.to(F64)
    B, H, W, C2 = x.shape
    C = C2 // 2
    a = rnd(R._silu(x))
    y = rnd(R._dwconv(a, w, b))
    yv, yg = y[..., :C], y[..., C:]
    s = rnd(R._silu(yg))
    dyv, dyg = rnd(do * s), rnd(do * yv * _dsilu(yg))
    dy = torch.cat([dyg, dyv] if slip == "halves_swapped" else [dyv, dyg], -1)
    clamp = slip == "clamp_padding"
    dyp, ap = _pad1(dy, clamp), _pad1(a, clamp)
    da = torch.zeros_like(x)
    dw = torch.zeros_like(w64)
    for ky in range(3):
        for kx in range(3):
            # y[p] read a[p + t - 1] through tap t, so a[q] is read by y[q - (t - 1)]: the flipped window of dy
            sy, sx = (ky, kx) if slip == "unflipped_taps" else (2 - ky, 2 - kx)
            da = da + dyp[:, sy:sy + H, sx:sx + W, :] * w64[:, 0, ky, kx]
            dw[:, 0, ky, kx] = (dy * ap[:, ky:ky + H, kx:kx + W, :]).sum((0, 1, 2))
    db = (dy[:1] if slip == "dbias_one_sample" else dy).sum((0, 1, 2))
    return dict(dx=rnd(da * _dsilu(x)), dw=dw, db=db, mag={})
