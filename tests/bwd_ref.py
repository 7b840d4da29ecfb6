"""CPU float64 references of the training backward kernels (csrc/backward.hip, the attn_bwd_* kernels of csrc/attention.hip, autograd.Linear).

Every function takes the operands exactly as the kernel sees them (bf16 or fp32 values, here widened to float64) and returns the exact result of
the operation. Where a GPU bound is relative to "the kernel's own rounding points", the same function also returns a second variant (`*_r` keys;
bf16() of the exact result where the output is the only rounding point) that rounds to bf16 where the kernel rounds - attention: P and dS as matrix operands; gate: bf16(x + c); every output - so a
test can bound the kernel by 1.5 x that variant's own error against the exact value. Some outputs are a difference of two fp32 quantities that can
cancel (dS = P (dP - delta), d logits = g (dg - sum dg g)); for those a cancellation-free magnitude (`*_m`) is returned as well, and `err` allows
ABS_U of it on top of the relative error. tests/test_bwd_ref_cpu.py checks every function here against torch.autograd in float64."""
import math

import torch

F64 = torch.float64
LOG2E = 1.0 / math.log(2.0)
ABS_U = 2.0 ** -20          # 16 fp32 ulps of a cancellation-free magnitude: the absolute allowance of an fp32 difference that cancels


def bf16(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest even), back to float64"""
    return t.to(torch.bfloat16).to(F64)


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp of each value (8 significant bits); 0 for 0"""
    e = torch.floor(torch.log2(t.abs().clamp_min(1e-300)))
    return torch.where(t == 0, torch.zeros_like(t), torch.exp2(e - 7))


def err(got: torch.Tensor, truth: torch.Tensor, mag=None, rows_from=None):
    """-> (total, worst row, worst row of the tail): max(0, |got - truth| - ABS_U |mag|) / |truth| in the L2 norm over the whole tensor and
    over each row (last dimension); 0 / 0 counts as 0, x / 0 as inf. rows_from: the tail is the rows with index >= rows_from along dim -2
    (None: no tail)."""
    g, t = got.to(F64).cpu(), truth.to(F64)
    d = g - t

    def one(dn, tn, mn):
        ex = (dn - ABS_U * mn).clamp_min(0.0)
        return torch.where(ex == 0, torch.zeros_like(ex), ex / tn)

    m = mag.to(F64) if mag is not None else torch.zeros_like(t)
    total = float(one(d.norm(), t.norm(), m.norm()))
    rows = one(d.norm(dim=-1), t.norm(dim=-1), m.norm(dim=-1)) if t.dim() > 0 else torch.zeros(1, dtype=F64)
    worst = float(rows.max()) if rows.numel() else 0.0
    tail = 0.0
    if rows_from is not None and t.dim() >= 2 and rows_from < t.shape[-2]:
        tail = float(rows[..., rows_from:].max())
    return total, worst, tail


# ----------------------------------------------------------------------------------------------------------------------------------
# attention: S = q k^T, c = scale log2(e), lse2 = log2 sum_k 2^(c S), P = 2^(c S - lse2), O = P v;  backward with dO:
# dP = dO v^T, delta = rowsum(dO . O) (O: the output the backward reads), dS = P (dP - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T dO
# ----------------------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, do, scale, o=None, lsum_bf16=False, backward=True):
    """q, do [..., Lq, dh], k, v [..., Lkv, dh] (float64 holding the kernel's operands); o: the forward output the backward reads (the kernel's
    bf16 O), None = the exact O. Returns a dict of every intermediate plus the rounding-point variants:
      O_r   = bf16(bf16(p) v / l), p = 2^(c S - rowmax), l = sum p (lsum_bf16: sum bf16(p), the head-width-64 forward's denominator)
      dq_r, dk_r, dv_r: P and dS rounded to bf16 as operands, the products exact, the results rounded to bf16
      dq_m, dk_m: the same products with |dO| |v|^T + rowsum(|dO| |O|) in place of dP - delta (cancellation-free magnitude: the two fp32 dot
                  products and their difference are where a kernel's error is absolute, not relative)."""
    q, k, v, do = (t.to(F64) for t in (q, k, v, do))
    c = scale * LOG2E
    S = q @ k.transpose(-1, -2)
    cs = c * S
    mx = cs.amax(-1, keepdim=True)
    p = torch.exp2(cs - mx)
    lse2 = (mx + torch.log2(p.sum(-1, keepdim=True))).squeeze(-1)
    P = torch.exp2(cs - lse2[..., None])
    O = P @ v
    pb = bf16(p)
    O_r = bf16((pb @ v) / (pb.sum(-1, keepdim=True) if lsum_bf16 else p.sum(-1, keepdim=True)))
    out = dict(S=S, lse2=lse2, P=P, O=O, O_r=O_r)
    if not backward:
        return out
    ob = O if o is None else o.to(F64)
    dP = do @ v.transpose(-1, -2)
    delta = (do * ob).sum(-1)
    dS = P * (dP - delta[..., None])
    dSm = P * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * ob.abs()).sum(-1)[..., None])     # sums of |terms|: nothing cancels
    Pb, dSb = bf16(P), bf16(dS)
    out.update(dP=dP, delta=delta, dS=dS,
               dq=scale * dS @ k, dk=scale * dS.transpose(-1, -2) @ q, dv=P.transpose(-1, -2) @ do,
               dq_r=bf16(scale * dSb @ k), dk_r=bf16(scale * dSb.transpose(-1, -2) @ q), dv_r=bf16(Pb.transpose(-1, -2) @ do),
               dq_m=scale * dSm @ k, dk_m=scale * dSm.transpose(-1, -2) @ q)
    return out


def row_lse(S, scale, valid_cols=None):
    """natural-log log-sum-exp of scale S over the first valid_cols columns"""
    S = S.to(F64)
    n = S.shape[-1] if valid_cols is None else valid_cols
    return torch.logsumexp(scale * S[..., :n], -1)


def attn_prob(S, lse, scale, valid_cols=None):
    """exp(scale S - lse) in the first valid_cols columns, 0 beyond"""
    S = S.to(F64)
    n = S.shape[-1] if valid_cols is None else valid_cols
    P = torch.exp(scale * S - lse.to(F64)[..., None])
    P[..., n:] = 0.0
    return P


def attn_dscore(P, dP, delta, scale):
    return scale * P.to(F64) * (dP.to(F64) - delta.to(F64)[..., None])


def rowdot(a, b, groups):
    """a, b [rows, groups * cols] -> [groups, rows]"""
    rows = a.shape[0]
    return (a.to(F64) * b.to(F64)).view(rows, groups, -1).sum(-1).transpose(0, 1)


# ----------------------------------------------------------------------------------------------------------------------------------
# elementwise / row-wise backward kernels
# ----------------------------------------------------------------------------------------------------------------------------------
_K0 = math.sqrt(2.0 / math.pi)


def gelu_tanh_bwd(x, dy):
    """dy * d/dx [0.5 x (1 + tanh(u))], u = sqrt(2/pi) (x + 0.044715 x^3). Returns (dx, mag): mag = |dy| (s + |x s (1 - s) u'|) with
    s = (1 + tanh u) / 2 - the two terms the kernel adds in fp32 (gelu_grad_f), for the allowance of their cancellation near x = -0.75."""
    x, dy = x.to(F64), dy.to(F64)
    u = _K0 * (x + 0.044715 * x ** 3)
    s = torch.sigmoid(2.0 * u)                                # = (1 + tanh u) / 2 without its cancellation below u = -19
    du = 2.0 * _K0 * (1.0 + 3.0 * 0.044715 * x * x)         # d(2u)/dx: s = sigmoid(2u)
    g = s + x * s * (1.0 - s) * du
    return dy * g, dy.abs() * (s + (x * s * (1.0 - s) * du).abs())


def moe_gate_bwd(gates, dgates, x, c, wg):
    """gates = softmax((x + c) wg^T) [S, E] (as given), d gates [S, E] -> dict(dx, dw exact; dx_r, dw_r with bf16(x + c) and bf16 outputs;
    dx_m, dw_m cancellation-free magnitudes). dx is d(x + c): the same tensor is d x and d c."""
    g, dg = gates.to(F64), dgates.to(F64)
    xc = x.to(F64) + c.to(F64)
    w = wg.to(F64)
    dot = (dg * g).sum(-1, keepdim=True)
    dl = g * (dg - dot)
    dlm = g * (dg.abs() + (dg.abs() * g).sum(-1, keepdim=True))
    return dict(dl=dl, dx=dl @ w, dw=dl.transpose(0, 1) @ xc, dx_r=bf16(dl @ w), dw_r=bf16(dl.transpose(0, 1) @ bf16(xc)),
                dx_m=dlm @ w, dw_m=dlm.transpose(0, 1) @ xc)


def adaln_modulate_bwd(x, dy, scale, rows_per_sample, eps=1e-6):
    """y = LayerNorm(x) (1 + scale[row // rows_per_sample]) + shift[...] -> (dx, d shift, d scale); x, dy [rows, D], scale [samples, D]"""
    x, dy, sc = x.to(F64), dy.to(F64), scale.to(F64)
    rows, D = x.shape
    mu = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    s1 = (1.0 + sc).repeat_interleave(rows_per_sample, 0)
    gg = dy * s1
    dx = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    dshift = dy.view(-1, rows_per_sample, D).sum(1)
    dscale = (dy * xh).view(-1, rows_per_sample, D).sum(1)
    return dx, dshift, dscale


def qk_rmsnorm_rope_bwd(x, dy, w, cos, sin, rows_per_batch, pos_offset, heads, dh, eps=1e-6):
    """Forward per (row, head) vector: u = x rsqrt(mean(x^2) + eps) w (w None: u = x), y = rope(u) with the pair rotation
    y[2i] = u[2i] cos[p][2i] - u[2i+1] sin[p][2i], y[2i+1] = u[2i+1] cos[p][2i+1] + u[2i] sin[p][2i+1] at p = pos_offset + row % rows_per_batch
    (cos None: y = u). x, dy [rows, heads * dh] -> (dx, d w or None)."""
    x, dy = x.to(F64), dy.to(F64)
    rows = x.shape[0]
    xv, gv = x.reshape(rows, heads, dh), dy.reshape(rows, heads, dh)
    if cos is not None:
        pos = pos_offset + torch.arange(rows) % rows_per_batch
        cc, sn = cos.to(F64)[pos][:, None, :], sin.to(F64)[pos][:, None, :]
        g0, g1 = gv[..., 0::2], gv[..., 1::2]
        dun = torch.empty_like(gv)
        dun[..., 0::2] = g0 * cc[..., 0::2] + g1 * sn[..., 1::2]
        dun[..., 1::2] = g1 * cc[..., 1::2] - g0 * sn[..., 0::2]
    else:
        dun = gv
    if w is None:
        return dun.reshape(rows, heads * dh), None
    wv = w.to(F64)
    rs = torch.rsqrt((xv * xv).mean(-1, keepdim=True) + eps)
    u = xv * rs
    du = dun * wv
    dx = rs * (du - u * (du * u).mean(-1, keepdim=True))
    dw = (dun * u).sum((0, 1))
    return dx.reshape(rows, heads * dh), dw


def linear_bwd(x, w, dy):
    """y = x w^T + b -> (dx = dy w, dw = dy^T x, db = colsum dy)"""
    x, w, dy = x.to(F64), w.to(F64), dy.to(F64)
    return dy @ w, dy.transpose(0, 1) @ x, dy.sum(0)


def colsum(a, b=None, rows_per_group=None, alpha=1.0):
    """[rows, cols] -> [rows / rows_per_group, cols]: alpha * per-group column sums of a (. b)"""
    t = a.to(F64) if b is None else a.to(F64) * b.to(F64)
    g = t.shape[0] if rows_per_group is None else rows_per_group
    return alpha * t.view(-1, g, t.shape[1]).sum(1)
