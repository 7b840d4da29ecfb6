"""CPU float64 references of the training backward kernels (csrc/backward.hip, the attn_bwd_* kernels of csrc/attention.hip, autograd.Projection / LinearResScale / LinearCat2).

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
def attention(q, k, v, do, scale, o=None, lsum_bf16=False, backward=True, fwd_tile=64, fwd_lazy=8.0):
    """q, do [..., Lq, dh], k, v [..., Lkv, dh] (float64 holding the kernel's operands); o: the forward output the backward reads (the kernel's
    bf16 O), None = the exact O. Returns a dict of every intermediate plus the rounding-point variants:
      O_r   = bf16(bf16(p) v / l), p = 2^(c S - rowmax), l = sum p (lsum_bf16: sum bf16(p), the head-width-64 forward's denominator)
      O_l   = the same roundings along flash_attn_kernel's own trajectory (forward_lazy below): its reference point is not the row maximum
              (O_l and everything derived from it - moves, last_move, lse2_l, *_rl - are left out with fwd_tile=None)
      moves, last_move [..., Lq]: how often a row's reference point moved, and the last key tile in which it did
      dq_r, dk_r, dv_r: P and dS rounded to bf16 as operands, the products exact, the results rounded to bf16
      dq_rl, dk_rl, dv_rl: the same with P = 2^(c S - lse2_l), lse2_l the LSE the forward kernel itself leaves (forward_lazy)
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
    if fwd_tile is not None:
        O_l, moves, last_move, lse2_l = forward_lazy(cs, v, lsum_bf16, fwd_tile, fwd_lazy)
        out.update(O_l=O_l, moves=moves, last_move=last_move, lse2_l=lse2_l)
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
    if fwd_tile is None:
        return out
    # the same variants with P recomputed from the forward's own statistics lse2_l, as attn_bwd_dkv_kernel / attn_bwd_kernel do when the caller
    # passes the forward's LSE (`lse_in`): at head width 64 that LSE is the log of a sum of bf16-rounded probabilities
    Pl = torch.exp2(cs - lse2_l[..., None])
    Plb, dSlb = bf16(Pl), bf16(Pl * (dP - delta[..., None]))
    out.update(dq_rl=bf16(scale * dSlb @ k), dk_rl=bf16(scale * dSlb.transpose(-1, -2) @ q), dv_rl=bf16(Plb.transpose(-1, -2) @ do))
    return out


def forward_lazy(cs, v, lsum_bf16=False, tile=64, lazy=8.0):
    """The forward output with flash_attn_kernel's rounding points along the kernel's trajectory (csrc/attention.hip, do_SM); cs = c S
    [..., Lq, Lkv] and v [..., Lkv, dh] in float64. Per row and `tile` keys: the reference point m becomes the tile's maximum in the first tile,
    and later only where that maximum exceeds m by more than `lazy` (`up = (tmax - m_run) * c > 8.0f`; one maximum per row and tile: the kernel
    joins its two lane halves, ug_max_halves); p = 2^(cs - m) (`exp2f(fmaf(s, c, -mc))`); bf16(p) multiplies v (`pack2bf`, the P.V operand);
    the accumulator and l are rescaled by 2^(m_old - m_new) (`alpha`); l adds p, or bf16(p) with lsum_bf16 (LSUM: the head-width-64 row sums
    come from the packed fragments); the output is bf16(acc / l). Everything else is float64.
    -> (O_l, moves, last_move, lse2_l): moves [..., Lq] counts how often a row's m moved (the first tile included), last_move the last tile where
    it did, lse2_l = m + log2(l) the statistics the kernel leaves for the backward (`lse_out[...] = logf(l_tot) + m_run * c`: with lsum_bf16 the
    log of the sum of ROUNDED probabilities, off by up to 2^-9 / ln 2 on a peaked row)."""
    cs, v = cs.to(F64), v.to(F64)
    lead, Lkv = cs.shape[:-1], cs.shape[-1]
    m = torch.full(lead, -math.inf, dtype=F64)
    l = torch.zeros(lead, dtype=F64)
    acc = torch.zeros(*lead, v.shape[-1], dtype=F64)
    moves = torch.zeros(lead, dtype=torch.long)
    last_move = torch.full(lead, -1, dtype=torch.long)
    for t, k0 in enumerate(range(0, Lkv, tile)):
        ct = cs[..., k0:k0 + tile]
        tmax = ct.amax(-1)
        up = (tmax - m) > lazy if t else torch.ones(lead, dtype=torch.bool)
        m_new = torch.where(up, tmax, m)
        alpha = torch.where(up, torch.exp2(m - m_new), torch.ones_like(m))
        p = torch.exp2(ct - m_new[..., None])
        pb = bf16(p)
        acc = acc * alpha[..., None] + pb @ v[..., k0:k0 + tile, :]
        l = l * alpha + (pb if lsum_bf16 else p).sum(-1)
        m = m_new
        moves += up
        last_move = torch.where(up, torch.full_like(last_move, t), last_move)
    return bf16(acc / l[..., None]), moves, last_move, m + torch.log2(l)


# ----------------------------------------------------------------------------------------------------------------------------------
# attention regimes: operands whose softmax rows are peaked, so that the forward's lazy reference point moves in later tiles and the
# backward kernels see probabilities near 1 (tests/test_attn_regimes_cpu.py checks what each regime promises)
# ----------------------------------------------------------------------------------------------------------------------------------
REGIMES = ("gaussian", "rising", "falling", "spike_tail", "spike_mid", "near_threshold", "one_key")
BACKGROUND = 0.3            # standard deviation of c S over the background keys, in log2 units
RAMP = 5.0                  # rising / falling: what a chosen row's tile maximum gains / loses per 64-key tile
SPIKE = 14.0                # spike_tail / spike_mid: the spike key's c S in a chosen row, 12 above the rest (the background's maximum stays below 2)
NEAR = (7.5, 8.5)           # near_threshold: the spike's gap over the row's reference point, below and above the kernel's 8
NEAR_CLEAR = 0.05           # ... and how far from 8 every realised gap has to stay
ONE_KEY = 20.0              # one_key: 2^-20 x ~1000 background keys leaves the dominant key more than 0.99
SPIKE_POS = (1, 38, 29, 58)   # spike keys inside their 64-key tile: both 32-key blocks, key % 8 in 0..3 (1, 58) and in 4..7 (38, 29)


def regime_fits(regime, Lq, Lkv):
    """whether the regime can be built at these lengths"""
    full, part = Lkv // 64, Lkv % 64
    if regime in ("rising", "falling"):
        return full >= 4
    if regime == "spike_tail":
        return part != 0 and full >= 1
    if regime == "spike_mid":
        return full >= (2 if part else 3) and Lq > 32
    if regime == "near_threshold":
        return full >= 2
    return True


def attention_regime(g, regime, dh, B, H, Lq, Lkv, scale):
    """-> dict: q, do [B, H, Lq, dh] and k, v [B, H, Lkv, dh] in bf16; `rows`: the query rows the regime acts on; `keys`: the key rows it
    spikes (None: all or none); `row_key` [len(rows)]: each chosen row's spike key; `row_gap`: its target. Amplitudes are in log2 units of
    c S, c = scale log2(e): background q is drawn with standard deviation BACKGROUND / (c sqrt(dh)) against unit k, and both lose their
    components along four orthonormal directions u_j. A chosen row of class j = (row // 4) % 4 gains w u_j / c and a key b u_j, so exactly that
    pair's c S gains w b and every other score keeps its background value (up to the bf16 rounding of q and k).
      gaussian        N(0, 1) operands, q times dh^-0.5 / scale: today's sweeps' scores at every scale
      rising/falling  even rows; every key gains RAMP x (its tile's index, centred) along all four directions: the ramp is centred so that
                      |scale S| stays below 40 at 17 tiles
      spike_tail      rows 0, 4, 8, ...; one key per class in the partial last tile at SPIKE
      spike_mid       the same in a full tile that is neither first nor last, in the even 32-row groups only: the odd groups have no spiking
                      row (their waves skip the rescale), the even ones are mixed
      near_threshold  rows 0, 4, 8, ...; spikes in the last full tile but one (the last full one if no other is left) whose gap over the
                      row's first-tile maximum is NEAR[0] for the even classes, NEAR[1] for the odd ones: fitted on the float64 scores of
                      the rounded operands, rows within NEAR_CLEAR of 8 are drawn again
      one_key         rows 0, 4, 8, ...; the dominant key at ONE_KEY, in the first tile for classes 0 and 1, in the last tile for classes 2
                      and 3 (the last but one where the tail is too short to hold the class's position)"""
    assert regime in REGIMES and regime_fits(regime, Lq, Lkv), (regime, Lq, Lkv)
    c = scale * LOG2E
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    if regime == "gaussian":
        q, k, v, do = rn(B, H, Lq, dh) * (dh ** -0.5 / scale), rn(B, H, Lkv, dh), rn(B, H, Lkv, dh), rn(B, H, Lq, dh)
        none = torch.arange(0)
        return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), do=do.to(torch.bfloat16), rows=none, keys=None,
                    row_key=none, row_gap=none.to(F64))
    U = torch.linalg.qr(rn(dh, 4))[0]                                  # [dh, 4] orthonormal columns
    off = lambda t: t - (t @ U) @ U.T
    sq = BACKGROUND / (c * math.sqrt(dh))
    q, k, v, do = off(rn(B, H, Lq, dh) * sq), off(rn(B, H, Lkv, dh)), rn(B, H, Lkv, dh), rn(B, H, Lq, dh)
    ntiles, part = (Lkv + 63) // 64, Lkv % 64
    if regime in ("rising", "falling"):
        rows = torch.arange(0, Lq, 2)
        tile = (torch.arange(Lkv) // 64).to(F64) - (ntiles - 1) / 2
        k = k + (RAMP * (tile if regime == "rising" else -tile))[:, None] * U.sum(1) / 2        # |sum of the four u_j| = 2
        q[:, :, rows] += U.sum(1) / (2 * c)
        return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), do=do.to(torch.bfloat16), rows=rows, keys=None,
                    row_key=torch.arange(0), row_gap=torch.arange(0).to(F64))
    rows = torch.arange(0, Lq, 4)
    if regime == "spike_mid":
        rows = rows[(rows // 32) % 2 == 0]
    cls = (rows // 4) % 4
    last = ntiles - 1
    width = lambda t: min(64, Lkv - 64 * t)
    at = lambda t, j: 64 * t + SPIKE_POS[j] % width(t)
    if regime == "spike_tail":
        key_of, gap_of = [at(last, j) for j in range(4)], [SPIKE] * 4
    elif regime == "spike_mid":
        mid = min(max(1, (last + 1) // 2), last - 1)
        key_of, gap_of = [at(mid, j) for j in range(4)], [SPIKE] * 4
    elif regime == "near_threshold":
        full_last = last - 1 if part else last
        late = full_last - 1 if full_last >= 2 else full_last
        key_of, gap_of = [at(late, j) for j in range(4)], [NEAR[j % 2] for j in range(4)]
    else:
        later = [last if width(last) > SPIKE_POS[j] or last <= 1 else last - 1 for j in range(4)]      # at 65 keys: the one key of the tail
        key_of, gap_of = [at(0, 0), at(0, 1), at(later[2], 2), at(later[3], 3)], [ONE_KEY] * 4
    keys = torch.tensor(sorted(set(key_of)))
    row_key = torch.tensor(key_of)[cls]
    row_gap = torch.tensor(gap_of, dtype=F64)[cls]
    amp = 4.0                                                           # key amplitude b; the row's weight is gap / b
    for j in range(4):
        k[:, :, key_of[j]] += amp * U[:, j]
    k = bf16(k)
    if regime != "near_threshold":
        q[:, :, rows] += (row_gap / (amp * c))[:, None] * U[:, cls].T
        return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), do=do.to(torch.bfloat16), rows=rows, keys=keys,
                    row_key=row_key, row_gap=row_gap)
    # near_threshold: the gap is what the kernel compares - the spike's c S minus the maximum of the row's first tile - on the ROUNDED operands.
    # Fit every chosen row's weight to it (the gap is linear in the weight up to the rounding of q), then draw again what still sits near 8.
    ks = k[:, :, row_key]                                               # [B, H, rows, dh] each chosen row's spike key
    dirs = U[:, cls].T
    w = (row_gap / amp).expand(B, H, -1).clone()
    base = q[:, :, rows].clone()
    for attempt in range(8):
        for _ in range(4):
            qr = bf16(base + (w / c)[..., None] * dirs)
            gap = c * ((qr * ks).sum(-1) - (qr @ k[:, :, :64].transpose(-1, -2)).amax(-1))
            w = w + (row_gap - gap) / amp
        qr = bf16(base + (w / c)[..., None] * dirs)
        gap = c * ((qr * ks).sum(-1) - (qr @ k[:, :, :64].transpose(-1, -2)).amax(-1))
        bad = ((gap - 8.0).abs() <= NEAR_CLEAR) | ((gap - row_gap).abs() > 0.25)
        if not bool(bad.any()):
            break
        base = torch.where(bad[..., None], off(rn(B, H, len(rows), dh) * sq), base)
    assert not bool(bad.any()), "near_threshold: rows left within NEAR_CLEAR of the threshold"
    q[:, :, rows] = qr
    return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), do=do.to(torch.bfloat16), rows=rows, keys=keys,
                row_key=row_key, row_gap=row_gap)


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
