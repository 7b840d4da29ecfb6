"""tests/bwd_ref.py against torch.autograd in float64 on small random shapes (no GPU): the fp64 references the backward sweep
(tests/test_fuzz_backward_gpu.py) measures the kernels against are themselves right, to 1e-12."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bwd_ref as BR

F64 = torch.float64
TOL = 1e-12


def rel(a, b):
    """relative L2 error; against a truth below norm 1e-2 (one key: dS = 0 up to fp64 rounding) the absolute error over 1e-2"""
    a, b = a.detach().to(F64), b.detach().to(F64)
    return float((a - b).norm() / b.norm().clamp_min(1e-2))


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("Lq,Lkv,dh", [(1, 1, 8), (5, 17, 16), (33, 7, 8), (64, 65, 32)])
def test_attention_reference(Lq, Lkv, dh):
    g = _g(Lq * 100 + Lkv)
    B, H = 2, 3
    q, k, v = (torch.randn(B, H, L, dh, generator=g, dtype=F64).requires_grad_(True) for L in (Lq, Lkv, Lkv))
    do = torch.randn(B, H, Lq, dh, generator=g, dtype=F64)
    scale = dh ** -0.5
    Z = (q @ k.transpose(-1, -2)) * scale
    Z.retain_grad()
    P = torch.softmax(Z, -1)
    P.retain_grad()
    O = P @ v
    O.backward(do)
    r = BR.attention(q.detach(), k.detach(), v.detach(), do, scale)
    assert rel(r["S"] * scale, Z) < TOL and rel(r["P"], P) < TOL and rel(r["O"], O) < TOL
    assert rel(r["lse2"], torch.logsumexp(Z, -1) / math.log(2.0)) < TOL
    assert rel(r["dP"], P.grad) < TOL and rel(r["dS"], Z.grad) < TOL
    assert rel(r["delta"], (do * O).sum(-1)) < TOL
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        assert rel(r[name], t.grad) < TOL, name
    # F.scaled_dot_product_attention agrees as well
    assert rel(r["O"], F.scaled_dot_product_attention(q.detach(), k.detach(), v.detach())) < TOL
    # delta from a given O (the backward reads the forward's output): with the exact O it is the same gradient
    r2 = BR.attention(q.detach(), k.detach(), v.detach(), do, scale, o=O.detach())
    assert rel(r2["dq"], q.grad) < TOL
    # the rounding-point variants sit within bf16 reach of the exact values and hold bf16 values
    for name in ("O_r", "dq_r", "dk_r", "dv_r"):
        exact = r[name[:-2]]
        assert torch.equal(r[name], BR.bf16(r[name])), name
        if exact.norm() > 0:
            assert rel(r[name], exact) < 3e-2, (name, rel(r[name], exact))
    # the cancellation-free magnitudes bound the gradients elementwise in their own row sums
    dSm = r["P"] * (do.abs() @ v.detach().abs().transpose(-1, -2) + (do.abs() * O.detach().abs()).sum(-1)[..., None])
    assert float((r["dS"].abs() - dSm).max()) <= 1e-15 and rel(r["dq_m"], dq_m := scale * dSm @ k.detach()) < TOL and dq_m.norm() > 0


def test_attention_single_key_gradients_vanish():
    """One key: P = 1, O = v, dS = 0 exactly - dq = dk = 0; the magnitudes are not zero (what `err` allows against)."""
    g = _g(7)
    q, k, v, do = (torch.randn(1, 2, L, 16, generator=g, dtype=F64) for L in (5, 1, 1, 5))
    r = BR.attention(q, k, v, do, 0.25)
    assert float(r["dq"].abs().max()) < 1e-15 and float(r["dk"].abs().max()) < 1e-15 and float(r["dq_m"].abs().max()) > 1e-3
    total, worst, _ = BR.err(r["dq"] + 1e-9 * r["dq_m"], r["dq"], r["dq_m"])
    assert total == 0.0 and worst == 0.0                                        # within ABS_U of the magnitude
    assert BR.err(r["dq"] + 1e-3 * r["dq_m"], r["dq"], r["dq_m"])[0] > 1e6       # beyond it, against a (rounding-level) zero truth


def test_err_metric():
    t = torch.tensor([[3.0, 4.0], [0.0, 1.0], [6.0, 8.0]], dtype=F64)
    got = t.clone()
    got[2, 0] += 1.0
    total, worst, tail = BR.err(got, t, rows_from=2)
    assert abs(total - 1.0 / float(t.norm())) < TOL and abs(worst - 0.1) < TOL and abs(tail - 0.1) < TOL
    assert BR.err(t, t, rows_from=1) == (0.0, 0.0, 0.0)
    u = BR.bf16_ulp(torch.tensor([1.0, 1.5, -3.0, 0.0], dtype=F64))
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0]


def test_softmax_row_kernels_reference():
    g = _g(11)
    S = torch.randn(6, 40, generator=g, dtype=F64) * 3
    scale, n = 0.3, 29
    lse = BR.row_lse(S, scale, n)
    assert rel(lse, torch.logsumexp(scale * S[:, :n], -1)) < TOL
    P = BR.attn_prob(S, lse, scale, n)
    assert rel(P[:, :n], torch.softmax(scale * S[:, :n], -1)) < TOL and float(P[:, n:].abs().max()) == 0.0
    # dscore = d loss / d S through the softmax: scale P (dP - rowsum(dP P))
    St = S[:, :n].clone().requires_grad_(True)
    Pt = torch.softmax(scale * St, -1)
    dP = torch.randn(6, n, generator=g, dtype=F64)
    Pt.backward(dP)
    delta = (dP * Pt.detach()).sum(-1)
    assert rel(BR.attn_dscore(Pt.detach(), dP, delta, scale), St.grad) < TOL
    a, b = torch.randn(5, 3 * 7, generator=g, dtype=F64), torch.randn(5, 3 * 7, generator=g, dtype=F64)
    want = torch.stack([(a[:, i * 7:(i + 1) * 7] * b[:, i * 7:(i + 1) * 7]).sum(-1) for i in range(3)])
    assert rel(BR.rowdot(a, b, 3), want) < TOL


def test_gelu_tanh_bwd_reference():
    x = torch.cat([torch.linspace(-10, 10, 2001, dtype=F64), torch.zeros(3, dtype=F64)]).requires_grad_(True)
    dy = torch.randn(x.shape, generator=_g(12), dtype=F64)
    F.gelu(x, approximate="tanh").backward(dy)
    dx, mag = BR.gelu_tanh_bwd(x.detach(), dy)
    assert float((dx - x.grad).abs().max()) < TOL and bool((mag >= dx.abs() - 1e-15).all())
    # far left (x < -5) torch's 1 + tanh(u) cancels to 0 in float64 too: a central difference of x sigmoid(2u) there, to 1e-6 relative
    xl = torch.linspace(-10, -5, 51, dtype=F64)
    gl = lambda t: t * torch.sigmoid(2 * math.sqrt(2 / math.pi) * (t + 0.044715 * t ** 3))
    h = 1e-5
    fd = (gl(xl + h) - gl(xl - h)) / (2 * h)
    got = BR.gelu_tanh_bwd(xl, torch.ones_like(xl))[0]
    assert bool((got < 0).all()) and float(((got - fd) / fd).abs().max()) < 1e-6


@pytest.mark.parametrize("S,E,D", [(5, 1, 8), (9, 3, 16), (33, 16, 24)])
def test_moe_gate_bwd_reference(S, E, D):
    g = _g(S * E + D)
    x, c = torch.randn(S, D, generator=g, dtype=F64).requires_grad_(True), torch.randn(S, D, generator=g, dtype=F64).requires_grad_(True)
    wg = (torch.randn(E, D, generator=g, dtype=F64) * D ** -0.5).requires_grad_(True)
    gates = torch.softmax(F.linear(x + c, wg), -1)
    dg = torch.randn(S, E, generator=g, dtype=F64)
    gates.backward(dg)
    r = BR.moe_gate_bwd(gates.detach(), dg, x.detach(), c.detach(), wg.detach())
    if E == 1:                                                      # softmax over one expert is constant: every gradient is exactly zero
        assert float(r["dx"].abs().max()) == 0.0 and float(x.grad.abs().max()) == 0.0
    else:
        assert rel(r["dx"], x.grad) < TOL and rel(r["dx"], c.grad) < TOL and rel(r["dw"], wg.grad) < TOL


@pytest.mark.parametrize("rows,rps,D", [(6, 1, 8), (14, 7, 24), (10, 10, 40)])
def test_adaln_modulate_bwd_reference(rows, rps, D):
    g = _g(rows + D)
    x = torch.randn(rows, D, generator=g, dtype=F64).requires_grad_(True)
    sc = (0.3 * torch.randn(rows // rps, D, generator=g, dtype=F64)).requires_grad_(True)
    sh = torch.zeros(rows // rps, D, dtype=F64, requires_grad=True)
    dy = torch.randn(rows, D, generator=g, dtype=F64)
    y = F.layer_norm(x, (D,), eps=1e-6).view(-1, rps, D) * (1 + sc[:, None]) + sh[:, None]
    y.reshape(rows, D).backward(dy)
    dx, dsh, dsc = BR.adaln_modulate_bwd(x.detach(), dy, sc.detach(), rps)
    assert rel(dx, x.grad) < TOL and rel(dsh, sh.grad) < TOL and rel(dsc, sc.grad) < TOL


@pytest.mark.parametrize("with_w,with_rope", [(True, True), (True, False), (False, True)])
def test_qk_rmsnorm_rope_bwd_reference(with_w, with_rope):
    g = _g(13)
    heads, dh, rpb, off, batches = 3, 16, 5, 4, 2
    rows = batches * rpb
    x = torch.randn(rows, heads * dh, generator=g, dtype=F64).requires_grad_(True)
    w = (1 + 0.2 * torch.randn(dh, generator=g, dtype=F64)).requires_grad_(True) if with_w else None
    ang = torch.rand(off + rpb, dh // 2, generator=g, dtype=F64) * 6.28
    cos, sin = (ang.cos().repeat_interleave(2, 1), ang.sin().repeat_interleave(2, 1)) if with_rope else (None, None)
    dy = torch.randn(rows, heads * dh, generator=g, dtype=F64)
    xv = x.view(rows, heads, dh)
    u = xv * torch.rsqrt(xv.pow(2).mean(-1, keepdim=True) + 1e-6) * w if with_w else xv
    if with_rope:
        pos = off + torch.arange(rows) % rpb
        rot = torch.stack([-u[..., 1::2], u[..., 0::2]], -1).flatten(-2)
        y = u * cos[pos][:, None] + rot * sin[pos][:, None]
    else:
        y = u
    y.reshape(rows, heads * dh).backward(dy)
    dx, dw = BR.qk_rmsnorm_rope_bwd(x.detach(), dy, None if w is None else w.detach(), cos, sin, rpb, off, heads, dh)
    assert rel(dx, x.grad) < TOL
    assert (dw is None) == (w is None) and (dw is None or rel(dw, w.grad) < TOL)


def test_linear_and_colsum_reference():
    g = _g(14)
    x, w, b = (torch.randn(*s, generator=g, dtype=F64).requires_grad_(True) for s in ((9, 16), (24, 16), (24,)))
    dy = torch.randn(9, 24, generator=g, dtype=F64)
    F.linear(x, w, b).backward(dy)
    dx, dw, db = BR.linear_bwd(x.detach(), w.detach(), dy)
    assert rel(dx, x.grad) < TOL and rel(dw, w.grad) < TOL and rel(db, b.grad) < TOL
    a, c = torch.randn(12, 8, generator=g, dtype=F64), torch.randn(12, 8, generator=g, dtype=F64)
    assert rel(BR.colsum(a, c, rows_per_group=4, alpha=0.5), 0.5 * (a * c).view(3, 4, 8).sum(1)) < TOL
    assert rel(BR.colsum(a), a.sum(0, keepdim=True)) < TOL
