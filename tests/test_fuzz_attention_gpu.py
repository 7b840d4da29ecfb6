"""The MM-DiT attention forward and backward (flash_attn_kernel, attn_bwd_* of csrc/attention.hip) on peaked softmax rows: the score regimes
of tests/bwd_ref.py (attention_regime; what each one does to the forward's lazy reference point and to the probabilities is checked on the host
by tests/test_attn_regimes_cpu.py, over the same case ids) x {head width 128, 64 with the buffer-form K / V DMAs, 64 with the pointer form} x
three softmax scales x two seeds, through test_fuzz_backward_gpu._run_attention: the layouts, sentinels and bounds of the backward sweep, with

  - the forward bounded by max(1.5 x err(O_l), 2^-9): O_l is bwd_ref's variant with the kernel's rounding points along the kernel's own
    trajectory of the reference point (O_r, which rounds 2^(c S - rowmax), is NOT a bound on peaked rows: a dominant probability of up to 2^8
    carries its own bf16 rounding where O_r has p = 1 exactly);
  - every bound of the whole tensor repeated on the rows the regime acts on (O, dq) and on the keys it spikes (dk, dv): a wrong rescale on a
    quarter of the rows must not hide in the total;
  - ug_flash_attn_fwd (no LSE) bit-identical to ug_flash_attn_fwd_lse, ug_flash_attn_fwd_f32 on the widened operands within 1e-5 / 1e-4;
  - every element of the operand buffers that is not an operand NaN (in bounds: spare rows, pad columns): all outputs finite, sentinels intact.

Three regimes also go through autograd.FlashAttention on fp32 tensors (the GEMM-formulation verification backward).
Tolerances and measured errors: docs/PARITY_TOLERANCES.md, "Attention regimes sweep"."""
import random

import pytest
import torch

from tests import attn_regime_cases as AC
from tests import bwd_ref as BR
from tests.test_fuzz_backward_gpu import F32, _attn_case, _check, _run_attention, _tail

pytestmark = pytest.mark.gpu


def _pin_dma(c, rng, variant):
    """Pin the K / V row strides to the DMA form the variant names: the dispatcher takes the buffer form at head width 64 when both strides are
    equal and a multiple of 16 elements. H dh is a multiple of 64, so a stride's residue mod 16 is its pad's."""
    if variant == "dh128":
        return c
    P = list(c["pads"])
    if variant == "dh64_buf":
        if c["joint"]:
            c["kv_shared"] = True
            P[0] = 16 * rng.choice([0, 1, 4])
        elif c["kv_shared"]:
            P[1] = 16 * rng.choice([0, 1, 4])
        else:
            P[1] = P[2] = 16 * rng.choice([0, 1, 4])
    elif c["kv_shared"]:                                # pointer form, one stride for both: % 16 == 8
        P[0 if c["joint"] else 1] = rng.choice([8, 24])
    elif not c["joint"]:                                # two buffers: unequal strides, or equal and % 16 == 8
        P[1], P[2] = rng.choice([(0, 16), (16, 64), (8, 0), (8, 8), (24, 24)])
    # (joint with v in its own buffer: k's row holds 2 H dh + pad, v's H dh + pad - unequal whatever the pads)
    c["pads"] = P
    return c


def _rows_only(name, got, ref, key, idx, case):
    """the bound of the whole tensor again on the rows `idx` alone (backward with the forward's LSE: the `*_rl` variant, as _run_attention)"""
    if idx is None or len(idx) == 0:
        return
    mag = ref.get(key + "_m")
    var = "O_l" if key == "O" else key + ("_rl" if case.get("mode") == "lse" else "_r")
    _check(name, got[..., idx, :], ref[key][..., idx, :], case, var=ref[var][..., idx, :],
           mag=None if mag is None else mag[..., idx, :])


@pytest.mark.parametrize("case_id", AC.sweep_ids())
def test_attention_regimes(gpu, case_id):
    s = AC.sweep_spec(case_id)
    d = AC.sweep_data(s)
    rng = random.Random("layout-" + case_id)
    c = _pin_dma(_attn_case(rng, s["dh"], s["B"], s["H"], s["Lq"], s["Lkv"]), rng, s["variant"])
    c.update(scale=s["scale"], id=case_id)
    r = _run_attention(gpu, c, s["seed"], data=d)
    if s["dh"] == 64:
        assert (r["k_rs"] == r["v_rs"] and r["k_rs"] % 16 == 0) == (s["variant"] == "dh64_buf"), ("the case does not pin its DMA form", c)
    ref, rows, keys = r["ref"], d["rows"], d["keys"]
    assert bool(torch.isfinite(r["o"]).all()) and bool(torch.isfinite(r["lse2"]).all()), ("a NaN of the padding reached the forward's outputs", c)
    for mode, got in r["runs"].items():
        for n, t in got.items():
            assert bool(torch.isfinite(t).all()), (f"a NaN of the padding reached {n}", mode, c)
    _rows_only("forward O, chosen rows", r["o"], ref, "O", rows, c)
    for mode, got in r["runs"].items():
        _rows_only(f"bwd[{mode}] dq, chosen rows", got["dq"], ref, "dq", rows, dict(c, mode=mode))
        _rows_only(f"bwd[{mode}] dk, spike keys", got["dk"], ref, "dk", keys, dict(c, mode=mode))
        _rows_only(f"bwd[{mode}] dv, spike keys", got["dv"], ref, "dv", keys, dict(c, mode=mode))
    # the two other forward entry points
    assert torch.equal(r["forward_again"](torch.bfloat16), r["o_buf"]), ("ug_flash_attn_fwd and ug_flash_attn_fwd_lse differ", c)
    o32 = r["heads"](r["forward_again"](F32), 0, 0, s["Lq"])
    assert bool(torch.isfinite(o32).all()), c
    _check("fp32 forward O", o32, ref["O"], c, rows_from=_tail(s["Lq"]))


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("B,H,Lq,Lkv", [(1, 2, 100, 333), (2, 1, 33, 520)])
@pytest.mark.parametrize("regime", ["rising", "near_threshold", "one_key"])
def test_attention_regimes_fp32_verification_path(gpu, regime, B, H, Lq, Lkv, dh):
    """autograd.FlashAttention on fp32 tensors: ug_flash_attn_fwd_f32 and the GEMM formulation of the backward (row_lse, attn_prob, attn_dscore on
    peaked rows), against torch autograd in float64 on the same operands (which bwd_ref.attention, whose cancellation magnitudes the bound needs,
    must reproduce to 1e-10 first); q, k | v inside wider buffers whose pad columns hold NaN."""
    from unigen_amd import autograd as A
    D, scale = H * dh, dh ** -0.5
    c = dict(regime=regime, dh=dh, B=B, H=H, Lq=Lq, Lkv=Lkv)
    d = BR.attention_regime(torch.Generator().manual_seed(dh + len(regime)), regime, dh, B, H, Lq, Lkv, scale)
    flat = lambda t: t.transpose(1, 2).reshape(B, t.shape[2], D).float()
    Q = torch.full((B, Lq, D + 8), float("nan"))
    KV = torch.full((B, Lkv, 2 * D + 8), float("nan"))
    Q[..., :D], KV[..., :D], KV[..., D:2 * D] = flat(d["q"]), flat(d["k"]), flat(d["v"])
    Qg, KVg = Q.to(gpu).requires_grad_(True), KV.to(gpu).requires_grad_(True)
    out = A.attention(Qg[..., :D], KVg[..., :D], KVg[..., D:2 * D], H)
    out.backward(flat(d["do"]).to(gpu))
    torch.cuda.synchronize()
    hd = lambda t, L_: t.reshape(B, L_, H, dh).transpose(1, 2).double()
    o = hd(out.detach().cpu(), Lq)
    ref = BR.attention(d["q"], d["k"], d["v"], d["do"], scale, o=o, fwd_tile=None)
    q64, k64, v64 = (d[n].double().requires_grad_(True) for n in "qkv")
    o64 = torch.softmax(scale * q64 @ k64.transpose(-1, -2), -1) @ v64
    o64.backward(d["do"].double())
    exact = BR.attention(d["q"], d["k"], d["v"], d["do"], scale, fwd_tile=None)
    for n, t in (("O", o64.detach()), ("dq", q64.grad), ("dk", k64.grad), ("dv", v64.grad)):
        assert float((exact[n] - t).norm()) <= 1e-10 * float(t.norm()), ("bwd_ref.attention against torch autograd in float64", n, c)
    ref = dict(ref, O=o64.detach(), dv=v64.grad)                 # dq, dk: bwd_ref's, with delta from the O the backward read
    _check("fp32 forward O", o, ref["O"], c)
    gq, gkv = Qg.grad.cpu(), KVg.grad.cpu()
    assert float(gq[..., D:].abs().max()) == 0.0 and float(gkv[..., 2 * D:].abs().max()) == 0.0, ("gradient in the pad columns", c)
    for n, got, rows, idx in (("dq", gq[..., :D], Lq, d["rows"]), ("dk", gkv[..., :D], Lkv, d["keys"]), ("dv", gkv[..., D:2 * D], Lkv, d["keys"])):
        got = hd(got, rows)
        assert bool(torch.isfinite(got).all()), (n, c)
        _check(f"fp32 bwd {n}", got, ref[n], c, mag=ref.get(n + "_m"), rows_from=_tail(rows))
        if idx is not None and len(idx):
            mag = ref.get(n + "_m")
            _check(f"fp32 bwd {n}, chosen rows", got[..., idx, :], ref[n][..., idx, :], c, mag=None if mag is None else mag[..., idx, :])
