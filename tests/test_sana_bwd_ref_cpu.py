"""tests/sana_bwd_ref.py on the host: the closed forms are the gradients torch autograd takes of tests/sana_ref's float64 forwards; every named slip
is further from the truth than the bf16 bound of tests/test_sana_bwd_kernels_gpu.py (1.5 x err(G_v)) on at least one listed case - so the GPU bounds
catch each of them; the references are finite; the rows and heads whose forward output is identically zero have exactly zero gradients."""
import pytest
import torch

from tests import bwd_ref as BR
from tests import sana_bwd_ref as G
from tests import sana_ref as R

F64 = torch.float64
SMALL_ATTN = ["gaussian-1x1x1", "gaussian-1x2x33", "gaussian-2x3x64", "gaussian-1x4x257", "negative_query_row-1x2x33", "negative_key_head-2x3x64",
              "cancelling-1x2x300"]
SMALL_GLU = ["glu-1x1x1x8-pad0", "glu-1x1x5x16-pad0", "glu-1x6x1x16-pad0", "glu-2x5x7x40-pad0", "glu-1x3x70x16-pad0", "glu-1x17x33x8-pad0"]


@pytest.mark.parametrize("case_id", SMALL_ATTN)
def test_attention_closed_form_is_autograd(case_id):
    d = G.attn_case(case_id)
    q, k, v = (d[n].to(F64).requires_grad_(True) for n in "qkv")
    (R.linear_attention(q, k, v) * d["do"].to(F64)).sum().backward()
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        diff, mag = (d["G"][name] - t.grad).norm(dim=-1), d["G"]["mag"][name].norm(dim=-1)       # against what cancels: one token gives exact zeros
        assert bool((diff <= 1e-12 * mag).all()), (case_id, name, float((diff / mag.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("case_id", SMALL_GLU)
def test_glu_closed_form_is_autograd(case_id):
    d = G.glu_case(case_id)
    x, w, b = (d[n].to(F64).requires_grad_(True) for n in "xwb")
    (R.glu_dwconv(x, w, b) * d["do"].to(F64)).sum().backward()
    for name, t in (("dx", x), ("dw", w), ("db", b)):
        total, _, _ = BR.err(d["G"][name], t.grad)
        assert total <= 1e-12, (case_id, name, total)


def _caught(cases, case_fn, slipped, names):
    """the cases on which a slipped result exceeds the GPU test's bound on some tensor (total or worst row)"""
    hit = []
    for cid in cases:
        d = case_fn(cid)
        s = slipped(d)
        for n in names:
            mag = d["G"]["mag"].get(n) if (d.get("N") == 1 and n != "dv") else None        # as tests/test_sana_bwd_kernels_gpu.py applies it
            b_total, b_row = G.bounds(d["G"][n], d["G_v"][n], mag)
            total, worst, _ = BR.err(s[n], d["G"][n], mag)
            if total > b_total or worst > b_row:
                hit.append((cid, n))
    return hit


@pytest.mark.parametrize("slip", G.ATTN_SLIPS)
def test_attention_slips_exceed_the_bound(slip):
    hit = _caught(G.attn_case_ids(), G.attn_case, lambda d: G.linear_attention_bwd(d["q"], d["k"], d["v"], d["do"], slip=slip), ("dq", "dk", "dv"))
    print(slip, hit)
    assert hit, f"the slip {slip} passes the bound on every attention case: the case list does not see it"


@pytest.mark.parametrize("slip", G.GLU_SLIPS)
def test_glu_slips_exceed_the_bound(slip):
    hit = _caught(G.glu_case_ids(), G.glu_case, lambda d: G.glu_dwconv_bwd(d["x"], d["w"], d["b"], d["do"], slip=slip), ("dx", "dw", "db"))
    print(slip, hit)
    assert hit, f"the slip {slip} passes the bound on every convolution case: the case list does not see it"


def test_references_are_finite_and_zero_where_the_forward_is():
    for cid in G.attn_case_ids():
        d = G.attn_case(cid)
        for n in ("dq", "dk", "dv"):
            assert bool(torch.isfinite(d["G"][n]).all()) and bool(torch.isfinite(d["G_v"][n]).all()), (cid, n)
    for cid in G.glu_case_ids():
        d = G.glu_case(cid)
        for n in ("dx", "dw", "db"):
            assert bool(torch.isfinite(d["G"][n]).all()) and bool(torch.isfinite(d["G_v"][n]).all()), (cid, n)
    d = G.attn_case("negative_query_row-1x2x33")
    assert bool((d["G"]["dq"][0, 1, 17] == 0).all()), "a query row without a positive entry has no gradient"
    d = G.attn_case("negative_key_head-2x3x64")
    for n in ("dq", "dk", "dv"):
        assert bool((d["G"][n][1, 2] == 0).all()), (n, "a head without a positive key entry has no gradient")


def test_case_lists():
    assert G.attn_case_ids() == R.attn_case_ids() and G.glu_case_ids()[:len(R.GLU_SHAPES)] == R.glu_case_ids()
    assert "glu-1x17x33x8-pad0" in G.glu_case_ids()
    d = G.glu_case("glu-1x17x33x8-pad0")
    assert d["H"] * d["W"] > 2 * G.SLAB and (d["H"] * d["W"]) % G.SLAB and G.SLAB % d["W"]       # three slabs, the last partial, boundaries mid-row
    assert any(G.attn_case(c)["N"] % G.BWD_CHUNK and G.attn_case(c)["N"] > G.BWD_CHUNK for c in ("gaussian-1x4x257", "cancelling-1x2x300"))
