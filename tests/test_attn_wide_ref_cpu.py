"""tests/attn_wide_ref.py on the host: the float64 reference the GPU test of ug_flash_attn_fwd_wide is bounded by, over the GPU test's own case ids.

  - O equals torch.softmax attention in float64 to 1e-10;
  - the rounding-point variant O_v is bwd_ref.forward_lazy at the wide kernel's tile length, its own error against O is nonzero and within the
    project's attention row (4e-3), peaked cases included: max(1.5 x err(O_v), 2^-9) is then a bound a correct kernel can meet and a wrong one not;
  - the bounds catch slips: each of attn_wide_ref.SLIPS, applied to the whole tensor, exceeds the total AND the worst-row bound on at least one
    listed case, and applied to ONE query row it still exceeds the worst-row bound."""
import pytest
import torch

from tests import attn_wide_ref as WR
from tests import bwd_ref as BR

SLIP_CASES = [i for i in WR.case_ids() if WR.case_spec(i)["Lq"] * WR.case_spec(i)["Lkv"] <= 300 * 600]      # every case but the two large gaussian ones


@pytest.mark.parametrize("case_id", WR.case_ids())
def test_reference_is_softmax_attention_and_its_variant_is_within_the_attention_row(case_id):
    d, ref = WR.case_data(case_id), WR.case_reference(case_id)
    q, k, v = (d[n].double() for n in "qkv")
    exact = torch.softmax(d["scale"] * q @ k.transpose(-1, -2), -1) @ v
    assert float((ref["O"] - exact).norm()) <= 1e-10 * float(exact.norm()), case_id
    cs = (d["scale"] * BR.LOG2E) * (q @ k.transpose(-1, -2))
    assert torch.equal(ref["O_v"], BR.forward_lazy(cs, v, False, WR.KV_TILE, WR.LAZY)[0]), ("O_v is not bwd_ref.forward_lazy at 32 keys per tile", case_id)
    total, worst, _ = BR.err(ref["O_v"], ref["O"])
    print(f"{case_id}: err(O_v) rel-L2 {total:.3e}, worst row {worst:.3e}")
    if d["Lkv"] == 1:          # one key: the softmax is 1 and O is that key's value, a bf16 number: the variant rounds nothing (the 2^-9 floor is the bound)
        assert total == 0.0 and worst == 0.0, (case_id, total, worst)
        return
    assert 0.0 < total <= WR.ROW_BOUND and 0.0 < worst <= WR.ROW_BOUND, (case_id, total, worst)
    if len(d["rows"]):
        rt, rw, _ = BR.err(ref["O_v"][..., d["rows"], :], ref["O"][..., d["rows"], :])
        assert 0.0 < rt <= WR.ROW_BOUND and rw <= WR.ROW_BOUND, (case_id, rt, rw)


def test_case_list_covers_what_the_kernel_can_get_wrong():
    ids = WR.case_ids()
    assert len(ids) == len(set(ids)) == len(WR.SHAPES) + len(WR.REGIMES) * len(WR.REGIME_SHAPES) * len(WR.SCALES)
    specs = [WR.case_spec(i) for i in ids]
    assert any(s["Lkv"] % WR.KV_TILE and s["Lkv"] > WR.KV_TILE for s in specs) and any(s["Lkv"] < WR.KV_TILE for s in specs)
    assert any(s["Lq"] > 128 and s["Lq"] % 128 for s in specs) and any(s["H"] > 1 for s in specs) and any(s["B"] > 1 for s in specs)
    for r in WR.REGIMES:                                  # the regimes can be built at their shapes, and their rows are peaked at every scale
        for s in (x for x in specs if x["regime"] == r):
            assert BR.regime_fits(r, s["Lq"], s["Lkv"]) and len(WR.case_data(s["id"])["rows"]) > 0, s


@pytest.mark.parametrize("slip", WR.SLIPS)
def test_the_gpu_bounds_catch_a_slip(slip):
    caught_total, caught_row, caught_one_row = [], [], []
    for case_id in SLIP_CASES:
        d, ref = WR.case_data(case_id), WR.case_reference(case_id)
        bad = WR.slipped(d["q"], d["k"], d["v"], d["scale"], slip)
        if torch.equal(bad.nan_to_num(1e30), ref["O_v"]):                  # the slip has no hold on this case (no ragged tail, no rescale)
            continue
        b_total, b_row = WR.bounds(ref)
        nan = not bool(torch.isfinite(bad).all())                         # nothing written: the GPU test's finiteness check
        total, worst, _ = (float("inf"),) * 3 if nan else BR.err(bad, ref["O"])
        if total > b_total:
            caught_total.append(case_id)
        if worst > b_row:
            caught_row.append(case_id)
        # the same slip confined to the one query row it hurts most: the worst-row bound must see it
        rows_err = (bad.nan_to_num(1e30) - ref["O"]).norm(dim=-1)
        flat = int(rows_err.flatten().argmax())
        one = ref["O_v"].clone().flatten(0, -2)
        one[flat] = bad.nan_to_num(1e30).flatten(0, -2)[flat]
        o_total, o_worst, _ = BR.err(one.view_as(ref["O_v"]), ref["O"])
        if o_worst > b_row:
            caught_one_row.append((case_id, o_total > b_total))
    print(slip, "total:", caught_total, "worst row:", caught_row)
    assert caught_total, f"no listed case puts the slip {slip} over the total bound"
    assert caught_row, f"no listed case puts the slip {slip} over the worst-row bound"
    assert caught_one_row, f"the slip {slip} in one query row is not caught by the worst-row bound on any listed case"
