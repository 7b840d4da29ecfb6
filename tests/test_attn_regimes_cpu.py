"""tests/bwd_ref.py's lazy-reference-point forward variant (O_l) and its score regimes (no GPU): the variant reduces to O_r where the kernel's
trajectory is the row maximum, and every case the regimes sweep runs on the GPU (tests/test_fuzz_attention_gpu.py, the same ids and seeds)
does to the forward's reference point and to the probabilities what its regime promises - which Gaussian operands do not."""
import math

import pytest
import torch

from tests import attn_regime_cases as AC
from tests import bwd_ref as BR

F64 = torch.float64
IDS = AC.sweep_ids()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ref(d, scale, dh, **kw):
    return BR.attention(d["q"], d["k"], d["v"], d["do"], scale, lsum_bf16=dh == 64, **kw)


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("regime,Lkv", [("gaussian", 1), ("gaussian", 17), ("gaussian", 64), ("one_key", 64), ("one_key", 40)])
def test_lazy_variant_is_the_rounding_point_variant_within_one_tile(regime, Lkv, dh):
    d = BR.attention_regime(_g(Lkv), regime, dh, 2, 2, 37, Lkv, dh ** -0.5)
    r = _ref(d, dh ** -0.5, dh)
    assert torch.equal(r["O_l"], r["O_r"])
    assert bool((r["moves"] == 1).all()) and bool((r["last_move"] == 0).all())


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("regime", ["gaussian", "rising", "spike_tail"])
def test_lazy_variant_with_one_tile_and_no_laziness_is_the_rounding_point_variant(regime, dh):
    d = BR.attention_regime(_g(5), regime, dh, 1, 2, 40, 333, 0.25)
    r = _ref(d, 0.25, dh, fwd_tile=333, fwd_lazy=0.0)
    assert torch.equal(r["O_l"], r["O_r"])
    # and with 64-key tiles and no laziness the reference point is the running maximum: it ends at the row maximum, the output within bf16 reach
    r = _ref(d, 0.25, dh, fwd_lazy=0.0)
    cs = 0.25 * BR.LOG2E * r["S"]
    first = (cs == cs.amax(-1, keepdim=True)).to(torch.int8).argmax(-1) // 64
    assert torch.equal(r["last_move"], first)


def test_sweep_grid():
    specs = [AC.sweep_spec(i) for i in IDS]
    assert len(specs) == len(BR.REGIMES) * 3 * 3 * 2
    for s in specs:
        assert BR.regime_fits(s["regime"], s["Lq"], s["Lkv"]) and s["B"] * s["H"] <= 6 and s["B"] * s["H"] * s["Lq"] * s["Lkv"] <= AC.SWEEP_CAP, s
    for regime in BR.REGIMES:
        mine = [s for s in specs if s["regime"] == regime]
        assert len({s["Lkv"] for s in mine}) >= 3 and len({s["Lq"] for s in mine}) >= 2, regime
    assert any(s["Lkv"] > 1024 for s in specs)


def _placement(d, s):
    """spike rows in both 16-row halves of a 32-row group, spike keys in both 32-key blocks and both lane halves of their tile (where the tile
    is wide enough to have them)"""
    rows, keys = d["rows"], d["row_key"]
    assert {int(x) for x in (rows % 32) // 16} == {0, 1}, s
    wide = [int(k) for k in keys if min(64, s["Lkv"] - int(k) // 64 * 64) > max(BR.SPIKE_POS)]
    if wide:
        assert {k % 64 // 32 for k in wide} == {0, 1} and {k % 8 // 4 for k in wide} == {0, 1}, s


def _properties(s, d, r):
    regime, rows, moves, last = s["regime"], d["rows"], r["moves"], r["last_move"]
    cs = s["scale"] * BR.LOG2E * r["S"]
    assert float((s["scale"] * r["S"]).abs().max()) <= 41.0, s            # the fp32 twin's 1e-5 stays meaningful
    if regime == "gaussian":
        assert bool((moves == 1).all()), s
        return
    odd = torch.ones(s["Lq"], dtype=torch.bool)
    odd[rows] = False
    assert bool((moves[..., odd] == 1).all()), ("a row the regime did not choose moved after the first tile", s)
    if regime == "rising":
        assert float((moves[..., rows] >= 3).double().mean()) >= 0.95, s
        return
    if regime == "falling":
        assert bool((moves[..., rows] == 1).all()) and bool((last == 0).all()), s
        return
    _placement(d, s)
    key_tile = d["row_key"] // 64
    own = cs[..., rows, d["row_key"]]                                    # [B, H, rows]: each chosen row's score at its own spike key
    rest = cs[..., rows, :].clone()
    rest[..., torch.arange(len(rows)), d["row_key"]] = -math.inf
    if regime in ("spike_tail", "spike_mid"):
        assert float((own - rest.amax(-1)).min()) >= 12.0, s
        assert bool((last[..., rows] == key_tile).all()) and bool((moves[..., rows] == 2).all()), s
        ntiles = (s["Lkv"] + 63) // 64
        if regime == "spike_tail":
            assert bool((key_tile == ntiles - 1).all()) and s["Lkv"] % 64 != 0, s
        else:
            assert bool((key_tile > 0).all()) and bool((key_tile < ntiles - 1).all()), s
            later = (moves > 1).reshape(-1, s["Lq"])
            groups = [later[:, g0:g0 + 32] for g0 in range(0, s["Lq"], 32)]
            for bh in range(later.shape[0]):
                none = sum(1 for gr in groups if not bool(gr[bh].any()))
                mixed = sum(1 for gr in groups if bool(gr[bh].any()) and not bool(gr[bh].all()))
                assert none >= 1 and mixed >= 1, (none, mixed, s)
    elif regime == "near_threshold":
        assert bool((key_tile > 0).all()), s
        m0 = cs[..., rows, :64].amax(-1)
        gap = own - m0
        assert float((gap - d["row_gap"]).abs().max()) <= 0.25 and float((gap - 8.0).abs().min()) > BR.NEAR_CLEAR, s
        stay = d["row_gap"] < 8.0
        assert int(stay.sum()) > 0 and int((~stay).sum()) > 0, s
        assert bool((moves[..., rows[stay]] == 1).all()), ("a 7.5 row moved", s)
        assert bool((last[..., rows[~stay]] == key_tile[~stay]).all()) and bool((moves[..., rows[~stay]] == 2).all()), ("an 8.5 row stayed", s)
    elif regime == "one_key":
        assert float(r["P"][..., rows, d["row_key"]].min()) >= 0.99, s
        assert bool((key_tile == 0).any()) and (s["Lkv"] <= 64 or bool((key_tile > 0).any())), s
        # dK and dV are concentrated in the dominant keys' rows
        hot = r["dv"][..., d["keys"], :].norm(dim=-1).min()
        cold = torch.ones(s["Lkv"], dtype=torch.bool)
        cold[d["keys"]] = False
        assert float(hot) > 4 * float(r["dv"][..., cold, :].norm(dim=-1).max()), s


@pytest.mark.parametrize("regime", BR.REGIMES)
def test_regime_promises_on_every_sweep_case(regime):
    """Every (variant, scale, seed) case of the regime as the GPU sweep builds it. Prints, per head width, the largest ratio of O_l's worst-row
    error to O_r's: the price of the lazy reference point (docs/PARITY_TOLERANCES.md, "Attention regimes sweep")."""
    ratio, chosen = {128: [], 64: []}, {128: [], 64: []}
    for case_id in IDS:
        s = AC.sweep_spec(case_id)
        if s["regime"] != regime:
            continue
        d = AC.sweep_data(s)
        r = _ref(d, s["scale"], s["dh"])
        _properties(s, d, r)
        e_l, e_r = BR.err(r["O_l"], r["O"]), BR.err(r["O_r"], r["O"])
        for name, e in (("O_l", e_l), ("O_r", e_r), *((n, BR.err(r[n + "_r"], r[n])) for n in ("dq", "dk", "dv"))):
            assert all(math.isfinite(x) for x in e) and e[0] > 0 and e[1] > 0, (name, e, s)
        ratio[s["dh"]].append((e_l[1] / e_r[1], e_l[1], e_r[1]))
        if len(d["rows"]):
            rows = d["rows"]
            c_l, c_r = (BR.err(r[n][..., rows, :], r["O"][..., rows, :])[1] for n in ("O_l", "O_r"))
            chosen[s["dh"]].append((c_l / c_r, c_l, c_r))
    for dh, rs in ratio.items():
        worst = max(rs)
        print(f"{regime} dh {dh}: worst-row err(O_l) / err(O_r) over {len(rs)} cases: max {worst[0]:.2f} ({worst[1]:.2e} vs {worst[2]:.2e}), "
              f"mean {sum(x[0] for x in rs) / len(rs):.2f}"
              + (f"; on the chosen rows alone: max {max(chosen[dh])[0]:.2f} ({max(chosen[dh])[1]:.2e} vs {max(chosen[dh])[2]:.2e})" if chosen[dh] else ""))


def test_gaussian_operands_reach_none_of_it():
    """the control: with today's operands no row's reference point moves after the first tile, at any scale of the sweep - what the regimes add"""
    for scale in (128 ** -0.5, 0.05, 0.25):
        d = BR.attention_regime(_g(3), "gaussian", 128, 1, 2, 300, 1025, scale)
        r = _ref(d, scale, 128, backward=False)
        assert bool((r["moves"] == 1).all()) and float(r["P"].max()) < 0.5
