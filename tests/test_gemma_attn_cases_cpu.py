"""What the case grid of tests/gemma_attn_cases.py promises, checked on the host in float64: the coverage of the geometry table, every regime's gaps
on the realised scores of the rounded operands, the dead rows, the two bounds the device sweep (tests/test_fuzz_gemma_gpu.py) uses - computed from the
references alone and printed - and that each mutant of gemma_ref.attention, judged like a kernel output, misses some case's bf16 bound by 2 x or more."""
import functools

import pytest
import torch

from tests import gemma_attn_cases as G
from tests import gemma_ref as R

F64 = torch.float64
GEOMETRY, REGIME = G.case_ids("geometry"), G.case_ids("regime")


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def test_the_grid_covers_what_it_says():
    geo = [c for c in G.cases() if c["kind"] == "geometry"]
    reg = [c for c in G.cases() if c["kind"] != "geometry"]
    assert 55 <= len(geo) <= 70 and 25 <= len(reg) <= 35, (len(geo), len(reg))
    assert G.case_ids() == [c["id"] for c in G.cases()] and len(set(G.case_ids())) == len(G.cases())
    assert {c["L"] for c in geo} == set(G.GEO_L) and {c["window_spec"] for c in geo} == set(G.GEO_WINDOWS)
    assert {n for c in geo if c["kv_spec"] for n in c["kv_spec"]} == set(G.GEO_KV) and {len(c["kv_spec"]) for c in geo if c["kv_spec"]} == {2, 3}
    assert {(c["H"], c["KV"]) for c in geo} == set(G.LAYOUTS) and {c["cap"] for c in geo} == set(G.CAPS)
    assert any(c["kv_spec"] == [0, "L"] for c in geo) and any(c["kv_spec"] == ["L", 1] for c in geo)
    for w in G.EDGE_WINDOWS:                                            # each edge window with lengths more than a tile beyond it
        assert sum(c["window"] == w and c["L"] > w + G.KT for c in geo) >= 2, w
    for n in G.GEO_KV:                                                  # each key-length edge without a window and with one of a tile or more
        has = lambda pred: any(c["kv_spec"] and n in c["kv_spec"] and pred(c) for c in geo)
        assert has(lambda c: c["window"] == 0) and has(lambda c: G.KT <= c["window"] < c["L"]), n
    # a whole workgroup without a live key: the second workgroup's first key max(0, 128 - window + 1) lies at or beyond the sample's key length
    assert sum(c["L"] > G.AQ and c["window"] and c["kv_len"] is not None and any(0 < n and n + c["window"] < G.AQ for n in c["kv_len"]) for c in geo) >= 2
    assert {c["kind"] for c in reg} == set(G.REGIMES) and {c["L"] for c in reg} == {96, 160, 300}
    assert {c["window"] for c in reg if c["kind"] == "spike_window_first"} == {32, 33, 97}
    assert {c["cap"] for c in reg if c["kind"] == "saturated"} == {4.0, 50.0}
    for c in reg:
        if c["kind"] == "spike_window_first":                           # the first chosen row's dominant key is the last key of a tile, and all four waves occur
            rows = G.regime_rows(c)
            assert (rows[0] - c["window"] + 1) % G.KT == G.KT - 1
    for kind in ("rising", "falling", "spike_diag", "spike_window_first"):          # all four waves of a workgroup
        assert {(r % G.AQ) // 32 for c in reg if c["kind"] == kind for r in G.regime_rows(c)} == {0, 1, 2, 3}, kind
    # both lane halves: a lane of the upper half holds the keys 4 .. 7 of every eight
    assert {(r - c["window"] + 1) % 8 // 4 for c in reg if c["kind"] == "spike_window_first" for r in G.regime_rows(c)} == {0, 1}
    assert {(n - 1) % 8 // 4 for c in reg if c["kind"] == "spike_kvlen_last" for n in c["kv_len"]} == {0, 1}


# ---- promises and bounds, one case at a time ---------------------------------------------------------------------------------------------
def _dead_by_hand(c):
    """rows without a live key from the definition alone: the keys of row r are max(0, r - window + 1) .. min(r, kv_len - 1)"""
    B, L, w = c["B"], c["L"], c["window"]
    dead = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        n = L if c["kv_len"] is None else c["kv_len"][b]
        for r in range(L):
            dead[b, r] = (max(0, r - w + 1) if w else 0) > min(r, n - 1)
    return dead


def _check_regime(c, d, rf):
    pre, fin = G.scores(c, d)
    live = rf["live"][:, None].expand_as(fin)
    masked = fin.masked_fill(~live, float("-inf"))
    B, H, L = c["B"], c["H"], c["L"]
    rows, kind = d["rows"], c["kind"]
    if kind in ("rising", "falling"):
        nt = (L + G.KT - 1) // G.KT
        pad = torch.full((B, H, L, nt * G.KT), float("-inf"), dtype=F64)
        pad[..., :L] = masked
        tmax = pad.view(B, H, L, nt, G.KT).amax(-1)[:, :, rows]         # [B, H, rows, tiles]
        gain = (tmax[..., 1:] - tmax[..., :-1]) * (1.0 if kind == "rising" else -1.0)
        both = torch.isfinite(tmax[..., 1:]) & torch.isfinite(tmax[..., :-1])
        assert bool(both.any()) and float(gain[both].min()) >= G.RAMP - G.RAMP_CLEAR, (c["id"], float(gain[both].min()))
        return f"tile maximum moves by {float(gain[both].min()):.2f} .. {float(gain[both].max()):.2f} per live tile"
    if kind == "saturated":
        sat = (pre.abs() >= 8 * c["cap"]) & live
        share, pos, neg = (float((m & live).sum()) / float(live.sum()) for m in (sat, sat & (pre > 0), sat & (pre < 0)))
        assert share >= 0.8 and pos >= 0.3 and neg >= 0.3, (c["id"], share, pos, neg)
        assert bool((torch.tanh(pre / c["cap"])[sat].abs() == 1.0).all()), "the saturated pairs do not tie at exactly +- cap"
        return f"{share:.3f} of the live pairs at |scale q.k| >= 8 cap ({pos:.3f} above, {neg:.3f} below), all at exactly +- cap"
    worst = float("inf")
    for b in range(B):
        for i, r in enumerate(rows.tolist()):
            key = int(d["row_key"][b, i])
            if key < 0:
                continue
            assert bool(rf["live"][b, r, key]), (c["id"], b, r, key)
            others = masked[b, :, r].clone()
            others[:, key] = float("-inf")
            gap = fin[b, :, r, key] - others.amax(-1)                     # -inf others (a row of one key): an infinite gap
            worst = min(worst, float(gap.min()))
            if kind != "spike_diag":                                    # the hidden key behind the window / at kv_len: higher still, and 1e4 in V
                hid = key - 1 if kind == "spike_window_first" else key + 1
                assert not bool(rf["live"][b, r, hid]) and bool(d["planted"][b, hid]) and bool((d["v"][b, hid] == G.BIG_V).all())
                assert float((fin[b, :, r, hid] - fin[b, :, r, key]).min()) >= G.SPIKE - G.SPIKE_CLEAR, (c["id"], b, r)
    assert worst >= G.SPIKE - G.SPIKE_CLEAR, (c["id"], worst)
    return f"dominant key at least {worst:.2f} above every other live key"


@functools.lru_cache(maxsize=None)
def summary(case_id):
    """everything the aggregate tests need of one case: its bounds and the promise line (the tensors are dropped)"""
    c, d, rf = G.case(case_id), G.case_data(case_id), G.refs(case_id)
    for n in "qkv":
        assert torch.equal(R.bf(d[n]), d[n]), (case_id, n, "not bf16-representable")
    assert tuple(d["q"].shape) == (c["B"], c["L"], c["H"], G.DH) and tuple(d["k"].shape) == tuple(d["v"].shape) == (c["B"], c["L"], c["KV"], G.DH)
    assert bool(torch.isfinite(d["v"]).all()) and bool(torch.isfinite(d["k"]).all())          # rows in [kv_len, L) are operands: finite
    assert torch.equal(rf["dead"], _dead_by_hand(c)), (case_id, "dead rows")
    for name in ("truth", "variant", "host32"):
        t = rf[name]
        if t is None:
            continue
        assert bool((t[rf["dead"]] == 0).all()), (case_id, name, "a dead row is not zero")
        assert bool(torch.isfinite(t).all()) and bool((t[~rf["dead"]].norm(dim=-1) > 0).all()), (case_id, name)
    line = _check_regime(c, d, rf) if c["kind"] != "geometry" else f"{int(rf['dead'].sum())} dead rows"
    return dict(bounds=G.bounds(c, rf), line=line)


@pytest.mark.parametrize("case_id", G.case_ids())
def test_case_promises_and_bounds(case_id):
    s = summary(case_id)
    print(f"{case_id}: {s['line']}")
    for (dt, group), (b, bw) in sorted(s["bounds"].items()):
        print(f"    {dt} {group}: rel-L2 bound {b:.3e}, worst-row bound {bw:.3e}")
        assert b > 0 and bw > 0


def test_the_regime_bounds_track_the_variant():
    """on at least 3/4 of the regime cases the bf16 rel-L2 bound of the clean rows is 1.5 x the rounding-point variant's own error, not the 2^-9 floor"""
    above = [cid for cid in REGIME if summary(cid)["bounds"]["bf16", "clean"][0] > G.FLOOR]
    print(f"regime cases whose bf16 bound is above the floor: {len(above)} of {len(REGIME)} = {len(above) / len(REGIME):.3f}; at the floor: "
          f"{sorted(set(REGIME) - set(above))}")
    assert len(above) >= 0.75 * len(REGIME)


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
def _candidates(mutant):
    """the cases built to catch the mutant first, then every other one (a mutant only the tail catches still counts)"""
    by = lambda pred: [c["id"] for c in G.cases() if pred(c)]
    first = {"window+1": by(lambda c: c["kind"] == "spike_window_first"), "window-1": by(lambda c: c["kind"] == "spike_window_first"),
             "tile_skip_early": by(lambda c: c["kind"] == "spike_window_first"), "kvlen+1": by(lambda c: c["kind"] == "spike_kvlen_last"),
             "group_mod": by(lambda c: c["H"] // c["KV"] > 1 and c["KV"] > 1), "no_rescale": by(lambda c: c["kind"] == "rising"),
             "cap_as_clamp": by(lambda c: c["kind"] == "geometry" and c["cap"] == 4.0 and c["L"] >= 32)}[mutant]
    return first + [cid for cid in G.case_ids() if cid not in first]


def test_every_mutant_is_caught():
    caught = []
    for mutant in R.MUTANTS:
        for cid in _candidates(mutant):
            c, d, rf = G.case(cid), G.case_data(cid), G.refs(cid)
            got = R.attention(d["q"], d["k"], d["v"], G.SCALE, c["cap"], c["window"], c["kv_len"], mutant=mutant)
            ratio, _ = G.judge(c, rf, got, True)
            if ratio >= 2.0:
                print(f"mutant {mutant}: caught by {cid}, {ratio:.3g} x its bf16 bound")
                caught.append(mutant)
                break
        else:
            print(f"mutant {mutant}: no case catches it")
    assert caught == list(R.MUTANTS), sorted(set(R.MUTANTS) - set(caught))


def test_mutant_argument_changes_nothing_by_default():
    cid = GEOMETRY[1]
    c, d = G.case(cid), G.case_data(cid)
    args = (d["q"], d["k"], d["v"], G.SCALE, c["cap"], c["window"], c["kv_len"])
    assert torch.equal(R.attention(*args), R.attention(*args, mutant=None)) and torch.equal(R.attention(*args), G.refs(cid)["truth"])
    with pytest.raises(AssertionError):
        R.attention(*args, mutant="window+2")
    with pytest.raises(AssertionError):
        R.attention(*args, rnd=R.bf, mutant="window+1")
