"""The case tables of tests/workspace_cases.py, checked without a device: the GEMM sequence alternates between different (K-slices, padded tail
tiles) pairs, the shapes of the other entry points are legal and differ in their workspace size, and the size formulas restated there are the
library's own (`*_workspace_bytes`, `*_partials`, `*_slices` are host functions: the built library answers them without a GPU)."""
import pytest

from tests import fwd_ref as FR
from tests import workspace_cases as WC
from tests.test_fuzz_gemm_gpu import GEMM_CASES


def _paths(ncu=256):
    return [FR.gemm_path(GEMM_CASES[i], ncu) for i in WC.GEMM_SEQUENCE]


def test_gemm_sequence_names_the_sweeps_cases_and_their_recorded_paths():
    assert len(WC.GEMM_SEQUENCE) == len(set(WC.GEMM_SEQUENCE)) == 6
    for i, p in zip(WC.GEMM_SEQUENCE, _paths()):
        assert p == GEMM_CASES[i]["path"], (GEMM_CASES[i]["name"], p)
        assert GEMM_CASES[i]["groups"] == 1 and p[0] == 256


def test_gemm_sequence_alternates_slice_counts_and_tail_tiles():
    pairs = [WC.slice_tail(p) for p in _paths()]
    assert pairs == [(8, 24), (5, 48), (3, 72), (1, 0), (8, 24), (8, 8)]
    assert len(set(pairs)) >= 3
    assert sum(n == 1 for n, _ in pairs) == 1 and pairs[0][0] > 1 and pairs[-1][0] > 1, "one unsplit launch, in between"
    ring = pairs + pairs[:1]                                       # the sequence repeats in the back-to-back test
    for seq in (ring, ring[::-1]):
        assert all(a != b for a, b in zip(seq, seq[1:])), seq
    # the K lengths differ too: a slice of the second 24-tile case is half as long as one of the first
    assert GEMM_CASES[WC.GEMM_SEQUENCE[0]]["K"] == 2 * GEMM_CASES[WC.GEMM_SEQUENCE[4]]["K"]
    assert WC.slice_tail(FR.gemm_path(GEMM_CASES[WC.SMALL_M], 256))[0] > 1


def test_gemm_touched_bytes_fit_the_workspace():
    for p in _paths():
        t = WC.gemm_touched_bytes(p)
        assert WC.TICKET_BYTES <= t <= WC.GEMM_WORKSPACE_BYTES
        assert (t == WC.TICKET_BYTES) == (p[2] == 1)
    assert len({WC.gemm_touched_bytes(p) for p in _paths()}) >= 4


def _legal(name, s):
    """what the entry point's host function requires of a shape"""
    base = name.split("/")[0]
    if base == "ug_groupnorm_nhwc":
        cg = s["C"] // s["G"]
        return s["C"] % s["G"] == 0 and s["C"] % 8 == 0 and cg <= 256 and 256 % cg == 0 and s["B"] < 65536
    if base == "ug_colsum":
        return s["rows"] % s["rpg"] == 0 and s["cols"] % 8 == 0 and s["rows"] // s["rpg"] < 65536
    if base == "ug_lora_wgrad":
        return s["R"] in (64, 128, 192, 256) and s["J"] % 64 == 0 and s["M"] > 0
    if base == "ug_flash_attn_bwd":
        return s["dh"] in (64, 128) and min(s["B"], s["H"], s["Lq"], s["Lkv"]) > 0
    if base == "ug_grad_sumsq":
        return all(n > 0 and dt in ("bf16", "f32") for n, dt in s["numels"])
    if base in ("ug_canny_u8", "ug_img_box_blur_u8"):
        return s["C"] in (1, 3) and 1 <= s["B"] < 65536 and 1 <= s["H"] < 65536 and s["W"] >= 1
    raise KeyError(name)


def _size_args(name, s):
    base = name.split("/")[0]
    return {"ug_groupnorm_nhwc": lambda: (s["B"], s["HW"], s["C"], s["G"]), "ug_lora_wgrad": lambda: (s["M"], s["R"], s["J"]),
            "ug_grad_sumsq": lambda: (s["numels"],)}.get(base, lambda: None)()


def _bytes(name, e, s):
    a = _size_args(name, s)
    return e["bytes"](*a) if a is not None else e["bytes"](**s)


@pytest.mark.parametrize("name", list(WC.WORKSPACES))
def test_workspace_shapes_are_legal_and_differ_in_size(name):
    e = WC.WORKSPACES[name]
    assert _legal(name, e["a"]) and _legal(name, e["b"]), name
    na, nb = _bytes(name, e, e["a"]), _bytes(name, e, e["b"])
    assert na > 0 and nb > 0 and na != nb, (name, na, nb)
    assert na % e["unit"] == 0 and nb % e["unit"] == 0 and na > e["unit"], (name, na, nb)


def test_shape_a_makes_more_than_one_partial():
    W = WC.WORKSPACES
    cd = lambda a, b: (a + b - 1) // b
    assert cd(W["ug_groupnorm_nhwc"]["a"]["HW"], 64) == 2 and cd(W["ug_groupnorm_nhwc/fast"]["a"]["HW"], 256) == 2
    assert cd(W["ug_colsum"]["a"]["rpg"], 128) == 2
    assert WC.lora_wgrad_splits(**W["ug_lora_wgrad"]["a"]) == 2 and WC.lora_wgrad_splits(256, 64, 64) == 1
    assert WC.lora_wgrad_splits(**W["ug_lora_wgrad"]["b"]) == 4
    for k in ("ug_flash_attn_bwd/64", "ug_flash_attn_bwd/128"):
        assert W[k]["a"]["Lq"] == 65 and W[k]["b"]["Lq"] % 64 != 0
    p = W["ug_flash_attn_bwd/pair_dq"]
    assert p["a"]["Lq"] < 2048 <= p["b"]["Lq"] and p["b"]["dh"] == 128 and p["b"]["Lq"] % 64 != 0
    assert WC.grad_sumsq_chunks(W["ug_grad_sumsq"]["a"]["numels"]) == 2 and WC.grad_sumsq_chunks(W["ug_grad_sumsq"]["b"]["numels"]) == 6


def test_partial_output_shapes():
    assert [WC.adaln_bwd_partials(r, s) for r, s, _ in WC.ADALN_BWD_PARTIALS] == [1, 2, 25, 341]
    r, s, _ = WC.ADALN_BWD_PARTIALS[1]
    assert s % ((s + WC.adaln_bwd_partials(r, s) - 1) // WC.adaln_bwd_partials(r, s)) != 0          # 7 rows in shares of 4
    r, s, _ = WC.ADALN_BWD_PARTIALS[3]
    p = WC.adaln_bwd_partials(r, s)
    assert p * ((s + p - 1) // p) > s                                                                 # the last partials own no row
    assert all(d % 8 == 0 and d <= 4096 and r % s == 0 for r, s, d in WC.ADALN_BWD_PARTIALS)
    assert [WC.qk_bwd_partials(r, h) for r, h, _ in WC.QK_BWD_PARTIALS] == [1, 583, 600, 2048]
    assert [WC.moe_gate_bwd_slices(S) for S, _, _ in WC.MOE_GATE_BWD_PARTIALS] == [1, 7, 2]
    assert all(D % 8 == 0 and 1 <= E <= 16 for _, D, E in WC.MOE_GATE_BWD_PARTIALS)


@pytest.fixture(scope="module")
def lib():
    from unigen_amd import lib as L
    return L.load()


def test_size_formulas_are_the_librarys(lib):
    assert int(lib.ug_gemm_workspace_bytes()) == WC.GEMM_WORKSPACE_BYTES
    for name, e in WC.WORKSPACES.items():
        base = name.split("/")[0]
        for s in (e["a"], e["b"]):
            want = _bytes(name, e, s)
            if base == "ug_groupnorm_nhwc":
                got = lib.ug_groupnorm_workspace_bytes(s["B"], s["HW"], s["G"])
            elif base == "ug_colsum":
                got = lib.ug_colsum_workspace_bytes(s["rows"], s["cols"], s["rpg"])
            elif base == "ug_lora_wgrad":
                got = lib.ug_lora_wgrad_workspace_bytes(s["M"], s["R"], s["J"])
            elif base == "ug_flash_attn_bwd":
                got = lib.ug_flash_attn_bwd_workspace_bytes(s["B"], s["H"], s["Lq"])
            elif base == "ug_grad_sumsq":
                got = lib.ug_grad_sumsq_workspace_bytes(WC.grad_sumsq_chunks(s["numels"]))
            elif base == "ug_canny_u8":
                got = lib.ug_canny_workspace_bytes(s["B"], s["H"], s["W"])
            else:
                got = lib.ug_img_blur_workspace_bytes(s["B"], s["H"], s["W"], s["C"])
            assert int(got) == want, (name, s, int(got), want)
    for r, s, _ in WC.ADALN_BWD_PARTIALS:
        assert int(lib.ug_adaln_modulate_bwd_partials(r, s)) == WC.adaln_bwd_partials(r, s)
    for r, h, _ in WC.QK_BWD_PARTIALS:
        assert int(lib.ug_qk_rmsnorm_rope_bwd_partials(r, h)) == WC.qk_bwd_partials(r, h)
    for S, _, _ in WC.MOE_GATE_BWD_PARTIALS:
        assert int(lib.ug_moe_gate_bwd_slices(S)) == WC.moe_gate_bwd_slices(S)
