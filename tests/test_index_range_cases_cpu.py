"""The index-range sweep without a GPU: every entry of tests/index_range_cases.py is what it claims to be (its byte offsets cross 2^31 / 2^32
where it says so, computed from the geometry; the dispatch predicates hold), the slips a far view or a packed coordinate can suffer are
rejected by the judging functions the GPU tests use, and the row-stride refusals of ug_flash_attn_fwd / _fwd_lse / _bwd come before any launch
(fake aligned pointers, as tests/test_attn_wide_code_object_cpu.py; a refused call is never followed by an accepted one: there is no GPU here)."""
import pytest
import torch

from tests import bwd_ref as BR
from tests import index_range_cases as IC
from tests import vae_kernel_ref as VR

B31, B32 = 1 << 31, 1 << 32


# ----------------------------------------------------------------------------------------------------------------------------------
# the row-stride rule
# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_documented_row_stride_limit_is_sound():
    """the kernels' tile offsets are (unsigned)(row * (int)rs + ch * 8) * 2u over rows 0..63 and chunks 0..15: the int product must not overflow
    (63 rs + 120 < 2^31), and then the doubled value fits 32 bits; the documented limit lies below that, and below the issue's 2^25"""
    assert 63 * IC.ATTN_RS_SOUND + 120 < B31 <= 63 * (IC.ATTN_RS_SOUND + 1) + 120
    assert IC.ATTN_RS_LIMIT <= 1 << 25 and IC.ATTN_RS_LIMIT - 8 <= IC.ATTN_RS_SOUND
    assert 2 * (63 * (IC.ATTN_RS_LIMIT - 8) + 120) < B31            # even as a signed byte offset
    assert IC.ATTN_RS_FAR % 16 == 0 and IC.ATTN_RS_FAR + 16 == IC.ATTN_RS_LIMIT
    assert 21504 < IC.ATTN_RS_LIMIT                                 # the widest row of the package (the single blocks' fused buffer)


def _fwd_args(**kw):
    P = 4096
    a = dict(q=P, q_rs=256, q_bs=64 * 256, k=P, k_rs=256, k_bs=64 * 256, v=P, v_rs=256, v_bs=64 * 256, o=P, o_rs=256, o_bs=64 * 256)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    P = 4096
    a = {}
    for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
        a[n], a[n + "_rs"], a[n + "_bs"] = P, 256, 64 * 256
    assert set(kw) <= set(a), kw
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("fn", ["ug_flash_attn_fwd", "ug_flash_attn_fwd_lse", "ug_flash_attn_bwd"])
@pytest.mark.parametrize("dh", [128, 64])
def test_attention_row_stride_refusals(fn, dh):
    """each row-stride argument of each entry point at the limit and at -512: UG_ERR_UNSUPPORTED, the message names the row strides; also 0.
    (2, 64, 64) problems that would be accepted but for the one field; every call here is refused before any launch"""
    from unigen_amd import lib
    cdll = lib.load()
    P = 4096
    names = IC.ATTN_BWD_ROW_STRIDES if fn.endswith("bwd") else IC.ATTN_FWD_ROW_STRIDES
    assert names == tuple(n for n in ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "dq_rs", "dk_rs", "dv_rs") if n in names)
    for name in names:
        for bad in (IC.ATTN_RS_LIMIT, -512, 0, IC.ATTN_RS_LIMIT + 512, 1 << 32):
            if fn == "ug_flash_attn_fwd":
                rc = cdll.ug_flash_attn_fwd(*_fwd_args(**{name: bad}), 1, 2, 64, 64, dh, dh ** -0.5, None)
            elif fn == "ug_flash_attn_fwd_lse":
                rc = cdll.ug_flash_attn_fwd_lse(*_fwd_args(**{name: bad}), 1, 2, 64, 64, dh, dh ** -0.5, P, 64, None)
            else:
                rc = cdll.ug_flash_attn_bwd(*_bwd_args(**{name: bad}), 1, 2, 64, 64, dh, dh ** -0.5, None, P, 1 << 20, None)
            msg = cdll.ug_last_error()
            assert rc == lib.UG_ERR_UNSUPPORTED, (fn, name, bad, rc, msg)
            assert b"row strides" in msg and b"2^24" in msg, (fn, name, bad, msg)


# ----------------------------------------------------------------------------------------------------------------------------------
# the far-view tables
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IC.ATTN_FAR_CASES + IC.ATTN_BATCH_CASES, ids=lambda c: c["name"])
def test_attention_cases_cross_the_boundaries_they_claim(c):
    D = c["H"] * c["dh"]
    lay = IC.attn_layout(c)
    assert set(lay) == set(IC.ATTN_OPERANDS)
    assert c["rs"] % 16 == 0 and c["bs"] % 8 == 0 and 0 < c["rs"] < IC.ATTN_RS_LIMIT
    for n, off in lay.items():
        rows = IC.attn_rows(c, n)
        assert 2 * off >= B31, (n, "an offset cut to 32 bits could leave the arena")
        assert off % 8 == 0                                            # 16-byte aligned in an arena whose base is
        last_of_batch0 = 2 * IC.view_extent(off, c["rs"], c["bs"], 1, rows, D + IC.SENT_COLS)
        first_of_batch1 = 2 * (off + c["bs"])
        assert last_of_batch0 <= first_of_batch1, (n, "the batches overlap")
        assert first_of_batch1 >= B32 and 2 * c["bs"] >= B32, (n, "batch 1 does not lie past 2^32 bytes, of the arena and from the operand's base")
        assert 2 * off < B32                                           # and batch 0 starts below it: both sides of the boundary
        assert c["B"] == 2
    # the operands of one row do not overlap (sentinels included), and every one fits the row stride
    spans = sorted((off, off + D + (IC.SENT_COLS if n in IC.ATTN_OUTPUTS else 0)) for n, off in lay.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] - spans[0][0] <= c["rs"]
    assert 2 * IC.attn_arena_elems(c) <= 12 * IC.GIB < IC.MEMORY_CAP
    if c in IC.ATTN_FAR_CASES:
        assert c["rs"] == IC.ATTN_RS_FAR
        # the last row of a 64-row tile lies less than 64 MiB below byte offset 2^31 of its tile (bit 30 of the offset set): the top of what the
        # documented rule lets a tile offset reach
        assert B31 - (1 << 26) < 2 * (63 * c["rs"] + 120) < B31
        assert 2 * (IC.attn_rows(c, "k") - 1) * c["rs"] >= B31 or c["Lkv"] <= 65
    else:
        assert c["rs"] == 8 * D + 4 * IC.SENT_COLS and max(c["Lq"], c["Lkv"]) <= 300


def test_attention_cases_cover_both_dma_forms_at_their_boundary():
    """head width 64 at the largest stride: Lkv = 64 is the last length on the buffer form, 65 the first on the pointer form"""
    rs = IC.ATTN_RS_FAR
    assert IC.bufd_ok(rs, rs, 64) and not IC.bufd_ok(rs, rs, 65)
    assert not IC.bufd_ok(rs, rs + 16, 64) and not IC.bufd_ok(rs - 8, rs - 8, 64)
    far64 = [c for c in IC.ATTN_FAR_CASES if c["dh"] == 64]
    assert {IC.bufd_ok(c["rs"], c["rs"], c["Lkv"]) for c in far64} == {True, False}
    assert {c["Lkv"] for c in far64} >= {64, 65, 130} and {c["Lq"] for c in far64} == {64, 130}
    far128 = [c for c in IC.ATTN_FAR_CASES if c["dh"] == 128]
    assert {c["Lkv"] for c in far128} >= {64, 65, 130} and {c["Lq"] for c in far128} == {64, 130}
    for c in IC.ATTN_FAR_CASES:
        assert ("buf" in c["name"]) == (c["dh"] == 64 and IC.bufd_ok(c["rs"], c["rs"], c["Lkv"])), c["name"]
    assert {c["dh"] for c in IC.ATTN_BATCH_CASES} == {64, 128}
    for c in IC.ATTN_BATCH_CASES:                                       # compact rows: the buffer form at head width 64
        assert c["dh"] == 128 or IC.bufd_ok(c["rs"], c["rs"], c["Lkv"])


@pytest.mark.parametrize("c", IC.WIDE_FAR_CASES, ids=lambda c: c["name"])
def test_wide_cases_cross_the_boundaries_they_claim(c):
    assert c["rs"] == (1 << 24) - 8 and c["rs"] % 8 == 0
    for size in (2, 4):
        lay = IC.wide_layout(c, size)
        for n, off in lay.items():
            assert size * off >= B31 and (size * off) % 16 == 0
            assert size * (off + c["bs"]) >= B32 and size * off < B32             # batch 1 past byte 2^32 of the arena, batch 0 below it
        assert size * c["bs"] >= (B31 if size == 2 else B32)                      # and, from the operand's own base, past 2^31 (bf16) / 2^32 (fp32)
        assert IC.wide_arena_bytes(c, size) <= 12 * IC.GIB
        # the last key row of batch 0 lies past 2^31 bytes from the operand's base in the three-tile case, just below it in the others
        assert (size * (c["Lkv"] - 1) * c["rs"] >= B31) == (c["Lkv"] == 70)
    assert {x["Lkv"] for x in IC.WIDE_FAR_CASES} == {32, 33, 70}
    assert IC.WIDE_CANVAS["Lkv"] == (4096 // 8) ** 2 and IC.WIDE_CANVAS["Lq"] == 130


# ----------------------------------------------------------------------------------------------------------------------------------
# packed convolution coordinates
# ----------------------------------------------------------------------------------------------------------------------------------
def test_conv256_high_bit_cases_take_the_route_and_set_the_bits():
    new = VR.CONV256_CASES[-IC.CONV256_HIGH_BITS:]
    for c in new:
        assert VR.conv_takes_256(c), c
        assert (c["B"] * c["Ho"] * c["Wo"]) % 256 == 0 and (c["Cin"], c["Cout"], c["KH"], c["KW"]) == (128, 256, 3, 3), c
    assert max(c["Wo"] for c in new) == 4032 and max(c["Ho"] for c in new) == 4032 and max(c["B"] for c in new) == 252
    assert max(c["W"] for c in new) == 2047 and max(c["H"] for c in new) == 2016
    assert (4032 - 1) >> 11 == 1 and (252 - 1) >> 7 == 1 and (2047 - 1) >> 10 == 1      # the top bit of each 12-bit coordinate, of the 8-bit sample and of an 11-bit input coordinate
    for c in VR.CONV256_CASES[:-IC.CONV256_HIGH_BITS]:                    # what the older rows left untested
        assert c["Ho"] <= 16 and c["Wo"] <= 16 and c["B"] <= 4, c
    # every packed pixel of every new case survives the round trip through the 8 | 12 | 12 fields
    for c in new:
        for b, oy, ox in ((c["B"] - 1, c["Ho"] - 1, c["Wo"] - 1), (0, c["Ho"] - 1, 0), (c["B"] - 1, 0, c["Wo"] - 1)):
            assert IC.conv_unpack(IC.conv_pack(b, oy, ox)) == (b, oy, ox) and IC.conv_pack(b, oy, ox) < B32
    # the limits themselves: one past each is refused by the route's guard
    for c in IC.CONV256_OUTSIDE:
        assert not VR.conv_takes_256(c) and VR.conv_check(c, True) == VR.OK, c
        assert (c["B"] * c["Ho"] * c["Wo"]) % 256 == 0 and c["Cout"] % 256 == 0
    assert VR.conv_takes_256(dict(IC.CONV256_OUTSIDE[0], W=2016, Wo=4032)) and VR.conv_takes_256(dict(IC.CONV256_OUTSIDE[1], B=252))


@pytest.mark.parametrize("field,shape", [("ox", (1, 2, 4032)), ("oy", (1, 4032, 2)), ("ox", (1, 2, 2304)), ("b", (252, 2, 2))])
def test_conv_judge_rejects_a_truncated_coordinate_field(field, shape):
    """the convolution of the high-bit geometries at reduced channel counts (Cin 64, Cout 8, the other axis 2 pixels): an output whose packed
    field keeps only 11 bits (b: 3 of its 8) - every pixel beyond 2047 (sample 7) receives the pixel its truncated coordinate names - fails the
    sweep's bounds; so does the same truncation on the input side, modelled as the truth of the wrapped pixel"""
    B, Ho, Wo = shape
    c = dict(Ho=Ho, Wo=Wo, stride=1, pad_t=1, pad_l=1, up=1 if max(Ho, Wo) > 2304 else 0)
    H, W = (Ho >> c["up"], Wo >> c["up"])
    g = torch.Generator().manual_seed(77)
    x = VR.bf16(torch.randn(B, H, W, 64, generator=g, dtype=torch.float64))
    w = VR.bf16(torch.randn(8, 3, 3, 64, generator=g, dtype=torch.float64) / 24)
    bias = VR.bf16(torch.randn(8, generator=g, dtype=torch.float64))
    truth, var, border = VR.conv2d(x, w, bias, None, **c)
    b = VR.bounds(VR.conv_metrics(VR.bf16(var), truth, border), True)
    good = VR.conv_metrics(VR.bf16(var), truth, border)
    assert VR.excess(good, b) <= 1.0
    bad = IC.conv_coordinate_slip(VR.bf16(var), field, 3 if field == "b" else 11)
    changed = float((bad != VR.bf16(var)).any(-1).double().mean())
    assert changed > 0.4 if field != "ox" or Wo > 4000 else changed > 0.1, changed
    m = VR.conv_metrics(bad, truth, border)
    print(f"{field} truncated: {changed:.2f} of the pixels moved, excess {VR.excess(m, b):.1f}")
    assert VR.excess(m, b) > 10.0, (field, m, b)


def test_coordinate_slip_is_the_identity_below_the_old_sizes():
    """at the sizes of the older rows (Ho, Wo <= 16, B <= 4) the truncation changes nothing: they could not have seen it"""
    out = torch.randn(4, 16, 16, 8, generator=torch.Generator().manual_seed(1))
    for field, bits in (("ox", 11), ("oy", 11), ("b", 3), ("ox", 5), ("oy", 5)):
        assert torch.equal(IC.conv_coordinate_slip(out, field, bits), out)
    assert not torch.equal(IC.conv_coordinate_slip(out, "ox", 3), out) and not torch.equal(IC.conv_coordinate_slip(out, "b", 1), out)


# ----------------------------------------------------------------------------------------------------------------------------------
# the attention judge on a displaced batch: (b) of the far-view criterion cannot be met by garbage
# ----------------------------------------------------------------------------------------------------------------------------------
def test_attention_judge_rejects_a_batch_computed_on_another_batchs_keys():
    B, H, Lq, Lkv, dh = 2, 2, 64, 65, 64
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(B, H, L_, dh, generator=g).to(torch.bfloat16) for L_ in (Lq, Lkv, Lkv, Lq))
    ref = BR.attention(q, k, v, do, dh ** -0.5, lsum_bf16=True, fwd_tile=None)
    wrong = BR.attention(q, torch.stack([k[0], k[0]]), torch.stack([v[0], v[0]]), do, dh ** -0.5, lsum_bf16=True, fwd_tile=None)
    for n in ("O", "dq", "dk", "dv"):
        e_ok, e_bad = BR.err(ref[n + "_r"], ref[n], ref.get(n + "_m"))[0], BR.err(wrong[n + "_r"], ref[n], ref.get(n + "_m"))[0]
        assert e_bad > 100 * max(1.5 * e_ok, 2.0 ** -9), (n, e_ok, e_bad)


# ----------------------------------------------------------------------------------------------------------------------------------
# the GEMM far views
# ----------------------------------------------------------------------------------------------------------------------------------
GEMM_FAR = IC.gemm_far_cases()


@pytest.mark.parametrize("k", GEMM_FAR, ids=[k["name"].replace(" ", "_") for k in GEMM_FAR])
def test_gemm_far_cases_cross_the_boundaries_they_claim(k):
    from tests import fwd_ref as FR
    c, far = k["base"], k["far"]
    assert 300 <= c["M"] <= 520 and c["N"] == 520 and c["K"] <= 6144 and c["c_map"] == (0, 0) and c["c_shift"] == 0
    used = [op for op in IC.GEMM_OPERANDS if IC.gemm_operand_shape(far, op)[1] and not (op == "r" and (c["alias"] or c["epilogue"] not in (FR.EPI_RES_GATE, FR.EPI_RES_SCALE)))
            and not (op == "bias" and not c["has_bias"])]
    for op in used:
        assert IC.gemm_last_byte(c, op) < B31 // 64, (op, "the compact descriptor is not compact")
        assert (IC.gemm_last_byte(far, op) >= B32) == (op in k["crosses"]), (op, IC.gemm_last_byte(far, op))
        gstride, ldim = IC.gemm_operand_strides(far, op)
        assert gstride % 8 == 0 and ldim % 8 == 0
    assert set(k["crosses"]) <= set(used)
    # nothing overlaps: every operand's first group, row by row, as intervals of the arena
    lay = IC.gemm_far_layout(far)
    spans = []
    for op in used:
        G, rows, width = IC.gemm_operand_shape(far, op)
        gstride, ldim = IC.gemm_operand_strides(far, op)
        width += IC.SENT_COLS if op == "c" else 0
        assert 2 * lay[op] >= B31 and lay[op] % 8 == 0
        assert 2 * (lay[op] + (G - 1) * gstride + (rows - 1) * ldim + width) <= IC.GEMM_ARENA_BYTES
        if ldim < (1 << 20):
            spans.append((lay[op], lay[op] + (rows - 1) * ldim + width))
            assert G == 1 or spans[-1][1] - IC.ARENA_BASE < gstride
        else:
            spans += [(lay[op] + r * ldim, lay[op] + r * ldim + width) for r in range(rows)]
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "operands overlap in the arena"
    # the dispatch this case is there for, at the 256 CUs of the chip
    assert FR.gemm_path(far, 256) == c["path"] and FR.gemm_path(far, 256, force=128) == (128, 1, 1, 0, 0)
    assert (FR.gemm_path(far, 256)[2] > 1) == k["split"]
    if "w" in k["crosses"] and far["ldw"] > (1 << 20):
        assert FR.gemm_path(c, 256)[0] == 256 and FR.gemm_path(far, 256, force=256)[0] == 128, "the far ldw is what sends the case to the 128^2 kernel"


def test_gemm_far_cases_cover_every_operand_on_both_tiles():
    ks = GEMM_FAR
    assert set().union(*(k["crosses"] for k in ks)) == set(IC.GEMM_OPERANDS)
    assert any(k["base"]["alias"] and "c" in k["crosses"] for k in ks) and any(not k["base"]["alias"] and "r" in k["crosses"] for k in ks)
    assert sum(k["split"] for k in ks) == 1 and {k["base"]["path"][0] for k in ks} == {128, 256}
    assert any(k["far"]["ldc"] == IC.GEMM_LD_FAR for k in ks) and any(k["far"]["c_gstride"] == IC.GEMM_GS_FAR for k in ks)
    assert IC.GEMM_ARENA_BYTES + IC.GIB <= IC.MEMORY_CAP


# ----------------------------------------------------------------------------------------------------------------------------------
# AdaLN / glue far views and the large-canvas convolution windows
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IC.ADALN_FAR_CASES, ids=str)
def test_adaln_far_cases_cross_4_gib(case):
    from tests import fwd_ref as FR
    D, rows, rps, how = case
    geo = IC.adaln_far_geometry(case)
    phys = FR.rowmap(torch.arange(rows), *geo["x_map"])
    assert 2 * int(phys.max()) * geo["ldx"] >= B32 > 2 * int(phys.min()) * geo["ldx"] and 2 * (rows - 1) * geo["ldo"] >= B32
    assert geo["ldx"] % 8 == 0 and geo["ldo"] % 8 == 0 and rows % (geo["x_map"][0] or rows) == 0
    assert (how is None) == (geo["x_map"] == (0, 0)) and (how is None or geo["ldx"] == D + 8)
    assert 2 * (IC.ARENA_BASE + 200000 + max(int(phys.max()) * geo["ldx"], (rows - 1) * geo["ldo"]) + D + IC.SENT_COLS) <= 10 * IC.GIB
    assert {c[0] for c in IC.ADALN_FAR_CASES} == {1536, 3072, 520}            # both fast widths of the FLUX / SD3.5 models and a generic one


def test_glue_far_geometry_crosses_4_gib():
    for size, rows in IC.GLUE_FAR_ROWS.items():
        ld = IC.far_ld(rows, size)
        assert size * (rows - 1) * ld >= B32 > size * (rows - 1) * (ld - 8) and ld % 8 == 0
        assert (1 << 31) + size * (4096 + 3 * 1024 + (rows - 1) * ld + IC.GLUE_FAR_D + IC.SENT_COLS) <= 10 * IC.GIB


@pytest.mark.parametrize("c", IC.CONV_WINDOW_CASES, ids=lambda c: c["name"].split(",")[0].replace(" ", "_"))
def test_conv_window_cases_cross_the_boundaries_they_claim(c):
    es = 4 if c["f32"] else 2
    Ho, Wo = IC.conv_window_out(c)
    nx, no = c["H"] * c["W"] * c["Cin"] * es, Ho * Wo * c["Cout"] * es
    assert nx + no + 2 * Wo * c["Cout"] * es <= 10.8 * IC.GIB
    assert VR.conv_check(dict(c, B=1, Ho=Ho, Wo=Wo, KH=3, KW=3, pad_t=c["pad"], pad_l=c["pad"], up=0), not c["f32"]) == VR.OK
    assert not VR.conv_takes_256(dict(c, B=1, Ho=Ho, Wo=Wo, KH=3, KW=3, pad_t=c["pad"], pad_l=c["pad"], up=0))       # the 128^2 kernel's
    bd = IC.conv_boundaries(c)
    assert [b for b, _ in bd["x"]] == [b for b in (B31, B32) if b < nx] and [b for b, _ in bd["out"]] == [b for b in (B31, B32) if b < no]
    assert bd["x"] or bd["out"]
    wins = IC.conv_windows(c)
    assert wins[0][0] == 0 and wins[-1][1] == Ho and all(0 <= a < b <= Ho and b - a <= 4 for a, b in wins)
    covered = lambda y: any(a <= y < b for a, b in wins)
    for _, r in bd["out"]:                              # output rows on both sides of the boundary
        assert covered(r - 1) and covered(r), (r, wins)
    for _, r in bd["x"]:                                # some judged output row reads input rows on both sides of the boundary
        reads = [set(range(IC.conv_band(c, y, y + 1)["x0"], IC.conv_band(c, y, y + 1)["x1"])) for a, b in wins for y in range(a, b)]
        assert any(r - 1 in s and r in s for s in reads), (r, wins)
    # the bands tile the output, and each is a small problem
    BH = IC.CONV_BAND_ROWS
    for i in range(-(-Ho // BH)):
        bnd = IC.conv_band(c, i * BH, min((i + 1) * BH, Ho))
        assert bnd["H"] * c["W"] * c["Cin"] * es < B31 // 2 and bnd["Ho"] * Wo * c["Cout"] * es < B31 // 2
        assert 0 <= bnd["x0"] < bnd["x1"] <= c["H"] and bnd["pad_t"] == (c["pad"] if i == 0 else 0)
        assert VR.conv_check(dict(c, B=1, H=bnd["H"], Ho=bnd["Ho"], Wo=Wo, KH=3, KW=3, pad_t=bnd["pad_t"], pad_l=c["pad"], up=0), not c["f32"]) == VR.OK


def test_conv_window_cases_are_the_layers_of_the_issue():
    cs = IC.CONV_WINDOW_CASES
    assert [(c["Cin"], c["Cout"], c["stride"]) for c in cs if not c["f32"]] == [(64, 128, 1), (128, 128, 1), (128, 8, 1), (128, 128, 2)]
    assert sum(c["res"] == "alias" for c in cs) == 1 and sum(c["f32"] for c in cs) == 1
    twin = [c for c in cs if c["f32"]][0]
    assert twin["H"] * twin["W"] * twin["Cin"] * 4 > B32


@pytest.mark.parametrize("stride,pad", [(1, 1), (2, 0)])
def test_a_band_is_the_same_problem_as_its_rows_of_the_whole(stride, pad):
    """conv_band on the reference: rows [y0, y1) of the whole convolution equal the band evaluated on its own input rows - at the top, inside
    and at the bottom edge (what the band screen and the window truth both rely on)"""
    c = dict(H=24, W=10, Cin=64, Cout=8, stride=stride, pad=pad, f32=False)
    Ho, Wo = IC.conv_window_out(c)
    g = torch.Generator().manual_seed(3)
    x = VR.bf16(torch.randn(1, c["H"], c["W"], 64, generator=g, dtype=torch.float64))
    w = VR.bf16(torch.randn(8, 3, 3, 64, generator=g, dtype=torch.float64) / 24)
    whole = VR.conv2d(x, w, None, None, Ho=Ho, Wo=Wo, stride=stride, pad_t=pad, pad_l=pad, up=0)[0]
    for y0, y1 in ((0, 2), (3, 7), (Ho - 2, Ho), (0, Ho)):
        bnd = IC.conv_band(c, y0, y1)
        part = VR.conv2d(x[:, bnd["x0"]:bnd["x1"]], w, None, None, Ho=y1 - y0, Wo=Wo, stride=stride, pad_t=bnd["pad_t"], pad_l=pad, up=0)[0]
        assert torch.equal(part, whole[:, y0:y1]), (y0, y1, bnd)


def _row_slip(good, slip, sentinel=3.0):
    """good [rows, ...] at the ROW geometry of the 4104-row cases (one reduced row stands for one real row of 2^20 bytes = 2^19 elements: byte
    offset 2^31 is row 2048, 2^32 bytes = 2^31 elements row 4096) -> what a kernel leaves whose row offset is displaced past a boundary"""
    bad = good.clone()
    if slip == "read_2^31_bytes_early":                  # bit 31 of a byte offset lost: rows from 2048 on are computed from the input 2048 rows up
        bad[2048:4096] = good[:2048]
        bad[4096:] = good[4096:]
    elif slip == "read_2^32_bytes_early":                # the byte offset cut to 32 bits: rows from 4096 on are computed from rows 0 ...
        bad[4096:] = good[:good.shape[0] - 4096]
    elif slip == "write_2^31_elements_early":            # the element index cut to 31 bits on the store: rows 4096 ... land on rows 0 ..., theirs keep the sentinel
        bad[:good.shape[0] - 4096] = good[4096:]
        bad[4096:] = sentinel
    return bad


SLIPS = ["read_2^31_bytes_early", "read_2^32_bytes_early", "write_2^31_elements_early"]


@pytest.mark.parametrize("slip", SLIPS)
def test_conv_window_judge_rejects_a_displaced_row(slip):
    """the resnet case at its own 4104 rows, reduced in width and channels only (W 8, Cin 64, Cout 8), so the boundary rows and the case's own
    windows apply unchanged: with a displaced read or write some window of conv_windows fails the sweep's bounds by a factor above 10, and
    some band of the screen differs"""
    real = IC.CONV_WINDOW_CASES[1]
    c = dict(real, W=8, Cin=64, Cout=8)
    assert [r for _, r in IC.conv_boundaries(real)["out"]] == [2048, 4096] and real["W"] * real["Cout"] * 2 == 1 << 20
    g = torch.Generator().manual_seed(21)
    x = VR.bf16(torch.randn(1, c["H"], c["W"], 64, generator=g, dtype=torch.float64))
    w = VR.bf16(torch.randn(8, 3, 3, 64, generator=g, dtype=torch.float64) / 24)
    bias = VR.bf16(0.3 * torch.randn(8, generator=g, dtype=torch.float64))
    truth, var, border = VR.conv2d(x, w, bias, None, Ho=c["H"], Wo=c["W"], stride=1, pad_t=1, pad_l=1, up=0)
    good = VR.bf16(var)[0]
    bad = _row_slip(good, slip)
    worst_good = worst_bad = 0.0
    for y0, y1 in IC.conv_windows(real):
        t, b_ = truth[:, y0:y1], border[:, y0:y1]
        bd = VR.bounds(VR.conv_metrics(good[None, y0:y1], t, b_), True)
        worst_good = max(worst_good, VR.excess(VR.conv_metrics(good[None, y0:y1], t, b_), bd))
        worst_bad = max(worst_bad, VR.excess(VR.conv_metrics(bad[None, y0:y1], t, b_), bd))
    assert worst_good <= 1.0 and worst_bad > 10.0, (slip, worst_good, worst_bad)
    BH = IC.CONV_BAND_ROWS
    assert any(not torch.equal(bad[i:i + BH], good[i:i + BH]) for i in range(0, c["H"], BH))


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm past 2^32 bytes: the helpers against vae_kernel_ref, the tail, the slips
# ----------------------------------------------------------------------------------------------------------------------------------
def _gn_small(HW=1000, C=128, G=32, chunk=64, tail=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = -(-HW // chunk)
    x = torch.randn(HW, C, generator=g)
    x[(n - tail) * chunk:] += IC.GN_TAIL_SHIFT
    x = x.to(torch.bfloat16)
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).to(torch.bfloat16), (0.3 * torch.randn(C, generator=g)).to(torch.bfloat16)
    return x, gamma, beta, n


@pytest.mark.parametrize("C,G,silu", [(128, 32, True), (64, 32, False)])
def test_chunked_group_statistics_and_window_formula_are_vae_kernel_refs(C, G, silu):
    x, gamma, beta, n = _gn_small(C=C, G=G)
    mean, var = IC.group_stats_chunked(x, G, 64)
    m0, v0 = VR.group_stats(x.float()[None], G)
    assert float((mean - m0.flatten()).abs().max()) <= 1e-13 and float((var - v0.flatten()).abs().max()) <= 1e-12
    t0, r0 = VR.groupnorm(x.float()[None], gamma.float(), beta.float(), G, 1e-6, silu)
    t1, r1 = IC.groupnorm_with_stats(x[None], gamma, beta, G, 1e-6, silu, m0.flatten(), v0.flatten())
    assert torch.equal(t1, t0) and torch.equal(r1, r0)
    t2, r2 = IC.groupnorm_with_stats(x[None, 100:164], gamma, beta, G, 1e-6, silu, mean, var)       # a window, the chunked statistics
    assert float((t2 - t0[:, 100:164]).abs().max()) <= 1e-11 and float((r2 != r0[:, 100:164]).double().mean()) <= 1e-3


@pytest.mark.parametrize("how", ["tail_dropped", "tail_read_twice"])
def test_groupnorm_judge_needs_the_tail_of_the_tensor(how):
    """at a reduced size with the GPU test's construction (the last two chunks around mean 3): statistics without the tail chunks, or with them
    counted twice, give windows the GroupNorm sweep's bounds reject"""
    x, gamma, beta, n = _gn_small(HW=66 * 64)
    mean, var = IC.group_stats_chunked(x, 32, 64)
    ids = list(range(n - 2)) if how == "tail_dropped" else list(range(n)) + [n - 2, n - 1]
    wm, wv = IC.group_stats_chunked(x, 32, 64, chunks=ids)
    for r0, r1 in ((0, 64), (x.shape[0] - 64, x.shape[0])):
        truth, v = IC.groupnorm_with_stats(x[None, r0:r1], gamma, beta, 32, 1e-6, True, mean, var)
        wrong = IC.groupnorm_with_stats(x[None, r0:r1], gamma, beta, 32, 1e-6, True, wm, wv)[1]
        b = VR.bounds(VR.gn_metrics(v, truth, 32, 256), True)
        assert VR.excess(VR.gn_metrics(v, truth, 32, 256), b) <= 1.0 and VR.excess(VR.gn_metrics(wrong, truth, 32, 256), b) > 3.0, (how, r0)


@pytest.mark.parametrize("c", IC.GN_FAR_CASES, ids=lambda c: c["name"].replace(" ", "_"))
def test_groupnorm_cases_cross_the_boundaries_they_claim(c):
    assert c["HW"] * c["C"] >= B31 and 2 * c["HW"] * c["C"] > B32 and VR.gn_fast(c) == (c["C"] == 128)
    assert 2 * (2 * c["HW"] * c["C"] + 128 * c["C"]) <= 10.8 * IC.GIB
    wins = IC.gn_windows(c)
    assert wins[0][0] == 0 and wins[-1][1] == c["HW"] and len(wins) == 4
    for b in (B31, B32):
        r = b // (2 * c["C"])
        assert any(a <= r - 1 < e and a <= r < e for a, e in wins), (b, wins)
    n = -(-c["HW"] // IC.GN_CHUNK_ROWS)
    assert [IC.gn_chunk_mean(c, i) for i in (0, n - 3, n - 2, n - 1)] == [0.0, 0.0, IC.GN_TAIL_SHIFT, IC.GN_TAIL_SHIFT]
    assert (n - 1) * IC.GN_CHUNK_ROWS * 2 * c["C"] >= B32 > (n - 2) * IC.GN_CHUNK_ROWS * 2 * c["C"]    # the last chunk is all of the tensor past byte 2^32, the one before it ends there


@pytest.mark.parametrize("slip", SLIPS)
def test_groupnorm_window_judge_rejects_a_displaced_row(slip):
    """the fast case at its own row geometry scaled by 4096 (4104 rows of 128 channels; one row stands for 2^20 bytes): windows on either
    side of rows 2048 and 4096 and at both ends, as gn_windows places them; a displaced read or write fails the bounds in some window"""
    x, gamma, beta, _ = _gn_small(HW=4104, chunk=64)
    mean, var = IC.group_stats_chunked(x, 32, 64)
    truth, v = IC.groupnorm_with_stats(x[None], gamma, beta, 32, 1e-6, True, mean, var)
    real = IC.GN_FAR_CASES[0]
    assert [a // 4096 for a, _ in IC.gn_windows(real)[1:3]] == [2047, 4095] and 2 * real["C"] * 4096 == 1 << 20
    bad = _row_slip(v[0], slip)
    worst_good = worst_bad = 0.0
    for r0, r1 in ((0, 8), (2044, 2052), (4092, 4100), (4096, 4104)):
        b = VR.bounds(VR.gn_metrics(v[:, r0:r1], truth[:, r0:r1], 32, 256), True)
        worst_good = max(worst_good, VR.excess(VR.gn_metrics(v[:, r0:r1], truth[:, r0:r1], 32, 256), b))
        worst_bad = max(worst_bad, VR.excess(VR.gn_metrics(bad[None, r0:r1], truth[:, r0:r1], 32, 256), b))
    assert worst_good <= 1.0 and worst_bad > 10.0, (slip, worst_good, worst_bad)


# ----------------------------------------------------------------------------------------------------------------------------------
# the remaining far views
# ----------------------------------------------------------------------------------------------------------------------------------
def test_remaining_far_geometries_cross_4_gib():
    q = IC.QK_FAR
    B, L, W = q["batches"], q["rpb"], q["width"]
    for name, (ld, bsr) in IC.qk_far_geometries().items():
        assert 2 * ((B - 1) * bsr + L - 1) * ld >= B32 > 2 * (L - 1) * ld and ld % 8 == 0 and bsr >= L and ld >= W
        assert 2 * (IC.ARENA_BASE + ((B - 1) * bsr + L - 1) * ld + W) <= 10 * IC.GIB
    assert (IC.qk_far_geometries()["ld"][1], IC.qk_far_geometries()["batch_stride"][0]) == (L, W)
    M, N, K = IC.SMALL_LINEAR_FAR[:3]
    assert M == 48 and 2 * (M - 1) * IC.far_ld(M) >= B32 and 2 * (N - 1) * IC.far_ld(N) >= B32
    assert 2 * (IC.ARENA_BASE + (M - 1) * IC.far_ld(M) + 4096 + (N - 1) * IC.far_ld(N) + K) <= 10.8 * IC.GIB
    a = IC.ADALN_BWD_FAR
    rows, lds = a["rps"] * a["samples"], IC.far_ld(a["samples"])
    assert 2 * (rows - 1) * IC.far_ld(rows) >= B32 and 2 * (a["samples"] - 1) * lds >= B32
    assert 2 * (IC.ARENA_BASE + 16384 + (a["samples"] - 1) * lds + a["D"]) <= 10 * IC.GIB
    ld = IC.far_ld(rows)                                  # x, dy and the scale rows as the GPU test lays them out
    IC.assert_disjoint([(o + r * ld, o + r * ld + a["D"]) for o in (0, 2048) for r in range(rows)] +
                       [(16384 + s * lds, 16384 + s * lds + a["D"]) for s in range(a["samples"])])
