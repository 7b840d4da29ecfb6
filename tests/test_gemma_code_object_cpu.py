"""The text-encoder kernels (csrc/text.hip; the fp32 attention twin in csrc/verify_f32.hip, the gather in csrc/elementwise.hip) without a GPU: the
kernels as compiled (through tests/code_object.py) and the refusals of the Gemma-2 C entry points (fake aligned pointers: every refusal comes before any
launch).

The register ceilings are what the commit that introduced each row compiled to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is
deterministic, so there is no margin, as in tests/code_object_contracts.py. The Gemma-2 rows are those of the kernels' first versions (attn_softcap_kernel,
attn_softcap_f32_kernel, gemma_norm_rows_kernel, gather_rows_scaled_kernel), the T5 / CLIP rows those of attn_bias_kernel and norm_rows_kernel<T, LN, REG>
before the two families became one template each. vgpr_count is the metadata's: it includes the AGPRs (the dh-256 attention runs one wave per SIMD - Q
fragments 64 registers, the O^T accumulator 128, S^T 16 - and so may use more than 256 registers per lane; what no kernel may do is spill). The attention
tiles are dynamic LDS (the launch's third argument), so group_segment_fixed_size is 0."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

_C = lambda v, a, s, lds, wg=256, sspill=0: dict(vgpr_count=v, agpr_count=a, sgpr_count=s, sgpr_spill_count=sspill, group_segment_fixed_size=lds,
                                                 max_flat_workgroup_size=wg)
CEILINGS = {
    # attn_plain_kernel<DH, KT, BIAS, CAUSAL, CAP, RAGGED>: Gemma-2 without and with the soft cap; T5 (table), CLIP (causal), both
    "attn_plain_kernel<256, 32, false, true, false, true>": _C(413, 157, 48, 0),
    "attn_plain_kernel<256, 32, false, true, true, true>": _C(425, 169, 49, 0),
    "attn_plain_kernel<64, 64, true, false, false, false>": _C(148, 32, 44, 0),
    "attn_plain_kernel<64, 64, false, true, false, false>": _C(148, 32, 40, 0),
    "attn_plain_kernel<64, 64, true, true, false, false>": _C(156, 32, 42, 0),
    # flash_attn_f32_kernel<DH, LPR, BIAS, RAGGED>: the Gemma-2 twin; the plain twins and the T5 / CLIP one (q in 17 / 33 KiB of static LDS, 64 threads);
    # the dh-512 twin has its row in tests/test_attn_wide_code_object_cpu.py and one here, so that every instantiation of a template is in one table
    "flash_attn_f32_kernel<256, 4, false, true>": _C(162, 0, 46, 0),
    "flash_attn_f32_kernel<64, 1, false, false>": _C(140, 0, 97, 17408, 64),
    "flash_attn_f32_kernel<128, 1, false, false>": _C(274, 18, 106, 33792, 64, 4),
    "flash_attn_f32_kernel<64, 1, true, false>": _C(140, 0, 102, 17408, 64),
    "flash_attn_f32_kernel<512, 16, false, false>": _C(100, 0, 39, 0),
    "rope_half_kernel<unsigned short>": _C(38, 0, 30, 0),
    "rope_half_kernel<float>": _C(46, 0, 30, 0),
    "norm_rows_kernel<unsigned short, NormGemma, true>": _C(112, 0, 34, 0),
    "norm_rows_kernel<unsigned short, NormGemma, false>": _C(39, 0, 26, 0),
    "norm_rows_kernel<float, NormGemma, true>": _C(114, 0, 34, 0),
    "norm_rows_kernel<float, NormGemma, false>": _C(34, 0, 26, 0),
    "norm_rows_kernel<unsigned short, NormT5, true>": _C(102, 0, 34, 0),
    "norm_rows_kernel<unsigned short, NormT5, false>": _C(27, 0, 24, 0),
    "norm_rows_kernel<float, NormT5, true>": _C(106, 0, 34, 0),
    "norm_rows_kernel<float, NormT5, false>": _C(28, 0, 24, 0),
    "norm_rows_kernel<unsigned short, NormLN, true>": _C(112, 0, 36, 0),
    "norm_rows_kernel<unsigned short, NormLN, false>": _C(38, 0, 28, 0),
    "norm_rows_kernel<float, NormLN, true>": _C(112, 0, 36, 0),
    "norm_rows_kernel<float, NormLN, false>": _C(44, 0, 28, 0),
    "gather_rows_kernel<unsigned short, true>": _C(20, 0, 44, 0),
    "gather_rows_kernel<float, true>": _C(26, 0, 46, 0),
    "gather_rows_kernel<unsigned short, false>": _C(20, 0, 42, 0, 1024),          # ug_gather_rows: no launch bound, as ever
    "gather_rows_kernel<float, false>": _C(24, 0, 42, 0, 1024),
}
# every launch of these kernels is dim3(256), but the fp32 attention twin's one lane per row (dim3(64)) and ug_gather_rows, which declares no bound
LAUNCH_THREADS = {n: c["max_flat_workgroup_size"] for n, c in CEILINGS.items()}


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_every_gemma_kernel_has_a_row(product):
    mine = {n for n in product if CC.template_name(n) in {CC.template_name(c) for c in CEILINGS}}
    assert mine == set(CEILINGS), mine ^ set(CEILINGS)


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_gemma_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS[name], rec
    assert name not in CC.EXCEPTIONS


def _attn(cdll, fn, **kw):
    """a valid (2 batches, 4 heads over 2, L = 40) call on a packed [q | k | v] buffer with fake aligned pointers, but for the fields in kw"""
    P, W = 4096, 8 * 256
    a = dict(q=P, q_rs=W, q_bs=40 * W, k=P + 2 * 4 * 256, k_rs=W, k_bs=40 * W, v=P + 2 * 6 * 256, v_rs=W, v_bs=40 * W, o=P, o_rs=4 * 256, o_bs=40 * 4 * 256,
             batches=2, heads=4, kv_heads=2, L=40, dh=256, scale=0.0625, cap=50.0, window=8, kv_len=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(a["q"], a["q_rs"], a["q_bs"], a["k"], a["k_rs"], a["k_bs"], a["v"], a["v_rs"], a["v_bs"], a["o"], a["o_rs"], a["o_bs"],
                           a["batches"], a["heads"], a["kv_heads"], a["L"], a["dh"], a["scale"], a["cap"], a["window"], a["kv_len"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_flash_attn_fwd_softcap", "ug_flash_attn_fwd_softcap_f32"])
def test_attn_softcap_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    f32 = fn.endswith("_f32")
    for dh in (64, 128, 512, 255):
        rc, msg = _attn(cdll, fn, dh=dh)
        assert rc == lib.UG_ERR_UNSUPPORTED and msg.startswith(fn.encode()) and b"256" in msg, (dh, rc, msg)
    for kw in (dict(heads=3), dict(kv_heads=3), dict(heads=2, kv_heads=4)):
        rc, msg = _attn(cdll, fn, **kw)
        assert rc == lib.UG_ERR_BAD_SHAPE and b"kv_heads" in msg, (kw, rc, msg)
    for kw in (dict(cap=-1.0), dict(cap=float("nan")), dict(cap=float("inf")), dict(window=-1)):
        assert _attn(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for name in ("q", "k", "v", "o"):                                    # misaligned bases (o: 8 bytes for bf16, 16 for fp32)
        assert _attn(cdll, fn, **{name: 4096 + 4})[0] == lib.UG_ERR_BAD_ALIGN, name
    assert _attn(cdll, fn, kv_len=4096 + 2)[0] == lib.UG_ERR_BAD_ALIGN
    bad = 2048 + 2 if f32 else 2048 + 4                                  # fp32: multiples of 4 elements; bf16: of 8 (o: of 4)
    for name in ("q_rs", "k_rs", "v_rs", "q_bs", "k_bs", "v_bs"):
        assert _attn(cdll, fn, **{name: bad})[0] == lib.UG_ERR_BAD_ALIGN, name
    for name in ("o_rs", "o_bs"):
        assert _attn(cdll, fn, **{name: 1024 + 2})[0] == lib.UG_ERR_BAD_ALIGN, name
    for kw in (dict(L=-1), dict(batches=-1), dict(heads=0), dict(kv_heads=0), dict(heads=-2), dict(q=None), dict(k=None), dict(v=None), dict(o=None)):
        assert _attn(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(L=0), dict(batches=0)):                              # nothing to do: no launch
        assert _attn(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _attn(cdll, fn, L=1 << 30)[0] == lib.UG_ERR_UNSUPPORTED
    assert _attn(cdll, fn, batches=1 << 28, heads=64, kv_heads=64)[0] == lib.UG_ERR_UNSUPPORTED          # the grid


def _rope(cdll, fn, **kw):
    P = 4096
    a = dict(buf=P, ld=1024, rows=48, rpb=24, col0=0, nheads=3, dh=256, cos=P, sin=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return getattr(cdll, fn)(a["buf"], a["ld"], a["rows"], a["rpb"], a["col0"], a["nheads"], a["dh"], a["cos"], a["sin"], None), cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_rope_half", "ug_rope_half_f32"])
def test_rope_half_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    for dh in (64, 128, 250):
        rc, msg = _rope(cdll, fn, dh=dh)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"256" in msg, (dh, rc, msg)
    for kw in (dict(buf=4096 + 8), dict(cos=4096 + 8), dict(sin=4096 + 8), dict(ld=1024 + 2), dict(col0=2, ld=1032)):
        assert _rope(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_ALIGN, kw
    for kw in (dict(rows=-1), dict(rpb=0), dict(nheads=-1), dict(col0=-8), dict(buf=None), dict(cos=None), dict(sin=None), dict(ld=512), dict(col0=512)):
        assert _rope(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(rows=0), dict(nheads=0)):
        assert _rope(cdll, fn, **kw)[0] == lib.UG_OK, kw


def _norm(cdll, fn, **kw):
    P = 4096
    a = dict(x=P, ldx=128, w=P, res=P, ldr=128, out=P, ldo=128, rows=5, D=128, eps=1e-6)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return getattr(cdll, fn)(a["x"], a["ldx"], a["w"], a["res"], a["ldr"], a["out"], a["ldo"], a["rows"], a["D"], a["eps"], None), cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_gemma_rmsnorm_rows", "ug_gemma_rmsnorm_rows_f32"])
def test_gemma_rmsnorm_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    for D in (4, 12, 100):
        rc, msg = _norm(cdll, fn, D=D)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"multiple of 8" in msg, (D, rc, msg)
    for kw in (dict(x=4096 + 8), dict(w=4096 + 8), dict(res=4096 + 8), dict(out=4096 + 8), dict(ldx=130), dict(ldo=130), dict(ldr=130)):
        assert _norm(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_ALIGN, kw
    for kw in (dict(rows=-1), dict(D=0), dict(D=-8), dict(x=None), dict(w=None), dict(out=None), dict(ldx=120), dict(ldo=120), dict(ldr=120)):
        assert _norm(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    assert _norm(cdll, fn, rows=0)[0] == lib.UG_OK
    assert _norm(cdll, fn, res=None, ldr=0, rows=0)[0] == lib.UG_OK


def _gather(cdll, fn, **kw):
    P = 4096
    a = dict(src=P, ld_src=128, idx=P, out=P, ld_out=128, n=5, W=128, scale=11.3125)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return getattr(cdll, fn)(a["src"], a["ld_src"], a["idx"], a["out"], a["ld_out"], a["n"], a["W"], a["scale"], None), cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_gather_rows_scaled", "ug_gather_rows_scaled_f32"])
def test_gather_rows_scaled_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    for kw in (dict(W=4, ld_src=128), dict(W=100), dict(src=4096 + 8), dict(out=4096 + 8), dict(idx=4096 + 2), dict(ld_src=130), dict(ld_out=130)):
        assert _gather(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_ALIGN, kw
    for kw in (dict(n=-1), dict(W=-8), dict(src=None), dict(idx=None), dict(out=None), dict(ld_src=120), dict(ld_out=120)):
        assert _gather(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(n=0), dict(W=0)):
        assert _gather(cdll, fn, **kw)[0] == lib.UG_OK, kw
