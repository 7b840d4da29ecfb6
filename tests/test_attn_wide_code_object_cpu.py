"""The head-width-512 flash attention forward (csrc/attn_wide.hip) without a GPU: the bf16 kernel and its fp32 twin (verify_f32.hip's one kernel at 16 lanes per row) as compiled (through tests/code_object.py) and the
refusals of their C entry points (fake aligned pointers: every refusal comes before any launch).

The register ceilings are what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so
there is no margin, as in tests/code_object_contracts.py. flash_attn_wide_kernel is one wave per SIMD on the whole unified file: 256 accumulator
registers (O^T) + 256 VGPRs (128 of them the Q fragments); what it may never do is spill (the universal contract)."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

# vgpr_count is the metadata's: it includes the AGPRs (unified file)
CEILINGS = {
    "flash_attn_wide_kernel": dict(vgpr_count=512, agpr_count=256, sgpr_count=46, sgpr_spill_count=0, max_flat_workgroup_size=256),
    "flash_attn_f32_kernel<512, 16, false, false>": dict(vgpr_count=100, agpr_count=0, sgpr_count=39, sgpr_spill_count=0, max_flat_workgroup_size=256),
}
LAUNCH_THREADS = 256          # both launches: dim3(256)


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_wide_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    assert rec["group_segment_fixed_size"] == 0, rec                  # the bf16 kernel's 128 KiB are dynamic LDS; the twin uses none
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS, rec
    assert name not in CC.EXCEPTIONS


def test_wide_kernel_keeps_its_accumulator_in_the_agpr_half(product):
    rec = product["flash_attn_wide_kernel"]
    assert rec["agpr_count"] == 256 and rec["vgpr_count"] - rec["agpr_count"] <= 256, rec


def _call(cdll, fn, **kw):
    """a valid (1, 1, 64, 64, 512) call with fake aligned pointers, but for the fields in kw"""
    P = 4096
    a = dict(q=P, q_rs=512, q_bs=64 * 512, k=P, k_rs=512, k_bs=64 * 512, v=P, v_rs=512, v_bs=64 * 512, o=P, o_rs=512, o_bs=64 * 512,
             batches=1, heads=1, Lq=64, Lkv=64, dh=512, scale=512 ** -0.5)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(a["q"], a["q_rs"], a["q_bs"], a["k"], a["k_rs"], a["k_bs"], a["v"], a["v_rs"], a["v_bs"], a["o"], a["o_rs"], a["o_bs"],
                           a["batches"], a["heads"], a["Lq"], a["Lkv"], a["dh"], a["scale"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_flash_attn_fwd_wide", "ug_flash_attn_fwd_wide_f32"])
def test_wide_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    f32 = fn.endswith("_f32")
    for dh in (64, 128, 256, 500):
        rc, msg = _call(cdll, fn, dh=dh)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"512" in msg, (dh, rc, msg)
    for name in ("q", "k", "v", "o"):                                     # misaligned bases
        assert _call(cdll, fn, **{name: 4096 + (4 if f32 or name != "o" else 2)})[0] == lib.UG_ERR_BAD_ALIGN, name
    bad_stride = 514 if f32 else 516                                      # fp32: multiples of 4 elements; bf16: of 8 (o: of 4)
    for name in ("q_rs", "k_rs", "v_rs", "q_bs", "k_bs", "v_bs"):
        assert _call(cdll, fn, **{name: bad_stride})[0] == lib.UG_ERR_BAD_ALIGN, name
    for name in ("o_rs", "o_bs"):
        assert _call(cdll, fn, **{name: 514})[0] == lib.UG_ERR_BAD_ALIGN, name
    for kw in (dict(Lkv=0), dict(Lkv=-1), dict(Lq=-1), dict(batches=-1), dict(heads=0), dict(heads=-2), dict(q=None), dict(o=None)):
        assert _call(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(Lq=0), dict(batches=0)):                              # nothing to do: no launch, as ug_flash_attn_fwd
        assert _call(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _call(cdll, fn, Lq=1 << 30)[0] == lib.UG_ERR_UNSUPPORTED
    if not f32:
        assert _call(cdll, fn, k_rs=1 << 24)[0] == lib.UG_ERR_UNSUPPORTED and _call(cdll, fn, v_rs=-512)[0] == lib.UG_ERR_UNSUPPORTED
        assert _call(cdll, fn, scale=0.0)[0] == lib.UG_ERR_UNSUPPORTED


def test_narrow_forward_still_refuses_the_wide_head():
    from unigen_amd import lib
    cdll = lib.load()
    for fn in ("ug_flash_attn_fwd", "ug_flash_attn_fwd_f32"):
        assert _call(cdll, fn, dh=512)[0] == lib.UG_ERR_UNSUPPORTED, fn
