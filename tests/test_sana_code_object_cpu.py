"""The Sana kernels (csrc/sana.hip) without a GPU: the kernels as compiled (through tests/code_object.py) and the refusals of their C entry points
(fake aligned pointers: every refusal comes before any launch).

The register ceilings are what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so
there is no margin, as in tests/code_object_contracts.py. vgpr_count is the metadata's: it includes the AGPRs (the fp32 twin of the convolution runs
128 threads per workgroup and so may use more than 256 registers per lane; what no kernel may do is spill)."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

_C = lambda v, a, s, lds, wg: dict(vgpr_count=v, agpr_count=a, sgpr_count=s, sgpr_spill_count=0, group_segment_fixed_size=lds, max_flat_workgroup_size=wg)
CEILINGS = {
    "linattn_state_kernel<unsigned short>": _C(79, 0, 42, 40960, 256),
    "linattn_state_kernel<float>": _C(79, 0, 42, 40960, 256),
    "linattn_reduce_kernel": _C(8, 0, 21, 0, 256),
    "linattn_apply_kernel<unsigned short>": _C(72, 0, 33, 25088, 256),
    "linattn_apply_kernel<float>": _C(72, 0, 33, 25088, 256),
    "glu_dwconv3x3_kernel<unsigned short, 8>": _C(210, 0, 50, 37376, 256),
    "glu_dwconv3x3_kernel<float, 4>": _C(290, 34, 53, 37376, 128),
}
# the launches of csrc/sana.hip: dim3(256) everywhere but the convolution's fp32 twin, dim3(GT_W * OCT) = 32 x 4
LAUNCH_THREADS = {n: (128 if n == "glu_dwconv3x3_kernel<float, 4>" else 256) for n in CEILINGS}


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_every_sana_kernel_has_a_row(product):
    mine = {n for n in product if CC.template_name(n) in {CC.template_name(c) for c in CEILINGS}}
    assert mine == set(CEILINGS), mine ^ set(CEILINGS)


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_sana_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS[name], rec
    assert name not in CC.EXCEPTIONS


def _attn(cdll, fn, **kw):
    """a valid (2, 4, 64) call on a packed [q | k | v] buffer with fake aligned pointers, but for the fields in kw"""
    P, D = 4096, 4 * 32
    a = dict(q=P, q_rs=3 * D, q_bs=64 * 3 * D, k=P + 2 * D, k_rs=3 * D, k_bs=64 * 3 * D, v=P + 4 * D, v_rs=3 * D, v_bs=64 * 3 * D, o=P, o_rs=D, o_bs=64 * D,
             batches=2, heads=4, N=64, dh=32, ws=P)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(a["q"], a["q_rs"], a["q_bs"], a["k"], a["k_rs"], a["k_bs"], a["v"], a["v_rs"], a["v_bs"], a["o"], a["o_rs"], a["o_bs"],
                           a["batches"], a["heads"], a["N"], a["dh"], a["ws"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_linear_attn", "ug_linear_attn_f32"])
def test_linear_attn_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    f32 = fn.endswith("_f32")
    for dh in (16, 64, 128, 33):
        rc, msg = _attn(cdll, fn, dh=dh)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"32" in msg, (dh, rc, msg)
    for name in ("q", "k", "v", "o", "ws"):                              # misaligned bases
        assert _attn(cdll, fn, **{name: 4096 + 8})[0] == lib.UG_ERR_BAD_ALIGN, name
    bad = 386 if f32 else 388                                            # fp32: multiples of 4 elements; bf16: of 8
    for name in ("q_rs", "k_rs", "v_rs", "o_rs", "q_bs", "k_bs", "v_bs", "o_bs"):
        assert _attn(cdll, fn, **{name: bad})[0] == lib.UG_ERR_BAD_ALIGN, name
    for kw in (dict(N=-1), dict(batches=-1), dict(heads=0), dict(heads=-2), dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(ws=None)):
        assert _attn(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(N=0), dict(batches=0)):                              # nothing to do: no launch
        assert _attn(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _attn(cdll, fn, N=1 << 30)[0] == lib.UG_ERR_UNSUPPORTED
    # the grid: head groups of 4 on y and batches on z stay below 65536, batches x heads (the reduce pass's x) below 2^31
    for kw in (dict(heads=4 * 65536), dict(batches=65536), dict(batches=65535, heads=40000)):
        assert _attn(cdll, fn, **kw)[0] == lib.UG_ERR_UNSUPPORTED, kw


def test_linear_attn_workspace_bytes():
    from unigen_amd import lib
    cdll = lib.load()
    state = (32 * 32 + 32) * 4
    assert cdll.ug_linear_attn_workspace_bytes(1, 1, 1) == 2 * state                     # the state and one chunk's partial
    assert cdll.ug_linear_attn_workspace_bytes(2, 8, 1024) == 2 * 8 * (4 + 1) * state
    assert cdll.ug_linear_attn_workspace_bytes(1, 70, 4097) == 70 * (17 + 1) * state
    assert cdll.ug_linear_attn_workspace_bytes(0, 4, 64) == cdll.ug_linear_attn_workspace_bytes(2, 4, 0) == 0


def _glu(cdll, fn, **kw):
    """a valid (2, 5, 7, 40) call with fake aligned pointers, but for the fields in kw"""
    P = 4096
    a = dict(x=P, ldx=80, w9=P, bias=P, out=P, ldo=40, B=2, H=5, W=7, C=40)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(a["x"], a["ldx"], a["w9"], a["bias"], a["out"], a["ldo"], a["B"], a["H"], a["W"], a["C"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_glu_dwconv3x3", "ug_glu_dwconv3x3_f32"])
def test_glu_dwconv_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    for C in (4, 12, 36):
        rc, msg = _glu(cdll, fn, C=C)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"multiple of 8" in msg, (C, rc, msg)
    for name in ("x", "w9", "bias", "out"):
        assert _glu(cdll, fn, **{name: 4096 + 8})[0] == lib.UG_ERR_BAD_ALIGN, name
    for kw in (dict(ldx=84), dict(ldo=44)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_ALIGN, kw
    for kw in (dict(B=-1), dict(H=-1), dict(W=-2), dict(C=0), dict(C=-8), dict(ldx=72), dict(ldo=32), dict(x=None), dict(w9=None), dict(bias=None), dict(out=None)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _glu(cdll, fn, B=65536)[0] == lib.UG_ERR_UNSUPPORTED
