"""The Sana backward kernels (csrc/sana_bwd.hip) without a GPU: the kernels as compiled (through tests/code_object.py) and the refusals of their C
entry points (fake aligned pointers: every refusal comes before any launch), in the style of tests/test_sana_code_object_cpu.py.

The ceilings are what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so there is
no margin. vgpr_count is the metadata's: it includes the AGPRs (the fp32 twin of glu_bwd_dy_kernel holds both halves' 3 x 3 windows unpacked; what no
kernel may do is spill)."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

_C = lambda v, a, s, lds, wg: dict(vgpr_count=v, agpr_count=a, sgpr_count=s, sgpr_spill_count=0, group_segment_fixed_size=lds, max_flat_workgroup_size=wg)
CEILINGS = {
    "linattn_bwd_q_kernel<unsigned short>": _C(156, 0, 47, 49920, 256),
    "linattn_bwd_q_kernel<float>": _C(156, 0, 47, 49920, 256),
    "linattn_bwd_reduce_kernel": _C(8, 0, 20, 0, 256),
    "linattn_bwd_kv_kernel<unsigned short>": _C(114, 0, 45, 49664, 256),
    "linattn_bwd_kv_kernel<float>": _C(114, 0, 45, 49664, 256),
    "glu_bwd_dy_kernel<unsigned short>": _C(237, 0, 32, 0, 256),
    "glu_bwd_dy_kernel<float>": _C(316, 60, 36, 0, 256),
    "glu_bwd_dx_kernel<unsigned short>": _C(38, 0, 30, 0, 256),
    "glu_bwd_dx_kernel<float>": _C(43, 0, 30, 0, 256),
    "glu_bwd_dw_kernel<unsigned short>": _C(110, 0, 54, 0, 64),
    "glu_bwd_dw_kernel<float>": _C(117, 0, 61, 0, 64),
    "glu_bwd_reduce_kernel": _C(6, 0, 20, 0, 256),
}
# the launches of csrc/sana_bwd.hip: dim3(256) everywhere but the weight-gradient pass, one wave per workgroup
LAUNCH_THREADS = {n: (64 if n.startswith("glu_bwd_dw_kernel") else 256) for n in CEILINGS}
STATE = (32 * 32 + 32) * 4


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_every_sana_bwd_kernel_has_a_row(product):
    mine = {n for n in product if CC.template_name(n) in {CC.template_name(c) for c in CEILINGS}}
    assert mine == set(CEILINGS), mine ^ set(CEILINGS)
    # the new kernels have names of their own: no further instantiation of a forward template
    assert not any(CC.template_name(n) in ("linattn_state_kernel", "linattn_apply_kernel", "glu_dwconv3x3_kernel") for n in CEILINGS)


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_sana_bwd_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS[name], rec
    assert name not in CC.EXCEPTIONS


VIEWS = ("q", "k", "v", "do", "dq", "dk", "dv")


def _attn(cdll, fn, **kw):
    """a valid (2, 4, 64) call: packed [q | k | v] in, packed [dq | dk | dv] out, fake aligned pointers, but for the fields in kw"""
    P, D = 4096, 4 * 32
    a = dict(batches=2, heads=4, N=64, dh=32, state=P, ws=P, ws_bytes=2 * 4 * 2 * STATE)
    for n in VIEWS:
        w = D if n == "do" else 3 * D
        a[n], a[n + "_rs"], a[n + "_bs"] = P, w, 64 * w
    assert set(kw) <= set(a), kw
    a.update(kw)
    args = []
    for n in ("q", "k", "v", "do"):
        args += [a[n], a[n + "_rs"], a[n + "_bs"]]
    args.append(a["state"])
    for n in ("dq", "dk", "dv"):
        args += [a[n], a[n + "_rs"], a[n + "_bs"]]
    rc = getattr(cdll, fn)(*args, a["batches"], a["heads"], a["N"], a["dh"], a["ws"], a["ws_bytes"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_linear_attn_bwd", "ug_linear_attn_bwd_f32"])
def test_linear_attn_bwd_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    f32 = fn.endswith("_f32")
    for dh in (16, 64, 128, 33):
        rc, msg = _attn(cdll, fn, dh=dh)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"32" in msg, (dh, rc, msg)
    for name in VIEWS + ("state", "ws"):                                 # misaligned bases
        assert _attn(cdll, fn, **{name: 4096 + 8})[0] == lib.UG_ERR_BAD_ALIGN, name
    bad = 386 if f32 else 388                                            # fp32: multiples of 4 elements; bf16: of 8
    for name in VIEWS:
        for s in ("_rs", "_bs"):
            assert _attn(cdll, fn, **{name + s: bad})[0] == lib.UG_ERR_BAD_ALIGN, name + s
    rc, msg = _attn(cdll, fn, state=None)
    assert rc == lib.UG_ERR_BAD_SHAPE and b"state" in msg and b"required" in msg, (rc, msg)
    for kw in (dict(N=-1), dict(batches=-1), dict(heads=0), dict(heads=-2), dict(ws=None)) + tuple({n: None} for n in VIEWS):
        assert _attn(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw
    rc, msg = _attn(cdll, fn, ws_bytes=2 * 4 * 2 * STATE - 16)           # one alignment unit short
    assert rc == lib.UG_ERR_BAD_SHAPE and b"workspace" in msg, (rc, msg)
    for kw in (dict(N=0), dict(batches=0)):                              # nothing to do: no launch
        assert _attn(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _attn(cdll, fn, N=1 << 30, ws_bytes=1 << 62)[0] == lib.UG_ERR_UNSUPPORTED
    for kw in (dict(heads=4 * 65536), dict(batches=65536), dict(batches=65535, heads=40000)):
        assert _attn(cdll, fn, ws_bytes=1 << 62, **kw)[0] == lib.UG_ERR_UNSUPPORTED, kw


def test_linear_attn_bwd_workspace_bytes():
    from unigen_amd import lib
    cdll = lib.load()
    q = cdll.ug_linear_attn_bwd_workspace_bytes
    assert q(1, 1, 1) == 2 * STATE                                        # dS | dz and one partial per 128 query rows
    assert q(1, 1, 128) == 2 * STATE and q(1, 1, 129) == 3 * STATE
    assert q(2, 8, 1024) == 2 * 8 * (8 + 1) * STATE
    assert q(1, 70, 4097) == 70 * (33 + 1) * STATE
    assert q(0, 4, 64) == q(2, 4, 0) == q(2, 0, 64) == 0
    assert q(2, 4, 64) % 16 == 0


def _glu_ws(B, H, W, C, elem):
    pixels = B * H * W
    return (pixels * 2 * C * elem + 15) // 16 * 16 + (pixels + 255) // 256 * 10 * 2 * C * 4


def _glu(cdll, fn, **kw):
    """a valid (2, 5, 7, 40) call with fake aligned pointers, but for the fields in kw"""
    P = 4096
    a = dict(x=P, ldx=80, w9=P, bias=P, dout=P, lddo=40, dx=P, lddx=80, dw9=P, dbias=P, B=2, H=5, W=7, C=40, ws=P,
             ws_bytes=_glu_ws(2, 5, 7, 40, 4 if fn.endswith("_f32") else 2))
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(a["x"], a["ldx"], a["w9"], a["bias"], a["dout"], a["lddo"], a["dx"], a["lddx"], a["dw9"], a["dbias"], a["B"], a["H"], a["W"], a["C"],
                           a["ws"], a["ws_bytes"], None)
    return rc, cdll.ug_last_error()


@pytest.mark.parametrize("fn", ["ug_glu_dwconv3x3_bwd", "ug_glu_dwconv3x3_bwd_f32"])
def test_glu_dwconv_bwd_abi_rejections(fn):
    from unigen_amd import lib
    cdll = lib.load()
    big = 1 << 62
    for C in (4, 12, 36):
        rc, msg = _glu(cdll, fn, C=C, ws_bytes=big)
        assert rc == lib.UG_ERR_UNSUPPORTED and b"multiple of 8" in msg, (C, rc, msg)
    for name in ("x", "w9", "bias", "dout", "dx", "dw9", "dbias", "ws"):
        assert _glu(cdll, fn, **{name: 4096 + 8})[0] == lib.UG_ERR_BAD_ALIGN, name
    for kw in (dict(ldx=84), dict(lddo=44), dict(lddx=84)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_ALIGN, kw
    for kw in (dict(B=-1), dict(H=-1), dict(W=-2), dict(C=0), dict(C=-8), dict(ldx=72), dict(lddo=32), dict(lddx=72), dict(x=None), dict(w9=None),
               dict(bias=None), dict(dout=None), dict(dx=None), dict(ws=None), dict(dw9=None), dict(dbias=None)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_ERR_BAD_SHAPE, kw      # (one of dw9 / dbias alone is refused; both NULL is the frozen form)
    rc, msg = _glu(cdll, fn, ws_bytes=_glu_ws(2, 5, 7, 40, 4 if fn.endswith("_f32") else 2) - 16)
    assert rc == lib.UG_ERR_BAD_SHAPE and b"workspace" in msg, (rc, msg)
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert _glu(cdll, fn, **kw)[0] == lib.UG_OK, kw
    assert _glu(cdll, fn, B=65536, ws_bytes=big)[0] == lib.UG_ERR_UNSUPPORTED


def test_glu_dwconv_bwd_workspace_bytes():
    from unigen_amd import lib
    cdll = lib.load()
    q = cdll.ug_glu_dwconv3x3_bwd_workspace_bytes
    for shape in ((1, 1, 1, 8), (2, 5, 7, 40), (1, 17, 33, 8), (1, 64, 64, 5600)):
        for elem in (2, 4):
            assert q(*shape, elem) == _glu_ws(*shape, elem) and q(*shape, elem) % 16 == 0, (shape, elem)
    assert q(1, 16, 16, 8, 4) - q(1, 16, 16, 8, 2) == 256 * 16 * 2       # dy is kept as T; the partials are fp32 either way
    assert q(0, 5, 7, 40, 2) == q(2, 5, 7, 0, 2) == q(2, 5, 7, 40, 3) == 0
