"""The DC-AE kernels (csrc/dcae.hip) without a GPU: the kernels as compiled (through tests/code_object.py) and the refusals of their C entry points
(fake aligned pointers: every refusal comes before any launch).

The register ceilings are what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so
there is no margin, as in tests/code_object_contracts.py. vgpr_count is the metadata's: it includes the AGPRs (the MFMA accumulator of the
multiscale projection). The 5 x 5 projection stays at or below 256 registers: two workgroups of one wave per SIMD fit a CU, which its LDS allows too."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

_C = lambda v, a, s, lds, wg: dict(vgpr_count=v, agpr_count=a, sgpr_count=s, sgpr_spill_count=0, group_segment_fixed_size=lds, max_flat_workgroup_size=wg)
_SILU = "pointwise_kernel<%s, PwMap<%s, Silu<%s> >, (PwLoop)0, 8, %s const*, %s*, long>"
CEILINGS = {
    "rmsnorm_bias_rows_kernel<unsigned short>": _C(104, 0, 42, 0, 256),
    "rmsnorm_bias_rows_kernel<float>": _C(114, 0, 42, 0, 256),
    "msconv_proj_kernel<unsigned short, 4, 5>": _C(244, 16, 48, 61696, 256),
    "msconv_proj_kernel<unsigned short, 4, 3>": _C(132, 16, 48, 37120, 256),
    "msconv_proj_kernel<float, 2, 5>": _C(256, 16, 48, 61696, 128),
    "msconv_proj_kernel<float, 2, 3>": _C(192, 16, 48, 37120, 128),
    "dc_shortcut_kernel<unsigned short, 1, false>": _C(26, 0, 30, 0, 256),
    "dc_shortcut_kernel<unsigned short, 1, true>": _C(30, 0, 32, 0, 256),
    "dc_shortcut_kernel<unsigned short, 2, false>": _C(24, 0, 31, 0, 256),
    "dc_shortcut_kernel<unsigned short, 2, true>": _C(32, 0, 31, 0, 256),
    "dc_shortcut_kernel<float, 1, false>": _C(26, 0, 30, 0, 256),
    "dc_shortcut_kernel<float, 1, true>": _C(30, 0, 32, 0, 256),
    "dc_shortcut_kernel<float, 2, false>": _C(28, 0, 31, 0, 256),
    "dc_shortcut_kernel<float, 2, true>": _C(36, 0, 31, 0, 256),
    _SILU % (("unsigned short",) * 5): _C(18, 0, 12, 0, 256),
    _SILU % (("float",) * 5): _C(34, 0, 17, 0, 256),
}
# the launches of csrc/dcae.hip: dim3(256) everywhere but the projection's fp32 twin, dim3(64 * NG) = 64 x 2
LAUNCH_THREADS = {n: (128 if n.startswith("msconv_proj_kernel<float") else 256) for n in CEILINGS}
OWN_TEMPLATES = ("rmsnorm_bias_rows_kernel", "msconv_proj_kernel", "dc_shortcut_kernel")


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_every_dcae_kernel_has_a_row(product):
    mine = {n for n in product if CC.template_name(n) in OWN_TEMPLATES or "Silu<" in n}
    assert mine == set(CEILINGS), mine ^ set(CEILINGS)


def test_dcae_templates_are_in_no_other_table():
    assert not {CC.template_name(n) for n in CC.HOT} & set(OWN_TEMPLATES + ("pointwise_kernel",))


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_dcae_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS[name], rec
    assert name not in CC.EXCEPTIONS


P = 1 << 20                # a fake device address, 4096-byte aligned
TWINS = lambda base: [base, base + "_f32"]


def _call(fn, valid, order, **kw):
    from unigen_amd import lib
    cdll = lib.load()
    a = dict(valid)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(*[a[n] for n in order], None)
    return rc, cdll.ug_last_error().decode()


def _refused(fn, valid, order, code, **kw):
    rc, msg = _call(fn, valid, order, **kw)
    assert rc == code and msg.split(":")[0] == fn, (fn, kw, rc, msg)
    return msg


NORM = dict(x=P, ldx=48, w=2 * P, bias=3 * P, residual=4 * P, ldr=40, out=5 * P, ldo=56, rows=5, C=40, eps=1e-5, act=0)
NORM_ORDER = ("x", "ldx", "w", "bias", "residual", "ldr", "out", "ldo", "rows", "C", "eps", "act")


@pytest.mark.parametrize("fn", TWINS("ug_rmsnorm_bias_rows"))
def test_rmsnorm_bias_rows_refusals(fn):
    from unigen_amd import lib
    f32 = fn.endswith("_f32")
    for kw in (dict(x=None), dict(w=None), dict(bias=None), dict(out=None), dict(rows=-1), dict(C=0), dict(C=-8), dict(act=2), dict(ldx=32), dict(ldo=32),
               dict(ldr=32)):
        _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_BAD_SHAPE, **kw)
    for C in (4, 12, 36, 4616):
        assert "multiple of 8" in _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_UNSUPPORTED, C=C, ldx=8192, ldo=8192, ldr=8192)
    _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_UNSUPPORTED, act=1)              # with the residual
    for name in ("x", "w", "bias", "residual", "out"):
        _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_BAD_ALIGN, **{name: NORM[name] + 8})
    bad = 50 if f32 else 52
    for name in ("ldx", "ldo", "ldr"):
        _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_BAD_ALIGN, **{name: bad})
    _refused(fn, NORM, NORM_ORDER, lib.UG_ERR_UNSUPPORTED, rows=1 << 40)       # 2^31 workgroups or more at any number of rows per workgroup (4 .. 256)
    assert _call(fn, NORM, NORM_ORDER, rows=0)[0] == lib.UG_OK
    assert _call(fn, NORM, NORM_ORDER, rows=0, x=None)[0] == lib.UG_OK


def test_valid_descriptors_pass_every_check_but_the_launch():
    """the VALID tables are valid: with one count set to zero each entry returns UG_OK (no launch), and nothing above relies on a typo"""
    from unigen_amd import lib
    for fn, valid, order, zero in (("ug_rmsnorm_bias_rows", NORM, NORM_ORDER, "rows"), ("ug_msconv_proj", MS, MS_ORDER, "B"),
                                   ("ug_dc_shortcut_down", DOWN, SC_ORDER, "H"), ("ug_dc_shortcut_up", UP, SC_ORDER, "W"), ("ug_silu", SILU, SILU_ORDER, "n")):
        for f in TWINS(fn):
            assert _call(f, valid, order, **{zero: 0})[0] == lib.UG_OK, f


MS = dict(x=P, ldx=192, w_dw=2 * P, w_pw=3 * P, out=4 * P, ldo=200, B=2, H=5, W=7, G=6, k=5)
MS_ORDER = ("x", "ldx", "w_dw", "w_pw", "out", "ldo", "B", "H", "W", "G", "k")


@pytest.mark.parametrize("fn", TWINS("ug_msconv_proj"))
def test_msconv_proj_refusals(fn):
    from unigen_amd import lib
    for kw in (dict(x=None), dict(w_dw=None), dict(w_pw=None), dict(out=None), dict(B=-1), dict(H=-1), dict(W=-2), dict(G=0), dict(G=-3), dict(ldx=184),
               dict(ldo=184)):
        _refused(fn, MS, MS_ORDER, lib.UG_ERR_BAD_SHAPE, **kw)
    for k in (1, 2, 4, 7, 9, 0, -5):
        assert "kernel size" in _refused(fn, MS, MS_ORDER, lib.UG_ERR_UNSUPPORTED, k=k)
    for name in ("x", "w_dw", "w_pw", "out"):
        _refused(fn, MS, MS_ORDER, lib.UG_ERR_BAD_ALIGN, **{name: MS[name] + 8})
    for kw in (dict(ldx=196), dict(ldo=204)):
        _refused(fn, MS, MS_ORDER, lib.UG_ERR_BAD_ALIGN, **kw)
    for kw in (dict(B=65536), dict(H=1 << 20), dict(W=1 << 20), dict(ldx=1 << 24), dict(ldo=1 << 24)):
        _refused(fn, MS, MS_ORDER, lib.UG_ERR_UNSUPPORTED, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert _call(fn, MS, MS_ORDER, **kw)[0] == lib.UG_OK, kw
    assert _call(fn, MS, MS_ORDER, k=3, B=0)[0] == lib.UG_OK


DOWN = dict(h=P, ldh=16, x=2 * P, ldx=16, x_shuffle=0, out=3 * P, ldo=24, B=2, H=4, W=6, Cin=16, Cout=16, factor=2)
UP = dict(h=P, ldh=32, x=2 * P, ldx=8, x_shuffle=0, out=3 * P, ldo=16, B=2, H=3, W=5, Cin=32, Cout=8, factor=2)
SC_ORDER = ("h", "ldh", "x", "ldx", "x_shuffle", "out", "ldo", "B", "H", "W", "Cin", "Cout", "factor")


@pytest.mark.parametrize("fn", TWINS("ug_dc_shortcut_down") + TWINS("ug_dc_shortcut_up"))
def test_dc_shortcut_refusals(fn):
    from unigen_amd import lib
    up = "_up" in fn
    V = UP if up else DOWN
    f32 = fn.endswith("_f32")
    for kw in (dict(h=None), dict(out=None), dict(B=-1), dict(H=-1), dict(W=-1), dict(Cin=0), dict(Cout=-8), dict(x_shuffle=2), dict(ldh=8), dict(ldo=0),
               dict(ldx=0)):
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, **kw)
    for f in (0, 3, 4, -1):
        assert "factor" in _refused(fn, V, SC_ORDER, lib.UG_ERR_UNSUPPORTED, factor=f)
    for kw in (dict(Cin=12, ldh=64), dict(Cout=20, ldo=64, ldx=64)):
        assert "multiples of 8" in _refused(fn, V, SC_ORDER, lib.UG_ERR_UNSUPPORTED, **kw)
    # g resp. r must be a positive integer
    if up:
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, Cin=24)                       # 8 x 4 / 24
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, Cin=64, ldh=64)               # r = 1 / 2
    else:
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, Cout=24, ldo=24, ldx=24)      # 16 x 4 / 24
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, Cout=128, ldo=128, ldx=128)   # g = 1 / 2
        assert "factor" in _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, H=5)
        assert "factor" in _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, W=7)
    # the row of an x still to be rearranged: Cout f^2 (up) resp. Cout / f^2 (down) channels
    _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_SHAPE, x_shuffle=1, ldx=24 if up else 0)
    assert _call(fn, V, SC_ORDER, x_shuffle=1, ldx=32 if up else 8, B=0)[0] == lib.UG_OK
    for name in ("h", "x", "out"):
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_ALIGN, **{name: V[name] + 8})
    bad = 34 if f32 else 36
    for name in ("ldh", "ldx", "ldo"):
        _refused(fn, V, SC_ORDER, lib.UG_ERR_BAD_ALIGN, **{name: bad})
    for kw in (dict(B=65536), dict(H=1 << 20), dict(W=1 << 20), dict(ldh=1 << 24)):
        _refused(fn, V, SC_ORDER, lib.UG_ERR_UNSUPPORTED, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert _call(fn, V, SC_ORDER, **kw)[0] == lib.UG_OK, kw
    assert _call(fn, V, SC_ORDER, x=None, ldx=0, B=0)[0] == lib.UG_OK


SILU = dict(x=P, y=2 * P, n=64)
SILU_ORDER = ("x", "y", "n")


@pytest.mark.parametrize("fn", TWINS("ug_silu"))
def test_silu_refusals(fn):
    from unigen_amd import lib
    for kw in (dict(x=None), dict(y=None), dict(n=-8)):
        _refused(fn, SILU, SILU_ORDER, lib.UG_ERR_BAD_SHAPE, **kw)
    for n in (12, 1001):
        assert "multiple of 8" in _refused(fn, SILU, SILU_ORDER, lib.UG_ERR_UNSUPPORTED, n=n)
    _refused(fn, SILU, SILU_ORDER, lib.UG_ERR_UNSUPPORTED, n=8 * 256 << 31)
    for kw in (dict(x=P + 8), dict(y=2 * P + 4)):
        _refused(fn, SILU, SILU_ORDER, lib.UG_ERR_BAD_ALIGN, **kw)
    assert _call(fn, SILU, SILU_ORDER, n=0)[0] == lib.UG_OK
