"""The ug_dpm_step kernels (csrc/sched.hip) as compiled, read through tests/code_object.py without a GPU: every DpmStep instantiation of
pointwise_kernel meets the universal contract (wave64, static stack, no scratch, no VGPR spills) and its register ceilings.

The ceilings are what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so there
is no margin, as in tests/test_dcae_code_object_cpu.py. The launch is dim3(256) under PwLoop::Chunks, whose kernels are bounded at 1024."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

_C = lambda v, s: dict(vgpr_count=v, agpr_count=0, sgpr_count=s, sgpr_spill_count=0, group_segment_fixed_size=0, max_flat_workgroup_size=1024)
_NAME = "pointwise_kernel<%s, DpmStep<%s, %d>, (PwLoop)1, 8, %s const*, %s const*, float, float*, float*, %s*, int, float, float, float, float, long>"
_name = lambda t, order: _NAME % (t, t, order, t, t, t)
CEILINGS = {
    _name("unsigned short", 1): _C(32, 42),
    _name("unsigned short", 2): _C(42, 42),
    _name("float", 1): _C(32, 52),
    _name("float", 2): _C(44, 54),
}
LAUNCH_THREADS = 256


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_every_dpm_step_kernel_has_a_row(product):
    mine = {n for n in product if "DpmStep" in n}
    assert mine == set(CEILINGS), mine ^ set(CEILINGS)


def test_dpm_step_template_is_in_no_other_table():
    assert "pointwise_kernel" not in {CC.template_name(n) for n in CC.HOT} and not [n for n in list(CC.HOT) + list(CC.EXCEPTIONS) if "DpmStep" in n]
    from tests import test_dcae_code_object_cpu as D
    assert not [n for n in D.CEILINGS if "DpmStep" in n]


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_dpm_step_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills, static LDS <= 64 KiB
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] >= LAUNCH_THREADS and rec["max_flat_workgroup_size"] == CEILINGS[name]["max_flat_workgroup_size"], rec
    assert name not in CC.EXCEPTIONS
