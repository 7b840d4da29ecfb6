"""The kernels of the low-precision AdamW step (csrc/optim.hip) as compiled, without a GPU (records from tests/code_object.py). The ceilings are
what the head commit compiles to with the flags of unigen_amd/build.py (hipcc 7.2.26015); compiler output is deterministic, so there is no margin,
as in tests/code_object_contracts.py. Both kernels are streaming kernels that want many waves per SIMD: at 128 registers or fewer four workgroups of
256 share a CU. The SGPR spills of adamw_lowp_kernel go to VGPR lanes (no memory traffic); what it may never do is spill VGPRs or use scratch - the
ten-round generator holds 20 words per 8 elements beside the 32 floats of the update."""
import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

CEILINGS = {
    "adamw_lowp_kernel": dict(vgpr_count=94, agpr_count=0, sgpr_spill_count=14, max_flat_workgroup_size=256),
    "sr_round_kernel": dict(vgpr_count=64, agpr_count=0, sgpr_spill_count=0, max_flat_workgroup_size=256),
}
LAUNCH_THREADS = 256


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_lowp_kernels_meet_their_contract(product, name):
    assert name in product, f"{name} is not in the product library"
    rec = product[name]
    assert CC.universal_violations(name, rec, {}) == [], rec          # wave64, static stack, no scratch, no VGPR spills
    assert rec["group_segment_fixed_size"] == 0, rec                  # no LDS: nothing is shared between lanes
    for f, c in CEILINGS[name].items():
        assert rec[f] <= c, (name, f, rec[f], c)
    assert rec["max_flat_workgroup_size"] == LAUNCH_THREADS and rec["vgpr_count"] <= 128, rec
    assert name not in CC.EXCEPTIONS and CC.template_name(name) not in {CC.template_name(n) for n in CC.HOT}
