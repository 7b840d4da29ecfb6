"""What ug_gemm_plan says is what ug_gemm_bf16 runs, on the device's own CU count: the planner against fwd_ref.gemm_path for every case of the
tables (tests/test_gemm_plan_cpu.py::table_cases), then three GEMM_CASES launched at their table sizes - the smallest split-K case, the smallest
unsplit 256^2 case, one 128^2 case - on a poisoned workspace. The one effect that differs by path ties "planned" to "ran"
(tests/test_workspace_gpu.py states the contract): a launch writes only the slabs of its own K-slices, bytes [4096, 4096 + rem8 nslices 65536 x 4)
with rem8 and nslices THE PLANNER'S, a split launch does write them, an unsplit one touches nothing, and the tickets are back at zero."""
import ctypes as C

import pytest
import torch

from tests import fwd_ref as FR
from tests import workspace_cases as WC
from tests.test_fuzz_gemm_gpu import GEMM_CASES, _desc, gemm_operands
from tests.test_gemm_plan_cpu import fake_desc, path_of, plan, table_cases

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def L(gpu):
    from unigen_amd import lib
    lib.load()
    return lib


def test_planner_is_gemm_path_on_this_chip(gpu, L):
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    for label, c, _, _ in table_cases():
        for ws in (True, False):
            rc, p = plan(L, fake_desc(L, c, ws), ncu)
            assert rc == L.UG_OK and path_of(p) == FR.gemm_path(c, ncu, workspace=ws), (label, ws, ncu, rc, path_of(p), FR.gemm_path(c, ncu, workspace=ws))


def test_planned_is_what_ran(gpu, L):
    lib = L.load()
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    size = lambda i: GEMM_CASES[i]["M"] * GEMM_CASES[i]["N"] * GEMM_CASES[i]["K"] * GEMM_CASES[i]["groups"]
    paths = [path_of(plan(L, fake_desc(L, c), ncu)[1]) for c in GEMM_CASES]
    kinds = dict(split=lambda p: p[0] == 256 and p[2] > 1, unsplit=lambda p: p[0] == 256 and p[2] == 1, tile128=lambda p: p[0] == 128)
    picks = {k: min((i for i, p in enumerate(paths) if f(p)), key=size, default=None) for k, f in kinds.items()}
    assert None not in picks.values(), (f"on {ncu} CUs the table has no case of every kind", picks)
    for kind, i in picks.items():
        c = GEMM_CASES[i]
        o = gemm_operands(c, 7000 + i, gpu)
        ws = torch.full((WC.GEMM_WORKSPACE_BYTES,), POISON, dtype=torch.uint8, device=gpu)
        ws[:WC.TICKET_BYTES] = 0
        cb = o["c0"].clone()
        d = _desc(L, c, o, cb, ws)
        rc, p = plan(L, d, ncu)                                  # the real descriptor's plan: the launch below takes this very decision
        assert rc == L.UG_OK and path_of(p) == paths[i], (c["name"], rc, path_of(p), paths[i])
        touched = WC.TICKET_BYTES + (p.rem8 * p.nslices * WC.SLAB_BYTES if p.nslices > 1 else 0)
        assert touched == WC.gemm_touched_bytes(path_of(p)) <= WC.GEMM_WORKSPACE_BYTES
        rc = lib.ug_gemm_bf16(C.byref(d), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, (c["name"], rc, lib.ug_last_error())
        print(f"{kind}: [{c['name']}] plan {path_of(p)} grid {p.grid} x {p.grid_z}, may touch {touched} bytes")
        assert not bool(ws[:WC.TICKET_BYTES].any()), (c["name"], "arrival tickets not left at zero")
        assert bool((ws[touched:] == POISON).all()), (c["name"], f"wrote beyond the slabs of the planned K-slices (byte {touched} on)")
        assert bool((ws[WC.TICKET_BYTES:touched] != POISON).any()) == (kind == "split"), (c["name"], "a split launch writes its slabs, an unsplit one nothing")
        assert bool((cb != o["c0"]).any()), (c["name"], "no output written")
        del o, ws, cb
