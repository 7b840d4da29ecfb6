"""The compiled artifact: every kernel of the product library against its resource contract (tests/code_object_contracts.py), read from the code
objects' metadata by tests/code_object.py. No GPU: hipcc cross-compiles for gfx950, llvm-objdump / llvm-readelf read what it wrote.

  - the reader itself, on three throwaway kernels (a reader that returned zeros would pass every contract below);
  - the universal contract: wave64, static stack, static LDS <= 64 KiB, no scratch and no VGPR spills outside EXCEPTIONS, and EXCEPTIONS only shrinks;
  - the HOT table: ceilings on VGPRs, AGPRs, SGPR spills and workgroup size of the hand-scheduled kernels, one row per instantiation;
  - no kernel that only tools/probe/csrc defines is in the product library.
`python tools/code_object_report.py` prints the same records as a table (docs/KERNEL_NOTES.md, "Code-object contracts")."""
import glob
import os
import re

import pytest

from tests import code_object as CO
from tests import code_object_contracts as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRIVIAL = """
#include <hip/hip_runtime.h>
__global__ void co_trivial(float* x) { x[threadIdx.x] += 1.0f; }
"""
BOUNDED = """
#include <hip/hip_runtime.h>
__global__ __launch_bounds__(256) void co_bounded(float* x) { x[threadIdx.x] += 1.0f; }
"""
# 1024 floats per thread, written and then read at run-time indices: cannot live in registers
STACK = """
#include <hip/hip_runtime.h>
__global__ void co_stack(float* x, const int* idx, int n) {
    float t[1024];
    for (int i = 0; i < 1024; ++i) t[i] = 0.0f;
    for (int i = 0; i < n; ++i) t[idx[i] & 1023] += x[i];
    x[threadIdx.x] = t[idx[threadIdx.x] & 1023];
}
"""


@pytest.fixture(scope="module")
def product():
    return CO.kernels()


def test_reader_on_throwaway_kernels(tmp_path):
    recs = {}
    for stem, src in (("trivial", TRIVIAL), ("bounded", BOUNDED), ("stack", STACK)):
        recs.update(CO.kernels(CO.compile_device(src, str(tmp_path), stem)))
    assert set(recs) == {"co_trivial", "co_bounded", "co_stack"}, sorted(recs)
    for r in recs.values():
        assert set(CO.FIELDS) <= set(r)
        assert r["wavefront_size"] == 64 and r["kernarg_segment_size"] >= 8 and r["vgpr_count"] > 0 and r["sgpr_count"] > 0, r
    t, b, s = recs["co_trivial"], recs["co_bounded"], recs["co_stack"]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and not t["uses_dynamic_stack"], t
    assert t["max_flat_workgroup_size"] == 1024 and b["max_flat_workgroup_size"] == 256, (t, b)      # hipcc's default bound is 1024
    assert s["private_segment_fixed_size"] >= 4096, s
    assert CC.universal_violations("co_trivial", t, {}) == [] and CC.universal_violations("co_bounded", b, {}) == []
    bad = CC.universal_violations("co_stack", s, {})
    assert bad and "private_segment_fixed_size" in bad[0], bad
    # ... and the exceptions table: a ceiling holds, a lower one does not, an entry for a clean or a missing kernel is refused
    e = dict(private_segment_fixed_size=s["private_segment_fixed_size"], vgpr_spill_count=s["vgpr_spill_count"], reason="self-test")
    assert CC.universal_violations("co_stack", s, {"co_stack": e}) == []
    assert CC.universal_violations("co_stack", s, {"co_stack": dict(e, private_segment_fixed_size=e["private_segment_fixed_size"] - 4)})
    assert CC.exception_violations(recs, {"co_stack": e}) == []
    assert CC.exception_violations(recs, {"co_trivial": e}) and CC.exception_violations(recs, {"co_gone": e}) and CC.exception_violations(recs, {"co_stack": dict(e, reason="")})
    # ... and the hot table: a ceiling one below the record, a missing row of a listed template, a row without a kernel
    row = {f: b[f] for f in ("vgpr_count", "agpr_count", "sgpr_spill_count", "max_flat_workgroup_size")}
    assert CC.hot_violations(recs, {"co_bounded": row}) == []
    assert CC.hot_violations(recs, {"co_bounded": dict(row, vgpr_count=row["vgpr_count"] - 1)})
    assert CC.hot_violations(recs, {"co_bounded": dict(row, max_flat_workgroup_size=128)})
    assert CC.hot_violations({"k<1>": b, "k<2>": b}, {"k<1>": row}) and CC.hot_violations(recs, {"co_absent": row})


def test_reader_normalises_names_like_the_asm_diff_tool():
    assert CO.normalise("void (anonymous namespace)::gemm256_kernel<4, false, 128, false>(ug_gemm_desc, int, int)") == "gemm256_kernel<4, false, 128, false>"
    assert CO.normalise("plain_kernel") == "plain_kernel"
    assert CO.demangle(["_ZN12_GLOBAL__N_114gemm128_kernelILi3EEEv12ug_gemm_desc"]) == ["gemm128_kernel<3>"]


def test_universal_contract(product):
    assert len(product) >= 200, len(product)          # the whole library was read, not one bundle of it
    bad = [v for name in sorted(product) for v in CC.universal_violations(name, product[name])]
    assert not bad, "\n".join(bad)


def test_exceptions_only_shrink(product):
    bad = CC.exception_violations(product)
    assert not bad, "\n".join(bad)


def test_hot_kernel_ceilings(product):
    for t in ("gemm256_kernel", "gemm128_kernel", "conv2d_nhwc_kernel", "flash_attn_kernel", "attn_bwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel",
              "small_linear_kernel", "gn_apply_fast_kernel", "gn_partial_fast_kernel"):
        assert any(CC.template_name(n) == t for n in CC.HOT), f"HOT lost every row of {t}"
    bad = CC.hot_violations(product)
    assert not bad, "\n".join(bad)
    # the head-width-64 forward shares a CU between two workgroups of 512: more than 128 registers would halve its occupancy
    for name in product:
        if name.startswith("flash_attn_kernel<64,"):
            assert CC.HOT[name]["vgpr_count"] <= 128, name


def _global_names(paths):
    names = set()
    for p in paths:
        with open(p) as f:
            names |= set(re.findall(r"__global__\b[^;{}]*?\bvoid\s+(\w+)\s*\(", f.read()))
    return names


def test_no_probe_only_kernel_in_the_product_library(product):
    probe = _global_names(glob.glob(os.path.join(ROOT, "tools", "probe", "csrc", "*.hip")))
    own = _global_names(glob.glob(os.path.join(ROOT, "unigen_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "unigen_amd", "csrc", "*.h")))
    assert len(probe) >= 5 and len(own) >= 50, (len(probe), len(own))       # the scan found the definitions
    assert {CC.template_name(n) for n in product} <= own, sorted({CC.template_name(n) for n in product} - own)
    leaked = sorted(n for n in product if CC.template_name(n) in probe - own)
    assert not leaked, leaked
