"""The compiled resource contracts of the product library's kernels (data of tests/test_code_object_cpu.py; the records come from tests/code_object.py).

UNIVERSAL: every kernel runs wave64, has a static stack, at most 64 KiB of static LDS, and neither scratch nor VGPR spills - unless EXCEPTIONS lists
it with its ceilings and the cause. SGPR spills go to VGPR lanes (v_writelane / v_readlane): no memory traffic, so they are recorded (HOT) but not
forbidden.

HOT: the hand-scheduled kernels whose register budget the sources and docs state. The ceilings are what the head commit compiles to with hipcc
7.2.26015 (AMD clang 22.0.0git, roc-7.2.0), the flags of unigen_amd/build.py; compiler output is deterministic, so there is no margin. An edit that moves
a row is made together with the edit of this table (`python tools/code_object_report.py --diff before.json` shows the rows that moved), so that
whoever changes a hot kernel sees what the change did to its registers before a GPU is asked for. docs/KERNEL_NOTES.md, "Code-object contracts".
"""

MAX_STATIC_LDS = 65536

# kernel name -> dict(private_segment_fixed_size=, vgpr_spill_count=, reason=). May only shrink: an entry whose kernel is gone, or clean, fails.
EXCEPTIONS: dict = {}

# kernel name -> ceilings (vgpr_count, agpr_count, sgpr_spill_count, max_flat_workgroup_size). vgpr_count is the metadata's: it includes the AGPRs of
# a kernel that uses them (unified file, AGPRs start at the next multiple of 4: small_linear_kernel<16> = 256 + 100).
_H = lambda v, a, s, wg: dict(vgpr_count=v, agpr_count=a, sgpr_spill_count=s, max_flat_workgroup_size=wg)
HOT = {
    # 256^2 GEMM <EPI, LORA, QKDH, CONV>: one workgroup of 512 per CU, budget 256 VGPRs
    "gemm256_kernel<0, false, 128, false>": _H(249, 0, 97, 512),
    "gemm256_kernel<0, false, 128, true>": _H(248, 0, 90, 512),
    "gemm256_kernel<0, true, 128, false>": _H(228, 0, 75, 512),
    "gemm256_kernel<1, false, 128, false>": _H(246, 0, 91, 512),
    "gemm256_kernel<1, true, 128, false>": _H(229, 0, 78, 512),
    "gemm256_kernel<2, false, 128, false>": _H(248, 0, 121, 512),
    "gemm256_kernel<2, true, 128, false>": _H(254, 0, 120, 512),
    "gemm256_kernel<3, false, 128, false>": _H(242, 0, 104, 512),
    "gemm256_kernel<3, false, 128, true>": _H(250, 0, 114, 512),
    "gemm256_kernel<3, true, 128, false>": _H(242, 0, 100, 512),
    "gemm256_kernel<4, false, 128, false>": _H(246, 0, 69, 512),
    "gemm256_kernel<5, false, 128, false>": _H(248, 0, 124, 512),
    "gemm256_kernel<5, false, 64, false>": _H(248, 0, 124, 512),
    # 128^2 GEMM <EPI> and the direct convolution <NWM, NST>
    "gemm128_kernel<0>": _H(84, 0, 0, 512),
    "gemm128_kernel<1>": _H(84, 0, 0, 512),
    "gemm128_kernel<2>": _H(81, 0, 0, 512),
    "gemm128_kernel<3>": _H(81, 0, 0, 512),
    "gemm128_kernel<4>": _H(84, 0, 0, 512),
    "conv2d_nhwc_kernel<2, 2>": _H(133, 0, 0, 256),
    # attention forward <DH, BUFD>: head width 64 must stay at or below 128 registers (two workgroups per CU)
    "flash_attn_kernel<128, false>": _H(227, 0, 9, 512),
    "flash_attn_kernel<64, false>": _H(123, 0, 25, 512),
    "flash_attn_kernel<64, true>": _H(125, 0, 22, 512),
    # attention backward
    "attn_bwd_kernel<128, false>": _H(97, 0, 0, 512),
    "attn_bwd_kernel<128, true>": _H(249, 0, 0, 512),
    "attn_bwd_kernel<64, false>": _H(82, 0, 0, 512),
    "attn_bwd_kernel<64, true>": _H(172, 0, 0, 512),
    "attn_bwd_dq_kernel<128>": _H(254, 0, 0, 512),
    "attn_bwd_dkv_kernel<128>": _H(240, 0, 0, 512),
    "attn_bwd_dkv_kernel<64>": _H(170, 0, 0, 512),
    # small linear <MT>
    "small_linear_kernel<4>": _H(166, 0, 0, 256),
    "small_linear_kernel<8>": _H(230, 0, 0, 256),
    "small_linear_kernel<16>": _H(356, 100, 0, 256),
    # fast GroupNorm <CCH>
    "gn_apply_fast_kernel<16>": _H(117, 0, 0, 256),
    "gn_apply_fast_kernel<32>": _H(117, 0, 0, 256),
    "gn_apply_fast_kernel<64>": _H(117, 0, 0, 256),
    "gn_partial_fast_kernel<16>": _H(62, 0, 0, 256),
    "gn_partial_fast_kernel<32>": _H(62, 0, 0, 256),
    "gn_partial_fast_kernel<64>": _H(62, 0, 0, 256),
}


def template_name(kernel: str) -> str:
    return kernel.split("<", 1)[0]


def universal_violations(name: str, rec: dict, exceptions: dict = EXCEPTIONS) -> list:
    """what the universal contract has against one kernel's record ([] = nothing)"""
    bad = []
    if rec["wavefront_size"] != 64:
        bad.append(f"{name}: wavefront_size {rec['wavefront_size']}, not 64")
    if rec["uses_dynamic_stack"]:
        bad.append(f"{name}: uses a dynamic stack")
    if rec["group_segment_fixed_size"] > MAX_STATIC_LDS:
        bad.append(f"{name}: {rec['group_segment_fixed_size']} bytes of static LDS, above {MAX_STATIC_LDS}")
    ceil = exceptions.get(name, dict(private_segment_fixed_size=0, vgpr_spill_count=0))
    for f in ("private_segment_fixed_size", "vgpr_spill_count"):
        if rec[f] > ceil[f]:
            bad.append(f"{name}: {f} {rec[f]}, ceiling {ceil[f]}" + ("" if name in exceptions else " (no scratch, no VGPR spills; EXCEPTIONS has no entry)"))
    return bad


def exception_violations(recs: dict, exceptions: dict = EXCEPTIONS) -> list:
    """entries of the exceptions table that have no business there any more: the table may only shrink"""
    bad = []
    for name, e in exceptions.items():
        if not str(e.get("reason", "")).strip():
            bad.append(f"EXCEPTIONS[{name!r}] gives no reason")
        if name not in recs:
            bad.append(f"EXCEPTIONS[{name!r}]: no such kernel in the library any more - delete the entry")
        elif recs[name]["private_segment_fixed_size"] == 0 and recs[name]["vgpr_spill_count"] == 0:
            bad.append(f"EXCEPTIONS[{name!r}]: the kernel is clean now - delete the entry")
    return bad


def hot_violations(recs: dict, hot: dict = HOT) -> list:
    bad = []
    templates = {template_name(n) for n in hot}
    for name in sorted(recs):
        if template_name(name) in templates and name not in hot:
            bad.append(f"{name}: an instantiation of a HOT template without a row in HOT")
    for name, ceil in hot.items():
        if name not in recs:
            bad.append(f"HOT[{name!r}]: no such kernel in the library - delete or rename the row")
            continue
        for f, c in ceil.items():
            if recs[name][f] > c:
                bad.append(f"{name}: {f} {recs[name][f]}, ceiling {c}")
    return bad
