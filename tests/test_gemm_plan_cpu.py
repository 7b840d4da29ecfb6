"""The GEMM dispatcher's own decision (ug_gemm_plan: gemm_check, then gemm_plan of csrc/gemm.hip - what ug_gemm_bf16 launches) against its
independent restatement tests/fwd_ref.py::gemm_path and the literal paths of the case tables, and every refusal of ug_gemm_bf16, without a GPU:
the planner dereferences no pointer, so the descriptors carry fake addresses (with the cases' c_off / r_off alignment).

  - test_case_tables: every GEMM_CASES entry of tests/test_fuzz_gemm_gpu.py, every GEMM entry of tests/index_range_cases.py (base and far) and
    the launch sequence of tests/workspace_cases.py: planner at 256 CUs == the literal path / path_nows == gemm_path.
  - test_lattice: planner == gemm_path on a lattice over M, N, K (95 and 96 K-tiles: either side of the split threshold), epilogue, groups,
    A row map, workspace, UG_GEMM_FORCE_TILE and CU count.
  - test_qk_rope_fusable_shapes_take_the_256_kernel: where ops.qk_rope_fusable says yes, a UG_EPI_QKV_ROPE descriptor is accepted, on 256^2 tiles.
  - test_refusals_*: REFUSALS trips each UG_REQUIRE of ug_gemm_bf16 (and of its q/k RoPE launcher) alone, and some in pairs for their order. The
    expected codes and leading message texts are literals written from the source of the commit BEFORE gemm_check existed; every refusal precedes
    any launch, so the same table runs against ug_gemm_bf16 here. That half (`-k gemm_bf16`) also passes in a checkout of that commit with this
    file copied in (its library has no ug_gemm_plan): 1 passed there, 1 passed here."""
import ctypes as C
import itertools

import pytest

from tests import fwd_ref as FR
from tests import index_range_cases as IC
from tests import test_fuzz_gemm_gpu as TG
from tests import workspace_cases as WC

P = 1 << 20                      # fake device addresses: operand i at (i + 1) * P, 4096-byte aligned
B, G, RG, RS, EF, QK = FR.EPI_BIAS, FR.EPI_BIAS_GELU, FR.EPI_RES_GATE, FR.EPI_RES_SCALE, FR.EPI_F32, 5


class _Fake:
    """stands where the sweeps' descriptor builder takes a tensor: an address, an element size, a byte count"""

    def __init__(self, addr, es=2, n=0):
        self.addr, self.es, self.n = addr, es, n

    def data_ptr(self):
        return self.addr

    def element_size(self):
        return self.es

    def numel(self):
        return self.n


@pytest.fixture(scope="module")
def L():
    from unigen_amd import lib
    lib.load()
    return lib


def fake_desc(L, c, workspace=True):
    """the descriptor tests/test_fuzz_gemm_gpu.py::_desc builds for case c, on fake operands"""
    res = c["epilogue"] in (RG, RS)
    o = dict(a=_Fake(1 * P), w=_Fake(2 * P), bias=_Fake(3 * P) if c.get("has_bias", True) else None, gate=_Fake(4 * P) if c["epilogue"] == RG else None,
             r=_Fake(5 * P) if res and not c.get("alias") else None)
    ws = _Fake(7 * P, 1, int(L.load().ug_gemm_workspace_bytes())) if workspace else None
    return TG._desc(L, c, o, _Fake(6 * P, 4 if c["epilogue"] == EF else 2), ws)


def plan(L, d, ncu, force=0):
    """-> (code, ug_gemm_dispatch)"""
    out = L.STRUCTS["ug_gemm_dispatch"]()
    return L.load().ug_gemm_plan(C.byref(d), ncu, force, C.byref(out)), out


def path_of(p):
    """the five figures the case tables and gemm_path name"""
    return p.tile, p.rounds, p.nslices, p.rem8, p.wide16


def table_cases():
    """(label, case, literal path or None, literal path without workspace or None) of every table"""
    rows = [(f"GEMM_CASES[{i}] {c['name']}", c, c["path"], c["path_nows"]) for i, c in enumerate(TG.GEMM_CASES)]
    for k in IC.gemm_far_cases():
        rows.append((f"index range base: {k['name']}", k["base"], None, None))                # the literal path is the FAR descriptor's (a far ldw
        rows.append((f"index range far: {k['name']}", k["far"], k["base"]["path"], None))     # is what sends a case to the 128^2 kernel)
    rows += [(f"GEMM_SEQUENCE {TG.GEMM_CASES[i]['name']}", TG.GEMM_CASES[i], TG.GEMM_CASES[i]["path"], TG.GEMM_CASES[i]["path_nows"]) for i in WC.GEMM_SEQUENCE]
    return rows


def test_case_tables(L):
    rows = table_cases()
    assert len(rows) == len(TG.GEMM_CASES) + 2 * len(IC.gemm_far_cases()) + len(WC.GEMM_SEQUENCE)
    for label, c, want, want_nows in rows:
        for ws, lit in ((True, want), (False, want_nows)):
            rc, p = plan(L, fake_desc(L, c, ws), 256)
            assert rc == L.UG_OK, (label, ws, rc, L.load().ug_last_error())
            ref = FR.gemm_path(c, 256, workspace=ws)
            assert path_of(p) == ref, (label, ws, path_of(p), ref)
            if lit is not None:
                assert path_of(p) == tuple(lit), (label, ws, path_of(p), lit)
            # what the launch gets is consistent with the five figures
            assert p.grid_z == (1 if p.tile == 256 else max(c["groups"], 1)) and p.variant == L.UG_GEMM_PLAIN
            if p.tile == 256:
                split = p.nslices > 1
                assert p.tiles == p.tiles_per_group * max(c["groups"], 1) and p.full_tiles == (p.tiles - p.tiles % 256 if split else p.tiles)
                assert p.grid == (p.rem8 * p.nslices if split and p.tiles < 256 else min(p.tiles, 256)) and p.group_m == 4 and p.walk == 0
        rc, p = plan(L, fake_desc(L, c), 256, 128)
        assert rc == L.UG_OK and path_of(p) == (128, 1, 1, 0, 0) == FR.gemm_path(c, 256, force=128), label


LATTICE_M = (1, 128, 191, 192, 255, 256, 257, 333, 512, 1024, 4608, 9216, 18432)
LATTICE_N = (64, 192, 256, 260, 1536, 3072, 9216, 12288, 15360)
LATTICE_K = (64, 128, 3072, 6080, 6144, 12288, 15360)          # 6080, 6144: 95 and 96 K-tiles
LATTICE_EPI = (B, G, RG, RS, EF)
LATTICE_GROUPS = (1, 3)
LATTICE_A_MAPS = ((0, 0), (100, 117), (500, 0))                 # identity, monotonic with batch jumps inside a tile, broadcasting
LATTICE_FORCE = (0, 128, 256)
LATTICE_NCU = (8, 64, 256, 304)


def lattice_case(M, N, K, epi, groups, a_map):
    """a compact case: lda = ldw = K, ldc = ldr = N (so N = 260 has the narrow epilogue), bases 16-byte aligned, group strides multiples of 8"""
    many = groups > 1
    return dict(M=M, N=N, K=K, epilogue=epi, groups=groups, has_bias=True, rows_per_sample=100 if epi == RG else 0, a_map=a_map, c_map=(0, 0), r_map=(0, 0),
                alias=False, gelu_from_n=0, c_shift_from_n=0, c_shift=0, alpha=1.0, lda=K, ldw=K, ldc=N, ldr=N, c_off=0, r_off=0, gate_ld=N,
                a_gstride=8 * M * K if many else 0, w_gstride=N * K if many else 0, bias_gstride=N if many else 0, c_gstride=2 * M * N if many else 0,
                r_gstride=2 * M * N if many else 0, gate_gstride=2 * M * N if many else 0)


def test_lattice(L):
    fn, out = L.load().ug_gemm_plan, L.STRUCTS["ug_gemm_dispatch"]()
    bad, n, seen = [], 0, set()
    for M, N, K, epi, groups, a_map in itertools.product(LATTICE_M, LATTICE_N, LATTICE_K, LATTICE_EPI, LATTICE_GROUPS, LATTICE_A_MAPS):
        c = lattice_case(M, N, K, epi, groups, a_map)
        for ws in (True, False):
            d = C.byref(fake_desc(L, c, ws))
            for force, ncu in itertools.product(LATTICE_FORCE, LATTICE_NCU):
                rc = fn(d, ncu, force, C.byref(out))
                got, ref = path_of(out), FR.gemm_path(c, ncu, force=force, workspace=ws)
                n += 1
                seen.add((got[0], got[2] > 1, got[4]))
                if rc != L.UG_OK or got != ref:
                    bad.append((M, N, K, epi, groups, a_map, ws, force, ncu, rc, got, ref))
    assert not bad, (len(bad), n, bad[:20])
    # the lattice reaches both tiles, split and unsplit launches and every wide16 value of the 256^2 kernel's identity C map
    assert {(128, False, 0), (256, False, 3), (256, True, 3), (256, False, 2), (256, True, 2)} <= seen, seen


def qk_case(M, N, K, dh):
    return dict(lattice_case(M, N, K, B, 1, (0, 0)), epilogue=QK, qk_dh=dh)


def qk_desc(L, c, until_n=256):
    d = fake_desc(L, dict(c, epilogue=B))
    d.epilogue, d.qk_wq, d.qk_wk, d.rope_cs, d.qk_until_n, d.qk_dh, d.qk_eps = QK, 8 * P, 9 * P, 10 * P, until_n, c["qk_dh"], 1e-6
    return d


def test_qk_rope_fusable_shapes_take_the_256_kernel(L):
    import torch
    from unigen_amd import ops
    n = 0
    for M, N, K, dh in itertools.product(LATTICE_M, LATTICE_N, LATTICE_K, (64, 128)):
        if not ops.qk_rope_fusable(M, N, 256, dh, torch.bfloat16):
            continue
        n += 1
        for force, ncu in itertools.product(LATTICE_FORCE, LATTICE_NCU):
            rc, p = plan(L, qk_desc(L, qk_case(M, N, K, dh)), ncu, force)
            assert rc == L.UG_OK and p.tile == 256, (M, N, K, dh, force, ncu, rc, L.load().ug_last_error())
            assert p.variant == (L.UG_GEMM_QK128 if dh == 128 else L.UG_GEMM_QK64) and (p.nslices, p.rem8, p.wide16) == (1, 0, 3)
            assert p.grid == min(p.tiles, ncu) and p.tiles == (M // 256) * (N // 256) and p.rounds == -(-p.tiles // ncu)
    assert n >= 20, n


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
# (epilogue of the starting descriptor, {field: value} laid over it, expected code, leading text of the message). Addresses: "+n" = n bytes
# off the fake base. Written from ug_gemm_bf16 and launch_qkrope of the commit before gemm_check, in the order of their UG_REQUIREs.
BIG = 1 << 31
LORA = dict(lora_r=64, lora_T=11 * P, ldt=64, lora_B=12 * P, ldb=64)
_S, _A, _U = "UG_ERR_BAD_SHAPE", "UG_ERR_BAD_ALIGN", "UG_ERR_UNSUPPORTED"
REFUSALS = [
    (B, dict(M=-1), _S, b"ug_gemm_bf16: bad M/N/K -1/"), (B, dict(N=0), _S, b"ug_gemm_bf16: bad M/N/K"), (B, dict(K=0), _S, b"ug_gemm_bf16: bad M/N/K"),
    (B, dict(K=-64), _S, b"ug_gemm_bf16: bad M/N/K"),
] + [(RG, {f: BIG}, _U, b"ug_gemm_bf16: row counts must fit 31 bits")
     for f in ("M", "N", "a_bstride", "c_bstride", "r_bstride", "a_rpb", "c_rpb", "r_rpb", "rows_per_sample")] + [
    (B, dict(K=96), _U, b"ug_gemm_bf16: K=96 must be a multiple of 64"),
    (B, dict(N=514), _U, b"ug_gemm_bf16: N=514 must be a multiple of 4"),
] + [(G, kw, _S, b"ug_gemm_bf16: column split needs gelu_from_n, c_shift_from_n multiples of 256")
     for kw in (dict(gelu_from_n=-256), dict(gelu_from_n=100), dict(c_shift_from_n=-256), dict(c_shift_from_n=100), dict(c_shift_from_n=256, c_shift=4),
                dict(c_shift=8), dict(c_shift_from_n=256, c_shift=16), dict(ldc=504))] + [     # ldc 520 < N + c_shift; ldc < N is caught HERE, not as a leading dim
    (B, {f: None}, _S, b"ug_gemm_bf16: null operand") for f in ("A", "W", "C")] + [
    (B, dict(lda=120), _S, b"ug_gemm_bf16: leading dims too small"), (B, dict(ldw=120), _S, b"ug_gemm_bf16: leading dims too small"),
] + [(B, kw, _A, b"ug_gemm_bf16: A/W need 16-byte aligned rows")
     for kw in (dict(lda=132), dict(ldw=132), dict(A="+8"), dict(W="+8"), dict(a_gstride=4), dict(w_gstride=4))] + [
    (B, dict(ldc=522), _A, b"ug_gemm_bf16: C needs ldc % 4 == 0"), (B, dict(C="+4"), _A, b"ug_gemm_bf16: C needs"),
    (EF, dict(C="+8"), _A, b"ug_gemm_bf16: C needs"), (B, dict(c_gstride=2), _A, b"ug_gemm_bf16: C needs"),
    (B, dict(bias="+4"), _A, b"ug_gemm_bf16: bias alignment"), (B, dict(bias_gstride=2), _A, b"ug_gemm_bf16: bias alignment"),
] + [(e, kw, _A, b"ug_gemm_bf16: residual missing/misaligned")
     for e in (RG, RS) for kw in (dict(R=None), dict(ldr=522), dict(R="+4"), dict(r_gstride=2))] + [
    (RG, kw, _S, b"ug_gemm_bf16: gate missing/misaligned")
    for kw in (dict(gate=None), dict(rows_per_sample=0), dict(rows_per_sample=-1), dict(gate_ld=522), dict(gate="+4"), dict(gate_gstride=2))] + [
    (B, dict(LORA, lora_r=32), _U, b"ug_gemm_bf16: lora_r=32 must be padded to a multiple of 64"),
] + [(B, dict(LORA, **kw), _A, b"ug_gemm_bf16: LoRA operands missing/misaligned")
     for kw in (dict(lora_T=None), dict(lora_B=None), dict(ldt=68), dict(ldb=68), dict(lora_T="+8"), dict(lora_B="+8"))] + [
    (B, dict(LORA, groups=2), _U, b"ug_gemm_bf16: LoRA epilogue is not grouped"),
    (B, dict(epilogue=6), _U, b"ug_gemm_bf16: unknown epilogue 6"), (B, dict(epilogue=-1), _U, b"ug_gemm_bf16: unknown epilogue -1"),
] + [(QK, kw, _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE needs M, N, qk_until_n multiples of 256 (M=")
     for kw in (dict(M=500), dict(N=520), dict(qk_until_n=0), dict(qk_until_n=128), dict(qk_until_n=768))] + [
    (QK, dict(groups=2), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE is neither grouped nor LoRA-extended"),
    (QK, dict(LORA), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE is neither grouped nor LoRA-extended"),
    (QK, dict(qk_dh=96), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE head width 96 not in {64, 128}"),
] + [(QK, kw, _A, b"ug_gemm_bf16: UG_EPI_QKV_ROPE operands missing/misaligned")
     for kw in (dict(qk_wq=None), dict(qk_wk=None), dict(rope_cs=None), dict(qk_dh=0, rope_cs=None), dict(qk_wq="+4"), dict(qk_wk="+4"), dict(rope_cs="+8"),
                dict(ldc=524), dict(C="+8"))] + [
    (QK, kw, _S, b"ug_gemm_bf16: UG_EPI_QKV_ROPE bad positions / column split")
    for kw in (dict(rope_rpb=100), dict(rope_rpb=BIG), dict(rope_pos0=-1), dict(rope_pos0=BIG), dict(gelu_from_n=256, qk_until_n=512),
               dict(c_shift_from_n=256, c_shift=8, qk_until_n=512))] + [
    (QK, kw, _S, b"ug_gemm_bf16: UG_EPI_QKV_ROPE needs a monotonic A row map (batch stride")
    for kw in (dict(a_rpb=256, a_bstride=0), dict(a_rpb=256, a_bstride=248), dict(lda=4210760), dict(ldw=4210760), dict(a_rpb=1, a_bstride=33000))] + [     # (255 batch jumps of 32999 rows x 256 bytes)
    (QK, dict(c_rpb=1000, c_bstride=1000), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE needs the C row map's rows per batch (1000)"),
    # in pairs: the earlier UG_REQUIRE wins
    (B, dict(M=-1, K=96), _S, b"ug_gemm_bf16: bad M/N/K"),
    (B, dict(M=BIG, K=96), _U, b"ug_gemm_bf16: row counts"),
    (B, dict(K=96, N=514), _U, b"ug_gemm_bf16: K=96"),
    (B, dict(N=514, A=None), _U, b"ug_gemm_bf16: N=514"),
    (G, dict(gelu_from_n=100, A=None), _S, b"ug_gemm_bf16: column split"),
    (B, dict(C=None, lda=120), _S, b"ug_gemm_bf16: null operand"),
    (B, dict(ldw=120, lda=132), _S, b"ug_gemm_bf16: leading dims"),
    (B, dict(A="+8", C="+4"), _A, b"ug_gemm_bf16: A/W need"),
    (RS, dict(ldc=522, bias="+4"), _A, b"ug_gemm_bf16: C needs"),
    (RS, dict(bias="+4", R=None), _A, b"ug_gemm_bf16: bias alignment"),
    (RG, dict(R=None, gate=None), _A, b"ug_gemm_bf16: residual"),
    (RG, dict(LORA, gate=None, lora_r=32), _S, b"ug_gemm_bf16: gate"),
    (B, dict(LORA, lora_r=32, lora_T=None), _U, b"ug_gemm_bf16: lora_r=32"),
    (B, dict(LORA, lora_B="+8", groups=2), _A, b"ug_gemm_bf16: LoRA operands"),
    (B, dict(LORA, groups=2, epilogue=6), _U, b"ug_gemm_bf16: LoRA epilogue is not grouped"),
    (QK, dict(K=96, M=500), _U, b"ug_gemm_bf16: K=96"),                                   # every general check before the q/k ones
    (QK, dict(bias="+4", M=500), _A, b"ug_gemm_bf16: bias alignment"),
    (QK, dict(LORA, lora_r=32), _U, b"ug_gemm_bf16: lora_r=32"),
    (QK, dict(M=500, groups=2), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE needs M, N"),
    (QK, dict(groups=2, qk_dh=96), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE is neither"),
    (QK, dict(qk_dh=96, qk_wq=None), _U, b"ug_gemm_bf16: UG_EPI_QKV_ROPE head width"),
    (QK, dict(qk_wk="+4", rope_pos0=-1), _A, b"ug_gemm_bf16: UG_EPI_QKV_ROPE operands"),
    (QK, dict(rope_rpb=100, a_rpb=256, a_bstride=0), _S, b"ug_gemm_bf16: UG_EPI_QKV_ROPE bad positions"),
    (QK, dict(lda=4210760, c_rpb=1000, c_bstride=1000), _S, b"ug_gemm_bf16: UG_EPI_QKV_ROPE needs a monotonic"),
]
# accepted by the checks: M == 0 ends them where it stands (UG_OK, nothing launched), whatever follows it
NOTHING_TO_DO = [(B, dict(M=0)), (B, dict(M=0, A=None, K=96, epilogue=6)), (QK, dict(M=0, qk_wq=None))]
# accepted, as far as the planner (never sent to ug_gemm_bf16 here: they would launch)
ACCEPTED = [(B, {}), (G, dict(gelu_from_n=256, c_shift_from_n=256, c_shift=8)), (RG, {}), (RS, {}), (EF, {}), (QK, {}), (QK, dict(qk_dh=64, rope_cs=None)),
            (QK, dict(qk_dh=0)), (B, dict(groups=0)), (B, dict(LORA, groups=-3)), (B, dict(LORA)), (QK, dict(rope_rpb=256, c_rpb=256, c_bstride=300)),
            (QK, dict(a_rpb=256, a_bstride=256)), (B, dict(a_rpb=256, a_bstride=0)), (B, dict(ldc=516)), (B, dict(bias=None))]
_PTRS = dict(A=1, W=2, bias=3, gate=4, R=5, C=6, workspace=7, qk_wq=8, qk_wk=9, rope_cs=10, lora_T=11, lora_B=12)


def start_desc(L, epi, kw):
    """a descriptor every check accepts (M 512, N 512, K 128, ldc 520; under UG_EPI_QKV_ROPE heads of 128 up to column 256), with kw laid over it"""
    c = dict(lattice_case(512, 512, 128, B if epi == QK else epi, 1, (0, 0)), ldc=520, ldr=520, gate_ld=520)
    d = qk_desc(L, dict(c, qk_dh=128)) if epi == QK else fake_desc(L, c)
    for k, v in kw.items():
        setattr(d, k, _PTRS[k] * P + int(v) if isinstance(v, str) else v)
    return d


def _refused(L, call, what):
    for epi, kw, code, text in REFUSALS:
        rc = call(C.byref(start_desc(L, epi, kw)))
        msg = L.load().ug_last_error()
        assert rc == getattr(L, code) and msg.startswith(text), (what, epi, kw, rc, msg, code, text)
    for epi, kw in NOTHING_TO_DO:
        assert call(C.byref(start_desc(L, epi, kw))) == L.UG_OK, (what, epi, kw, L.load().ug_last_error())
    rc = call(None)
    assert rc == L.UG_ERR_BAD_SHAPE and L.load().ug_last_error().startswith(b"ug_gemm_bf16: null descriptor"), (what, rc)


def test_refusals_gemm_bf16(L):
    """every refusal precedes the first HIP call of ug_gemm_bf16: none of these reaches a device"""
    _refused(L, lambda d: L.load().ug_gemm_bf16(d, None), "ug_gemm_bf16")


def test_refusals_gemm_plan(L):
    out = L.STRUCTS["ug_gemm_dispatch"]()
    _refused(L, lambda d: L.load().ug_gemm_plan(d, 256, 0, C.byref(out)), "ug_gemm_plan")
    for epi, kw in NOTHING_TO_DO:                                            # nothing to launch: an all-zero plan
        out.tile = out.grid = 77
        assert L.load().ug_gemm_plan(C.byref(start_desc(L, epi, kw)), 256, 0, C.byref(out)) == L.UG_OK and bytes(out) == bytes(C.sizeof(out))
    for epi, kw in ACCEPTED:
        rc, p = plan(L, start_desc(L, epi, kw), 256)
        assert rc == L.UG_OK and p.tile in (128, 256), (epi, kw, rc, L.load().ug_last_error())
    # its own two arguments, after the descriptor's checks
    d = start_desc(L, B, {})
    for ncu in (0, -1):
        assert L.load().ug_gemm_plan(C.byref(d), ncu, 0, C.byref(out)) == L.UG_ERR_BAD_SHAPE and L.load().ug_last_error().startswith(b"ug_gemm_plan:")
    assert L.load().ug_gemm_plan(C.byref(d), 256, 0, None) == L.UG_ERR_BAD_SHAPE
    assert L.load().ug_gemm_plan(C.byref(start_desc(L, B, dict(K=96))), 0, 0, None) == L.UG_ERR_UNSUPPORTED


def test_lora_descriptors_plan_the_lora_variant(L):
    """gemm_path leaves LoRA out; the rule of the header: the 256^2 kernel's LoRA variant with K >= 128, never under UG_EPI_F32, never split"""
    for epi, K, want in ((B, 128, 256), (RG, 6144, 256), (B, 64, 128), (EF, 6144, 128)):
        c = dict(lattice_case(4608, 4360, K, epi, 1, (0, 0)), ldc=4360 + 8, ldr=4360 + 8, gate_ld=4360 + 8)      # 18 x 18 tiles: a split tail without LoRA
        d = fake_desc(L, c)
        for k, v in LORA.items():
            setattr(d, k, v)
        for force in (0, 256):
            rc, p = plan(L, d, 256, force)
            assert rc == L.UG_OK and p.tile == want and p.nslices == 1 and p.variant == (L.UG_GEMM_LORA if want == 256 else L.UG_GEMM_PLAIN), (epi, K, force)
