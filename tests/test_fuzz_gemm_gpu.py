"""The base GEMM's dispatch paths (ug_gemm_bf16 without a LoRA segment, and ug_gemm_f32), ug_adaln_modulate (generic, fast NCH x 512, fp32 twin)
and ug_small_linear_bf16 against the float64 references of tests/fwd_ref.py (pinned to F.linear / F.gelu / F.layer_norm / F.silu and the
oracle's forms by tests/test_fwd_ref_cpu.py, which also shows that each plausible slip fails the judging function used here).

GEMM_CASES is data: each case names the dispatch path it is there for - (tile, rounds of the persistent walk, K-slices of the split-K tail,
tail tiles padded to 8, wide16 bits) at 256 CUs. tests/test_fwd_ref_cpu.py asserts fwd_ref.gemm_path(case, 256) == that path; the GPU test
asserts it again with the device's CU count and FAILS, naming the case, if it differs (no skip).

How a case is judged (docs/PARITY_TOLERANCES.md, "Base GEMM, AdaLN modulate and small linear sweep"):
  - bf16: rel-L2, worst row, worst row of the last partial tile <= max(1.5 x the rounding-point variant's own figure, 2^-9) against the fp64
    truth; fp32 twin and UG_EPI_F32 (nothing is rounded to bf16 in either): rel-L2 <= 1e-5, every row <= 1e-4.
  - M N K groups <= 2.5e9: the fp64 truth of every row. Larger: the fp64 truth on fwd_ref.sample_rows (tile rims, sample / row-map boundaries,
    last 8 rows, 8 seeded rows per tile) AND a full-output screen: torch's fp32 matmul on the GPU with the reference's bf16 epilogue steps in torch
    ops, itself first held to rel-L2 <= 1e-5 against the fp64 truth on the sampled rows; every output row within the row bound against the
    screen, and at most max(4 x SCREEN_SHARE, 0.1 %) of the elements more than one bf16 ulp from it.
  - every run (UG_GEMM_FORCE_TILE = 128, 256 without workspace, 0 with and without workspace) leaves every element outside its rows / columns
    (64 sentinels before and after, leading-dimension padding, row-map gaps, the column split's gap, the pads between groups) at 7.0; the 128^2
    and unsplit 256^2 results are bit-identical; a split-K result is bit-identical across three repeats; read-only operands are unchanged."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import fwd_ref as FR

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, PAD = 7.0, 64
FULL_TRUTH_MACS = 2.5e9
# share of elements of the rounding-point variant more than one bf16 ulp from the screen's rounded result, measured on the CPU on sampled rows of
# every large case (tests/test_fwd_ref_cpu.py::test_screen_share_of_the_variant asserts the measurement stays at or below this)
SCREEN_SHARE = 2.0e-4
SHARE_BOUND = max(4 * SCREEN_SHARE, 1e-3)
B, G, RG, RS, EF = FR.EPI_BIAS, FR.EPI_BIAS_GELU, FR.EPI_RES_GATE, FR.EPI_RES_SCALE, FR.EPI_F32


def _case(name, path, M, N, K, epilogue, *, path_nows=None, groups=1, bias=True, rps=0, a_map=(0, 0), c_map=(0, 0), alias=False, split=None, lda=None,
          ldc_extra=8, c_off=0, a_sparse=False, twin=True):
    """a GEMM case with its buffer geometry (elements): lda = K + 8, ldw = K + 8, ldc = N + shift + ldc_extra, R laid out as C; group strides
    64 elements larger than the operands"""
    cdiv = lambda x, y: (x + y - 1) // y
    span = lambda m: int(FR.rowmap(torch.arange(M), *m).max()) + 1
    gelu_from, shift = split or (0, 0)
    c = dict(name=name, path=tuple(path), path_nows=tuple(path_nows) if path_nows else None, M=M, N=N, K=K, epilogue=epilogue, groups=groups,
             has_bias=bias, rows_per_sample=rps, a_map=a_map, c_map=c_map, r_map=c_map, alias=alias, gelu_from_n=gelu_from,
             c_shift_from_n=gelu_from if shift else 0, c_shift=shift, alpha=0.7 if epilogue == RS else 1.0, lda=lda or K + 8, ldw=K + 8,
             ldc=N + shift + ldc_extra, c_off=c_off, r_off=c_off, a_sparse=a_sparse, twin=twin, a_rows=span(a_map), c_rows=span(c_map),
             gate_ld=N + 8, gate_rows=cdiv(M, rps) if rps else 0)
    c["ldr"] = c["ldc"]
    many = groups > 1
    c.update(a_gstride=c["a_rows"] * c["lda"] + 64 if many else 0, w_gstride=N * c["ldw"] + 64 if many else 0, bias_gstride=N + 8 if many else 0,
             c_gstride=c["c_rows"] * c["ldc"] + 64 if many else 0, gate_gstride=c["gate_rows"] * c["gate_ld"] + 16 if many else 0)
    c["r_gstride"] = c["c_gstride"]
    return c


_KT = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 20, 33)      # the K-tile-count classes of test_gemm256_every_k_tile_count_class_...
GEMM_CASES = [
    # persistent rounds: tiles > CUs, ragged rims in a late round, sample boundaries strictly inside tiles under RES_GATE, R aliased to C
    _case("rounds3 32x18 tiles, rps 300, R = C", (256, 3, 1, 0, 3), 8000, 4360, 256, RG, rps=300, alias=True),
    _case("rounds2 19x17 tiles ragged, rps 100", (256, 2, 1, 0, 3), 4678, 4120, 192, RG, rps=100),
    _case("rounds2 rps 1000, C map splits tiles, R = C", (256, 2, 1, 0, 1), 4678, 4120, 128, RG, rps=1000, c_map=(1000, 1010), alias=True),
    # split-K tail behind full rounds: tiles % CUs in (0, CUs / 2], >= 96 K-tiles
    _case("tail 16 of 272, bias", (256, 2, 8, 16, 3), 4296, 4096, 6144, B, path_nows=(256, 2, 1, 0, 3)),
    _case("tail 5 of 261, gelu", (256, 2, 8, 8, 3), 2304, 7424, 6144, G, path_nows=(256, 2, 1, 0, 3)),
    _case("tail 14 of 270, res_gate rps 1000, R = C, 97 K-tiles", (256, 2, 8, 16, 3), 4608, 3840, 6208, RG, path_nows=(256, 2, 1, 0, 3), rps=1000,
          alias=True),
    _case("tail 8 of 264, res_scale", (256, 2, 8, 8, 3), 3000, 5632, 6144, RS, path_nows=(256, 2, 1, 0, 3)),
    _case("tail 14 of 270, column split", (256, 2, 8, 16, 3), 2304, 7680, 6144, G, path_nows=(256, 2, 1, 0, 3), split=(3072, 264)),
    _case("tail 122 of 378, 2 slices, no bias", (256, 2, 2, 128, 3), 4608, 5376, 6144, B, path_nows=(256, 2, 1, 0, 3), bias=False),
    # split-K in the small-M regime: tiles < CUs, K = 6144 ... 15360 (without the workspace these go to the 128^2 kernel)
    _case("small-M 24 tiles K 12288, res_gate", (256, 1, 8, 24, 3), 512, 3072, 12288, RG, path_nows=(128, 1, 1, 0, 0), rps=256),
    _case("small-M 48 tiles ragged M, no bias", (256, 1, 5, 48, 3), 1000, 3072, 12288, B, path_nows=(128, 1, 1, 0, 0), bias=False),
    _case("small-M 72 tiles K 15360, A row map, res_gate", (256, 1, 3, 72, 3), 1536, 3072, 15360, RG, path_nows=(128, 1, 1, 0, 0), rps=512,
          a_map=(512, 520)),
    _case("small-M 24 tiles K 6144", (256, 1, 8, 24, 3), 512, 3072, 6144, B, path_nows=(128, 1, 1, 0, 0)),
    # epilogue access forms on the 256^2 kernel
    _case("narrow epilogue: N % 8 == 4", (256, 2, 1, 0, 2), 4096, 4100, 128, RS, ldc_extra=4),
    _case("narrow epilogue: ldc % 8 == 4", (256, 1, 1, 0, 2), 4096, 4096, 128, G, ldc_extra=4),
    _case("narrow epilogue: C / R base 8 bytes off, R = C", (256, 1, 1, 0, 2), 4096, 4096, 128, RG, rps=500, c_off=4, alias=True),
    _case("row map per tile: c_rpb % 256 == 0", (256, 1, 1, 0, 3), 4096, 4096, 128, RG, rps=1024, c_map=(1024, 1032)),
    _case("row map per row: c_rpb % 256 != 0", (256, 1, 1, 0, 1), 4096, 4096, 128, RG, rps=1000, c_map=(1000, 1032)),
    # groups, strides larger than the operands, a per-row gate
    _case("3 groups on the 128^2 kernel", (128, 1, 1, 0, 0), 150, 520, 128, RG, groups=3, rps=1),
    _case("6 groups on the 256^2 kernel", (256, 1, 1, 0, 3), 300, 520, 192, RG, groups=6, rps=1),
    _case("2 groups, res_scale, R = C", (256, 1, 1, 0, 3), 300, 1032, 64, RS, groups=2, alias=True),
    _case("4 groups x 72 tiles > CUs", (256, 2, 1, 0, 3), 2304, 2048, 128, B, groups=4),
    _case("2 groups UG_EPI_F32", (256, 1, 1, 0, 3), 300, 520, 128, EF, groups=2),
    # UG_EPI_F32 on both kernels, with and without bias
    _case("f32 out, 256^2, bias", (256, 1, 1, 0, 3), 300, 520, 192, EF),
    _case("f32 out, 128^2, no bias", (128, 1, 1, 0, 0), 150, 260, 64, EF, bias=False),
    _case("f32 out, 2 rounds", (256, 2, 1, 0, 3), 4608, 3840, 128, EF),
    # A row maps
    _case("A map monotonic, batch jumps inside a tile", (256, 1, 1, 0, 3), 4000, 4096, 128, B, a_map=(100, 117)),
    _case("A map broadcasting -> 128^2", (128, 1, 1, 0, 0), 2000, 1024, 128, G, a_map=(500, 0)),
    _case("A tile spans 2^31 bytes -> 128^2", (128, 1, 1, 0, 0), 200, 260, 64, B, lda=4210760, a_sparse=True, twin=False),
] + [_case(f"{nk} K-tiles, ragged 17x17 tiles", (256, 2, 1, 0, 3), 4166, 4120, 64 * nk, RG if nk % 2 else B, rps=1000 if nk % 2 else 0) for nk in _KT]


def _large(c):
    return c["M"] * c["N"] * c["K"] * c["groups"] > FULL_TRUTH_MACS


def case_rows(c, i):
    """the logical rows case i is judged on in fp64"""
    if not _large(c):
        return torch.arange(c["M"])
    return FR.sample_rows(c["M"], boundaries=(c["rows_per_sample"], c["a_map"][0], c["c_map"][0]), seed=i)


def gemm_operands(c, seed, dev, dt=BF):
    """flat operand buffers of a case (values bf16-representable, stored as dt): a, w, bias, gate, residual (None when R aliases C) and the C
    buffer before the call: 7.0 everywhere (PAD elements before the base and after the end), with the residual's values at the logical elements
    when R aliases C. The C buffer has the output's element type."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda n, s=1.0: (torch.randn(n, generator=g, device=dev) * s).to(BF)
    G_ = c["groups"]
    if c["a_sparse"]:                                    # a very wide lda: uninitialised, only the K columns filled
        a = torch.empty(c["a_rows"] * c["lda"], device=dev, dtype=BF)
        a.view(c["a_rows"], c["lda"])[:, :c["K"]] = rn(c["a_rows"] * c["K"]).view(c["a_rows"], c["K"])
    else:
        a = rn(G_ * c["a_gstride"] if G_ > 1 else c["a_rows"] * c["lda"])
    w = rn(G_ * c["w_gstride"] if G_ > 1 else c["N"] * c["ldw"], c["K"] ** -0.5)
    bias = rn(G_ * c["bias_gstride"] if G_ > 1 else c["N"], 0.1) if c["has_bias"] else None
    gate = rn(G_ * c["gate_gstride"] if G_ > 1 else c["gate_rows"] * c["gate_ld"]) if c["epilogue"] == RG else None
    span = G_ * c["c_gstride"] if G_ > 1 else c["c_rows"] * c["ldc"]
    res = c["epilogue"] in (RG, RS)
    cbuf = torch.full((PAD + c["c_off"] + span + PAD,), SENT, device=dev, dtype=F32 if c["epilogue"] == EF else BF)
    r = None
    if res and c["alias"]:
        dest = FR.gemm_dest(torch.arange(c["M"], device=dev), **c) + PAD + c["c_off"]
        cbuf[dest.reshape(-1)] = rn(dest.numel())
    elif res:
        r = rn(c["r_off"] + span)
    conv = lambda t: None if t is None else (t if dt == BF or t.numel() > 1 << 28 else t.to(dt))
    return dict(a=conv(a), w=conv(w), bias=conv(bias), gate=conv(gate), r=conv(r), c0=cbuf if dt == BF or c["epilogue"] == EF else cbuf.to(dt))


def gemm_reference(c, o, rows):
    """fwd_ref.gemm on a case's operands -> (exact, variant) [groups, len(rows), N]"""
    if c["epilogue"] in (RG, RS):
        R = o["c0"][PAD + c["c_off"]:] if c["alias"] else o["r"][c["r_off"]:]
    else:
        R = None
    return FR.gemm(o["a"], o["w"], o["bias"], rows=rows, residual=R, gate=o["gate"], **c)


def _desc(L, c, o, cbuf, ws):
    es = cbuf.element_size()
    ies = o["a"].element_size()
    d = L.GemmDesc()
    d.A, d.lda, d.a_rpb, d.a_bstride = o["a"].data_ptr(), c["lda"], *c["a_map"]
    d.W, d.ldw = o["w"].data_ptr(), c["ldw"]
    d.bias = None if o["bias"] is None else o["bias"].data_ptr()
    d.C, d.ldc, d.c_rpb, d.c_bstride = cbuf.data_ptr() + (PAD + c["c_off"]) * es, c["ldc"], *c["c_map"]
    if c["epilogue"] in (RG, RS):
        d.R = d.C if c["alias"] else o["r"].data_ptr() + c["r_off"] * ies
        d.ldr, d.r_rpb, d.r_bstride = c["ldr"], *c["r_map"]
    if o["gate"] is not None:
        d.gate, d.gate_ld, d.rows_per_sample = o["gate"].data_ptr(), c["gate_ld"], c["rows_per_sample"]
    d.alpha, d.epilogue = c["alpha"], c["epilogue"]
    d.M, d.N, d.K, d.groups = c["M"], c["N"], c["K"], c["groups"]
    for k in ("a_gstride", "w_gstride", "bias_gstride", "c_gstride", "r_gstride", "gate_gstride", "gelu_from_n", "c_shift_from_n", "c_shift"):
        setattr(d, k, c[k])
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    return d


def _ulp_far(got, screen):
    """elements of `got` more than one bf16 ulp of the screen's value away from it"""
    s = screen.float()
    _, e = torch.frexp(s.abs())
    ulp = torch.ldexp(torch.ones_like(s), e - 8)            # |s| = m 2^e, m in [0.5, 1): 2^(floor(log2 |s|) - 7)
    return (got.float() - s).abs() > torch.where(s == 0, torch.zeros_like(s), ulp)


def screen(c, o, unrounded):
    """the full-output screen of a large case (one group): torch's fp32 matmul with the reference's epilogue steps in torch ops -> [M, N] fp32;
    unrounded: no bf16 step (the fp32 twin's screen, and the form checked against the fp64 truth)"""
    dev = o["a"].device
    m = torch.arange(c["M"], device=dev)
    cols = torch.arange(c["N"], device=dev)
    rb = (lambda t: t) if unrounded else (lambda t: t.to(BF).float())
    A = o["a"].view(-1)[(FR.rowmap(m, *c["a_map"]) * c["lda"])[:, None] + torch.arange(c["K"], device=dev)[None, :]].float()
    W = o["w"].view(c["N"], c["ldw"])[:, :c["K"]].float()
    v = A @ W.t()
    if o["bias"] is not None:
        v = v + o["bias"].float()[None, :c["N"]]
    v = rb(v)
    if c["epilogue"] == G:
        y = rb(torch.nn.functional.gelu(v, approximate="tanh"))
        return torch.where((cols >= c["gelu_from_n"])[None, :], y, v)
    if c["epilogue"] in (RG, RS):
        rsrc = o["c0"][PAD + c["c_off"]:] if c["alias"] else o["r"][c["r_off"]:]
        R = rsrc[(FR.rowmap(m, *c["r_map"]) * c["ldr"])[:, None] + cols[None, :]].float()
        t = o["gate"][((m // c["rows_per_sample"]) * c["gate_ld"])[:, None] + cols[None, :]].float() * v if c["epilogue"] == RG else \
            torch.tensor(c["alpha"], dtype=F32, device=dev) * v
        return rb(R + rb(t))
    return v


def _row_err(got, ref):
    return (got.double() - ref.double()).norm(dim=-1) / ref.double().norm(dim=-1)


def _gemm_child():
    """runs in a child process with UG_ENV_DYNAMIC=1 (UG_GEMM_FORCE_TILE is read per call): every GEMM_CASES entry; one JSON record per case"""
    from unigen_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    ws = torch.zeros(int(lib.ug_gemm_workspace_bytes()), dtype=torch.uint8, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for i, c in enumerate(GEMM_CASES):
        rec = dict(case=i, name=c["name"], ncu=ncu, path=list(FR.gemm_path(c, ncu)), path_nows=list(FR.gemm_path(c, ncu, workspace=False)), fail=[])
        fail = rec["fail"]
        rows = case_rows(c, i)
        o = gemm_operands(c, 7000 + i, dev)
        exact, var = gemm_reference(c, o, rows)
        all_rows = torch.arange(c["M"], device=dev)
        dest_all = (FR.gemm_dest(all_rows, **c) + PAD + c["c_off"])
        written = torch.zeros(o["c0"].numel(), dtype=torch.bool, device=dev)
        written[dest_all.reshape(-1)] = True
        dest = dest_all[:, rows.to(dev)]
        tail = FR.tail_from(rows, c["M"])
        f32_out = c["epilogue"] == EF
        keep = {k: (v.clone() if v.numel() <= 1 << 28 else v.view(c["a_rows"], c["lda"])[:, :c["K"]].clone()) for k, v in o.items()
                if v is not None and k != "c0"}

        def run(ops_, fn, force, with_ws):
            os.environ["UG_GEMM_FORCE_TILE"] = str(force)
            cb = ops_["c0"].clone()
            d = _desc(L, c, ops_, cb, ws if with_ws else None)
            rc = fn(C.byref(d), stream())
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"case {i} ({c['name']}) force {force}: code {rc}: {lib.ug_last_error()}")
            if not bool((cb[~written] == SENT).all()):
                fail.append(f"force {force} ws {with_ws}: written outside its rows / columns")
            return cb

        def judged(tag, cb, v):
            k, b, ok = FR.judge(cb[dest].cpu(), exact, var=v, rows_from=tail)
            rec[tag], rec[tag + "_bound"] = k, b
            if not ok:
                fail.append(f"{tag}: {k} above {b}")

        bf_var = None if f32_out else var
        split = rec["path"][2] > 1
        outs = {"128": run(o, lib.ug_gemm_bf16, 128, True), "0": run(o, lib.ug_gemm_bf16, 0, True)}
        if FR.gemm_path(c, ncu, force=256, workspace=False)[0] == 256:
            outs["256u"] = run(o, lib.ug_gemm_bf16, 256, False)
            if not torch.equal(outs["256u"], outs["128"]):
                fail.append("the 128^2 and the unsplit 256^2 kernel differ")
        judged("k128", outs["128"], bf_var)
        if split:
            judged("split", outs["0"], bf_var)
            for _ in range(2):
                if not torch.equal(run(o, lib.ug_gemm_bf16, 0, True), outs["0"]):
                    fail.append("the split-K result is not bitwise repeatable")
            if not torch.equal(run(o, lib.ug_gemm_bf16, 0, False), outs["128"]):
                fail.append("without the workspace: differs from the unsplit kernels")
        elif not torch.equal(outs["0"], outs["128"]):
            fail.append("the dispatcher's own choice differs from the 128^2 kernel")
        if not bool((ws[:4096] == 0).all()):
            fail.append("arrival tickets not left at zero")
        o32 = t32 = None
        if c["twin"]:
            o32 = gemm_operands(c, 7000 + i, dev, F32)
            os.environ["UG_GEMM_FORCE_TILE"] = "0"
            t32 = run(o32, lib.ug_gemm_f32, 0, False)
            judged("f32", t32, None)
        if _large(c):
            assert c["groups"] == 1
            lg = lambda cb: cb[dest_all[0]]
            su = screen(c, o, True)
            rec["screen"] = FR.err(su[rows.to(dev)].cpu(), exact[0])[0]
            if not rec["screen"] <= 1e-5:
                fail.append(f"the screen itself is {rec['screen']} from the fp64 truth")
            if t32 is not None:
                rec["f32_screen_row"] = float(_row_err(lg(t32), su).max())
                if not rec["f32_screen_row"] <= FR.F32_ROW:
                    fail.append(f"fp32 twin: a row {rec['f32_screen_row']} from the screen")
            sr = su if f32_out else screen(c, o, False)
            for tag in ("128", "0") if split else ("128",):
                got = lg(outs[tag])
                re_ = float(_row_err(got, sr).max())
                bound = FR.F32_ROW if f32_out else rec["k128_bound"][1]
                rec["screen_row_" + tag] = (re_, bound)
                if not re_ <= bound:
                    fail.append(f"force {tag}: a row {re_} from the screen (bound {bound}), row {int(_row_err(got, sr).argmax())}")
                if not f32_out:
                    share = float(_ulp_far(got, sr).float().mean())
                    rec["share_" + tag] = share
                    if not share <= SHARE_BOUND:
                        fail.append(f"force {tag}: {share} of the elements more than one bf16 ulp from the screen")
            if c["K"] >= 15360 and t32 is not None:     # the twin's figure at the longest K next to torch's CPU fp32 matmul on the same rows
                A = FR._flat_rows(o["a"], FR.rowmap(rows, *c["a_map"]) * c["lda"], c["K"])
                W = FR._flat_rows(o["w"], torch.arange(c["N"]) * c["ldw"], c["K"])
                rec["torch_cpu_f32_matmul"] = FR.err((A.float() @ W.float().t()).double(), A @ W.t())[:2]
        for k, v in keep.items():
            now = o[k] if o[k].numel() <= 1 << 28 else o[k].view(c["a_rows"], c["lda"])[:, :c["K"]]
            if not torch.equal(now, v):
                fail.append(f"read-only operand {k} changed")
        print("GEMM " + json.dumps(rec), flush=True)
        del o, o32, outs, t32, written, dest_all, keep
    os.environ.pop("UG_GEMM_FORCE_TILE", None)


def test_gemm_dispatch_paths(gpu):
    env = dict(os.environ, UG_ENV_DYNAMIC="1")
    p = subprocess.run([sys.executable, "-c", "from tests.test_fuzz_gemm_gpu import _gemm_child; _gemm_child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    recs = [json.loads(l[5:]) for l in p.stdout.splitlines() if l.startswith("GEMM ")]
    bad = []
    for r in recs:
        c = GEMM_CASES[r["case"]]
        print(f"gemm case {r['case']} [{c['name']}] M {c['M']} N {c['N']} K {c['K']} epi {c['epilogue']} groups {c['groups']} path {r['path']}: " +
              "; ".join(f"{k} {v}" for k, v in r.items() if k not in ("case", "name", "path", "fail", "ncu")))
        if tuple(r["path"]) != c["path"] or (c["path_nows"] and tuple(r["path_nows"]) != c["path_nows"]):
            bad.append((c["name"], f"on {r['ncu']} CUs this case takes path {r['path']} / {r['path_nows']} without workspace, not {c['path']} / {c['path_nows']}"))
        bad += [(c["name"], f) for f in r["fail"]]
    print(p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-4000:]
    assert len(recs) == len(GEMM_CASES)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_adaln_modulate: generic, fast (D = 1536 / 3072 / 4096, also through the generic kernel), fp32 twin
# ----------------------------------------------------------------------------------------------------------------------------------
ADALN_D = (64, 200, 520, 1536, 1544, 3072, 4096)
ADALN_MEANS = (0.0, 4.0, 16.0, 64.0)          # row means in standard deviations
ADALN_TWIN_MAX_MEAN = 64.0                     # torch's own fp32 F.layer_norm stays inside 1e-5 / 1e-4 up to here (test_fwd_ref_cpu.py measures it)
ADALN_CASES = [   # D, rows, rows per sample (1: per-token modulation), x row map, ldx - D, ldo - D, scale = -1 in sample 0
    (64, 1, 1, (0, 0), 0, 0, False), (64, 4099, 1000, (0, 0), 8, 8, False), (200, 37, 1, (0, 0), 8, 0, False), (200, 130, 50, (65, 70), 0, 8, True),
    (520, 1027, 1027, (0, 0), 0, 0, False), (520, 6, 3, (3, 5), 24, 8, False), (1536, 5, 5, (0, 0), 0, 0, False), (1536, 1027, 1, (0, 0), 8, 8, False),
    (1536, 130, 65, (65, 70), 512, 8, True), (1544, 37, 37, (0, 0), 0, 0, False), (1544, 130, 1, (0, 0), 8, 8, True), (3072, 4099, 1024, (0, 0), 0, 0, False),
    (3072, 37, 1, (37, 40), 8, 8, False), (3072, 2, 1, (0, 0), 0, 8, True), (4096, 1027, 300, (500, 510), 8, 0, False), (4096, 7, 1, (0, 0), 0, 0, False),
]


def adaln_data(case, seed, dt):
    """x [physical rows, ldx], modulation [samples, 2 D + 8] (shift | scale, mod_ld = 2 D + 8) as float64 holding dt values. Logical row i: mean
    ADALN_MEANS[i % 4] standard deviations (standard deviation log-uniform in [0.1, 10]); i % 7 == 4: one channel 100 x the rest;
    i % 7 == 5: a constant row (3, -0.5 or 64: the fp32 row sum is exact, so LayerNorm is exactly 0 and the output must be `shift`)."""
    D, rows, rps, xmap, ex, eo, m1 = case
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(rows)
    phys = FR.rowmap(r, *xmap)
    xb = torch.randn(int(phys.max()) + 1, D + ex, generator=g, dtype=F64)
    sd = torch.exp(torch.empty(rows, 1, dtype=F64).uniform_(-2.3, 2.3, generator=g))
    mean = torch.tensor(ADALN_MEANS, dtype=F64)[r % 4][:, None]
    x = (torch.randn(rows, D, generator=g, dtype=F64) + mean) * sd
    big = (r % 7 == 4).nonzero().flatten()
    x[big, (big * 13) % D] *= 100.0
    const = (r % 7 == 5).nonzero().flatten()
    x[const] = torch.tensor([3.0, -0.5, 64.0], dtype=F64)[const % 3][:, None]
    xb[phys, :D] = x
    samples = (rows + rps - 1) // rps
    mod = 0.5 * torch.randn(samples, 2 * D + 8, generator=g, dtype=F64)
    if m1:
        mod[0, D:2 * D] = -1.0
    rd = lambda t: t.to(dt).to(F64)
    return rd(xb), rd(mod), const


def _adaln_kw(case):
    D, rows, rps, xmap, ex, eo, m1 = case
    return dict(rows=rows, D=D, rows_per_sample=rps, mod_ld=2 * D + 8, ldx=D + ex, x_map=xmap)


def _adaln_child():
    """child process with UG_ENV_DYNAMIC=1: every ADALN_CASES entry in bf16 (the fast widths also with UG_ADALN_FAST=0) and through the fp32 twin"""
    from unigen_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for i, case in enumerate(ADALN_CASES):
        D, rows, rps, xmap, ex, eo, m1 = case
        kw = _adaln_kw(case)
        rec = dict(case=i, fail=[])
        for dt, fn, modes in ((BF, lib.ug_adaln_modulate, ("1", "0") if D in (1536, 3072, 4096) else ("1",)), (F32, lib.ug_adaln_modulate_f32, ("1",))):
            xb, mod, const = adaln_data(case, 9000 + i, dt)
            exact, var = FR.adaln_modulate(xb, mod, mod.reshape(-1)[D:], **kw)
            xd, md = xb.to(dt).to(dev), mod.to(dt).to(dev)
            ldo = D + eo
            for fast in modes:
                os.environ["UG_ADALN_FAST"] = fast
                ob = torch.full((PAD + rows * ldo + PAD,), SENT, device=dev, dtype=dt)
                rc = fn(xd.data_ptr(), D + ex, xmap[0], xmap[1], md.data_ptr(), md.data_ptr() + D * md.element_size(), 2 * D + 8, rps,
                        ob.data_ptr() + PAD * ob.element_size(), ldo, rows, D, 1e-6, stream())
                torch.cuda.synchronize()
                if rc != 0:
                    raise RuntimeError(f"adaln case {i}: code {rc}: {lib.ug_last_error()}")
                body = ob[PAD:PAD + rows * ldo].view(rows, ldo)
                if not (bool((ob[:PAD] == SENT).all()) and bool((ob[PAD + rows * ldo:] == SENT).all()) and bool((body[:, D:] == SENT).all())):
                    rec["fail"].append(f"{dt} fast {fast}: written outside its rows / columns")
                got = body[:, :D].cpu()
                sh = mod[torch.arange(rows) // rps, :D]
                if not torch.equal(got[const].to(F64), sh[const]):
                    rec["fail"].append(f"{dt} fast {fast}: a constant row is not `shift` exactly")
                tag = ("bf16" if dt == BF else "f32") + ("" if fast == "1" else "_generic")
                k, b, ok = FR.judge(got, exact, var=var if dt == BF else None, rows_from=(rows - 1) // 4 * 4)
                rec[tag], rec[tag + "_bound"] = k, b
                if not ok:
                    rec["fail"].append(f"{tag}: {k} above {b}")
            if not (torch.equal(xd.cpu().to(F64), xb) and torch.equal(md.cpu().to(F64), mod)):
                rec["fail"].append(f"{dt}: a read-only operand changed")
        print("ADALN " + json.dumps(rec), flush=True)
    os.environ.pop("UG_ADALN_FAST", None)


def test_adaln_modulate_sweep(gpu):
    env = dict(os.environ, UG_ENV_DYNAMIC="1")
    p = subprocess.run([sys.executable, "-c", "from tests.test_fuzz_gemm_gpu import _adaln_child; _adaln_child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    recs = [json.loads(l[6:]) for l in p.stdout.splitlines() if l.startswith("ADALN ")]
    bad = []
    for r in recs:
        print(f"adaln case {r['case']} {ADALN_CASES[r['case']]}: " + "; ".join(f"{k} {v}" for k, v in r.items() if k not in ("case", "fail")))
        bad += [(ADALN_CASES[r["case"]], f) for f in r["fail"]]
    print(p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-4000:]
    assert len(recs) == len(ADALN_CASES)
    assert not bad, bad


def test_adaln_modulate_refusals_write_nothing(gpu):
    """D above 4096, D not a multiple of 8, a base 8 bytes off a 16-byte boundary: each returns its code and leaves the output untouched"""
    from unigen_amd import lib as L
    lib = L.load()
    x = torch.randn(8, 4200, device=gpu).to(BF)
    mod = torch.randn(2, 8416, device=gpu).to(BF)
    st = torch.cuda.current_stream().cuda_stream
    for fn, dt in ((lib.ug_adaln_modulate, BF), (lib.ug_adaln_modulate_f32, F32)):
        xd, md = x.to(dt), mod.to(dt)
        es = xd.element_size()
        off = 8 // es                                                    # elements that move a base 8 bytes
        for what, code, D, dx, dm, do in (("D = 4104", L.UG_ERR_UNSUPPORTED, 4104, 0, 0, 0), ("D = 100", L.UG_ERR_UNSUPPORTED, 100, 0, 0, 0),
                                          ("x 8 bytes off", L.UG_ERR_BAD_ALIGN, 64, off, 0, 0), ("shift 8 bytes off", L.UG_ERR_BAD_ALIGN, 64, 0, off, 0),
                                          ("out 8 bytes off", L.UG_ERR_BAD_ALIGN, 64, 0, 0, off)):
            out = torch.full((8 * 4200,), SENT, device=gpu, dtype=dt)
            rc = fn(xd.data_ptr() + dx * es, 4200, 0, 0, md.data_ptr() + dm * es, md.data_ptr() + (4208 + dm) * es, 8416, 4, out.data_ptr() + do * es,
                    4200, 8, D, 1e-6, st)
            torch.cuda.synchronize()
            assert rc == code, (what, dt, rc, code)
            assert bool((out == SENT).all()), (what, dt, "wrote to the output")


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_small_linear_bf16
# ----------------------------------------------------------------------------------------------------------------------------------
_SL_M, _SL_N, _SL_K = (1, 2, 3, 15, 16, 17, 33, 64), (8, 24, 1000, 1032, 6152), (8, 512, 520, 4096)
# M, N, K, SiLU on the input, bias, residual: every M with every N; every K with every N and with four of the M
SMALL_LINEAR_CASES = [(M, _SL_N[(i + j) % 5], _SL_K[(i + 2 * j) % 4], (i + j) % 3 != 0, (i * 5 + j) % 4 != 0, (i + j) % 2 == 0)
                      for i, M in enumerate(_SL_M) for j in range(5)]


def small_linear_data(case, seed):
    """x [M, K + 8] N(0, 3) with entries at +-30, +-20, +-10 (the SiLU's exp2 argument saturates), W [N, K + 16] N(0, 1 / K), bias [N], R [M, N + 8];
    float64 holding bf16 values"""
    M, N, K, act, has_b, has_r = case
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(M, K + 8, generator=g, dtype=F64)
    ext = torch.tensor([30.0, -30.0, 20.0, -20.0, 10.0, -10.0, 0.0, -5.0], dtype=F64)
    xs = x[:, :K].clone()
    idx = torch.arange(0, M * K, 5)
    xs.view(-1)[idx] = ext[(idx // 5) % 8]
    x[:, :K] = xs
    w = torch.randn(N, K + 16, generator=g, dtype=F64) * K ** -0.5
    b = 0.1 * torch.randn(N, generator=g, dtype=F64) if has_b else None
    r = torch.randn(M, N + 8, generator=g, dtype=F64) if has_r else None
    rd = lambda t: None if t is None else FR.bf16(t)
    return rd(x), rd(w), rd(b), rd(r)


def _small_linear_check(name, case, ob, exact, var, ldo):
    M, N = case[0], case[1]
    body = ob[PAD:PAD + M * ldo].view(M, ldo)
    assert bool((ob[:PAD] == SENT).all()) and bool((ob[PAD + M * ldo:] == SENT).all()) and bool((body[:, N:] == SENT).all()), (name, "written outside its rows / columns")
    k, b, ok = FR.judge(body[:, :N].cpu(), exact, var=var, rows_from=(M - 1) // 16 * 16)
    print(f"{name} {case}: rel-L2 {k[0]:.3e} ({b[0]:.3e}) worst row {k[1]:.3e} ({b[1]:.3e}) last chunk {k[2]:.3e} ({b[2]:.3e})")
    assert ok, (name, case, k, b)


@pytest.mark.parametrize("i", range(len(SMALL_LINEAR_CASES)))
def test_small_linear_bf16_sweep(gpu, i):
    from unigen_amd import ops
    case = SMALL_LINEAR_CASES[i]
    M, N, K, act, has_b, has_r = case
    x, w, b, r = small_linear_data(case, 11000 + i)
    exact, var = FR.small_linear_bf16(x, w, b, M=M, N=N, K=K, act_in=int(act), residual=r, ldx=K + 8, ldw=K + 16, ldr=N + 8)
    d = lambda t: None if t is None else t.to(BF).to(gpu)
    xd, wd, bd, rd = d(x), d(w), d(b), d(r)
    ldo = N + 8
    ob = torch.full((PAD + M * ldo + PAD,), SENT, device=gpu, dtype=BF)
    out = ob[PAD:PAD + M * ldo].view(M, ldo)[:, :N]
    ops.small_linear(xd[:, :K], wd[:, :K], bd, out, silu_in=act, residual=None if rd is None else rd[:, :N])
    torch.cuda.synchronize()
    _small_linear_check("small_linear", case, ob, exact, var, ldo)
    for t, t0 in ((xd, x), (wd, w), (bd, b), (rd, r)):
        assert t is None or torch.equal(t.cpu().to(F64), t0), "a read-only operand changed"


def test_small_linear_bf16_c_abi_and_refusal(gpu):
    """one M <= 16 call straight through the C ABI (M = 13: MT = 16 with three idle rows; N = 1000: the last wave's 8 columns straddle N), and
    M = 17 refused with nothing written"""
    from unigen_amd import lib as L
    lib = L.load()
    case = (13, 1000, 520, True, True, True)
    M, N, K = case[:3]
    x, w, b, r = small_linear_data(case, 12000)
    exact, var = FR.small_linear_bf16(x, w, b, M=M, N=N, K=K, act_in=1, residual=r, ldx=K + 8, ldw=K + 16, ldr=N + 8)
    xd, wd, bd, rd = (t.to(BF).to(gpu) for t in (x, w, b, r))
    ldo = N + 8
    st = torch.cuda.current_stream().cuda_stream
    ob = torch.full((PAD + 17 * ldo + PAD,), SENT, device=gpu, dtype=BF)
    rc = lib.ug_small_linear_bf16(xd.data_ptr(), K + 8, wd.data_ptr(), K + 16, bd.data_ptr(), rd.data_ptr(), N + 8, ob.data_ptr() + 2 * PAD, ldo, 17, N, K, 1, st)
    torch.cuda.synchronize()
    assert rc == L.UG_ERR_UNSUPPORTED and bool((ob == SENT).all())
    rc = lib.ug_small_linear_bf16(xd.data_ptr(), K + 8, wd.data_ptr(), K + 16, bd.data_ptr(), rd.data_ptr(), N + 8, ob.data_ptr() + 2 * PAD, ldo, M, N, K, 1, st)
    torch.cuda.synchronize()
    assert rc == 0, lib.ug_last_error()
    _small_linear_check("small_linear C ABI", case, ob[:PAD + M * ldo + PAD], exact, var, ldo)
    assert bool((ob[PAD + M * ldo:] == SENT).all())
