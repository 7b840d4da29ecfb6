"""Kernels at the top of their index ranges (tests/index_range_cases.py; docs/PARITY_TOLERANCES.md, "Index-range sweep"): row strides at the
largest admitted value, batch strides that put a sample past byte offset 2^32, the 4096^2 canvas' key count at head width 512, convolution
geometries just outside the limits of the packed-coordinate route, convolutions and GroupNorm on activations that cross 2^31 and 2^32 bytes.

Far views: operands carved out of one arena (torch.empty, at most 12 GiB) at huge strides, the first of them 2^31 bytes into it, only the
elements a kernel may read written, 64 sentinel elements behind every output row. Every far launch must give the bits of the same values
launched at compact strides, and the compact launch is first judged against float64 with the judging functions of the existing sweeps
(tests/test_fuzz_backward_gpu._check for attention, tests/attn_wide_ref.bounds at head width 512, tests/vae_kernel_ref for the convolution),
unchanged - so "equal to garbage" cannot pass. No test relies on a fault: an offset cut to 32 bits lands inside the arena and shows as wrong
values. Every test prints its peak device memory; none may hold more than 16 GiB."""
import pytest
import torch

from tests import attn_wide_ref as WR
from tests import bwd_ref as BR
from tests import index_range_cases as IC
from tests import vae_kernel_ref as VR
from tests.test_fuzz_backward_gpu import _check, _pad64, _tail
from tests.test_fuzz_vae_gpu import _conv_judge, _conv_once

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENT = 3.0                                                 # exact in bf16
F32_TOTAL, F32_ROW = 1e-5, 1e-4


@pytest.fixture(scope="module")
def arena(gpu):
    """the module's one arena, in bytes: nothing in it is initialised, and it is freed when the module's last test is done"""
    torch.cuda.empty_cache()
    need = max([2 * IC.attn_arena_elems(c) for c in IC.ATTN_FAR_CASES + IC.ATTN_BATCH_CASES] +
               [IC.wide_arena_bytes(c, s) for c in IC.WIDE_FAR_CASES for s in (2, 4)])
    assert need <= 12 * IC.GIB, need
    a = torch.empty(need, dtype=torch.uint8, device=gpu)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _memory(gpu):
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory {peak / IC.GIB:.2f} GiB")
    assert peak <= IC.MEMORY_CAP, peak


def _st():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_gemm_bf16: one child process (UG_GEMM_FORCE_TILE is read per call only under UG_ENV_DYNAMIC=1) with an arena of its own. These tests come
# first in the module: the child has come and gone before the parent's arena exists, so the two never add up.
# ----------------------------------------------------------------------------------------------------------------------------------
def _gemm_far_child():
    """every case of index_range_cases.gemm_far_cases() under UG_GEMM_FORCE_TILE = 128 and 0: the compact descriptor judged against float64 by
    fwd_ref.judge, then the far descriptor on the same values - bit-identical, sentinels intact; one JSON record per case"""
    import ctypes as C
    import json
    import os
    from tests import fwd_ref as FR
    from tests.test_fuzz_gemm_gpu import PAD, _desc, gemm_operands, gemm_reference
    from tests.test_fuzz_gemm_gpu import SENT as GSENT
    from unigen_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    ws = torch.zeros(int(lib.ug_gemm_workspace_bytes()), dtype=torch.uint8, device=dev)
    arena = torch.empty(IC.GEMM_ARENA_BYTES // 2, dtype=BF, device=dev)
    for i, k in enumerate(IC.gemm_far_cases()):
        c, far = k["base"], k["far"]
        rec = dict(case=i, name=k["name"], ncu=ncu, path=list(FR.gemm_path(far, ncu)), path128=list(FR.gemm_path(far, ncu, force=128)), fail=[])
        fail = rec["fail"]
        o = gemm_operands(c, 7300 + i, dev)
        rows = torch.arange(c["M"])
        exact, var = gemm_reference(c, o, rows)
        dest = FR.gemm_dest(rows.to(dev), **c) + PAD + c["c_off"]                  # [groups, M, N] into the compact C buffer
        written = torch.zeros(o["c0"].numel(), dtype=torch.bool, device=dev)
        written[dest.reshape(-1)] = True
        lay = IC.gemm_far_layout(far)
        fo = {}
        for op in ("a", "w", "bias", "gate", "r"):
            if o[op] is None:
                fo[op] = None
                continue
            G, nrows, width = IC.gemm_operand_shape(c, op)
            gstride, ldim = IC.gemm_operand_strides(c, op)
            IC.gemm_far_view(arena, far, lay, op).copy_(o[op].as_strided((G, nrows, width), (gstride, ldim, 1), c["r_off"] if op == "r" else 0))
            fo[op] = arena[lay[op] - (c["r_off"] if op == "r" else 0):]
        cview = IC.gemm_far_view(arena, far, lay, "c", IC.SENT_COLS)
        fo["c0"] = arena[lay["c"] - PAD - c["c_off"]:]                              # _desc adds PAD + c_off to this buffer's address
        for force in (128, 0):
            os.environ["UG_GEMM_FORCE_TILE"] = str(force)
            cb = o["c0"].clone()
            rc = lib.ug_gemm_bf16(C.byref(_desc(L, c, o, cb, ws)), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"case {i} compact, force {force}: code {rc}: {lib.ug_last_error()}")
            if not bool((cb[~written] == GSENT).all()):
                fail.append(f"force {force}: the compact launch wrote outside its rows / columns")
            fig, bound, ok = FR.judge(cb[dest].cpu(), exact, var=var)
            rec[f"compact_{force}"], rec[f"bound_{force}"] = fig, bound
            if not ok:
                fail.append(f"force {force}: the compact launch {fig} above {bound}")
            cview.fill_(GSENT)
            if c["alias"]:
                cview[..., :c["N"]].copy_(o["c0"][dest])
            rc = lib.ug_gemm_bf16(C.byref(_desc(L, far, fo, fo["c0"], ws)), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"case {i} far, force {force}: code {rc}: {lib.ug_last_error()}")
            if not bool((cview[..., c["N"]:] == GSENT).all()):
                fail.append(f"force {force}: the sentinels behind the far C rows were overwritten")
            diff = int((cview[..., :c["N"]] != cb[dest]).sum())
            rec[f"differ_{force}"] = diff
            if diff:
                fail.append(f"force {force}: {diff} elements of the far launch differ from the compact launch")
            if not bool((ws[:4096] == 0).all()):
                fail.append(f"force {force}: arrival tickets not left at zero")
        for op in ("a", "w", "bias", "gate", "r"):                                   # read-only operands unchanged
            if fo[op] is not None:
                G, nrows, width = IC.gemm_operand_shape(c, op)
                gstride, ldim = IC.gemm_operand_strides(c, op)
                if not torch.equal(IC.gemm_far_view(arena, far, lay, op), o[op].as_strided((G, nrows, width), (gstride, ldim, 1), c["r_off"] if op == "r" else 0)):
                    fail.append(f"read-only operand {op} of the far launch changed")
        rec["peak_gib"] = torch.cuda.max_memory_allocated() / IC.GIB
        print("GEMMFAR " + json.dumps(rec), flush=True)
    os.environ.pop("UG_GEMM_FORCE_TILE", None)


@pytest.fixture(scope="module")
def gemm_far(gpu):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() + IC.GEMM_ARENA_BYTES + IC.GIB <= IC.MEMORY_CAP, "the child's arena beside what this process holds"
    p = subprocess.run([sys.executable, "-c", "from tests.test_index_range_gpu import _gemm_far_child; _gemm_far_child()"], cwd=root,
                       env=dict(os.environ, UG_ENV_DYNAMIC="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]                 # not restarted: the exit code is the failure
    return {r["case"]: r for r in (json.loads(l[8:]) for l in p.stdout.splitlines() if l.startswith("GEMMFAR "))}


GEMM_FAR = IC.gemm_far_cases()


@pytest.mark.parametrize("i", range(len(GEMM_FAR)), ids=[k["name"].replace(" ", "_") for k in GEMM_FAR])
def test_gemm_with_operands_past_4_gib(gemm_far, i):
    """C, R (apart and aliased), W, the gate, the bias and A past byte offset 2^32 from their bases, by group stride or leading dimension, on the
    128^2 and the 256^2 kernel (one case with a split-K tail, one whose ldw must send it to the 128^2 kernel)"""
    from tests import fwd_ref as FR
    k, r = GEMM_FAR[i], gemm_far[i]
    print(f"gemm far case {i} [{k['name']}]: " + "; ".join(f"{n} {v}" for n, v in r.items() if n not in ("case", "name", "fail")))
    assert r["peak_gib"] * IC.GIB <= IC.MEMORY_CAP
    assert tuple(r["path"]) == FR.gemm_path(k["far"], 256) == k["base"]["path"], ("on this chip the far descriptor takes another path", r["path"], r["ncu"])
    assert tuple(r["path128"]) == (128, 1, 1, 0, 0)
    assert (r["path"][2] > 1) == k["split"]
    assert not r["fail"], r["fail"]


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_flash_attn_fwd, ug_flash_attn_fwd_lse, ug_flash_attn_bwd
# ----------------------------------------------------------------------------------------------------------------------------------
def _attention_launches(lib, L, c, ptr, rs, bs, lse):
    """-> the four launches as callables: forward without and with the LSE, backward with that LSE and with lse = NULL, on operands ptr[name] with
    the strides rs[name], bs[name]"""
    B, H, dh, Lq, Lkv = c["B"], c["H"], c["dh"], c["Lq"], c["Lkv"]
    scale = dh ** -0.5
    a = lambda *names: [v for n in names for v in (ptr[n], rs[n], bs[n])]
    ws = torch.empty(int(lib.ug_flash_attn_bwd_workspace_bytes(B, H, Lq)), device=lse.device, dtype=torch.uint8)
    steps = {}

    def fwd():
        L.check(lib.ug_flash_attn_fwd(*a("q", "k", "v", "o"), B, H, Lq, Lkv, dh, scale, _st()), "ug_flash_attn_fwd")

    def fwd_lse():
        L.check(lib.ug_flash_attn_fwd_lse(*a("q", "k", "v", "o"), B, H, Lq, Lkv, dh, scale, lse.data_ptr(), lse.shape[2], _st()), "ug_flash_attn_fwd_lse")

    def bwd(with_lse):
        L.check(lib.ug_flash_attn_bwd(*a("q", "k", "v", "o", "do", "dq", "dk", "dv"), B, H, Lq, Lkv, dh, scale, lse.data_ptr() if with_lse else None,
                                      ws.data_ptr(), ws.numel(), _st()), "ug_flash_attn_bwd")
    steps.update(fwd=fwd, fwd_lse=fwd_lse, bwd_lse=lambda: bwd(True), bwd_none=lambda: bwd(False))
    return steps


def _attention_run(dev, c, views, data):
    """views: name -> [B, rows, D + SENT_COLS] device view (inputs: only [..., :D] is written). Runs the four launches; -> dict of host copies of
    o (plain forward), o_lse, lse, and dq / dk / dv of both backward modes, with every output's sentinel columns checked."""
    from unigen_amd import lib as L
    lib = L.load()
    B, H, Lq, D = c["B"], c["H"], c["Lq"], c["H"] * c["dh"]
    for n in ("q", "k", "v", "do"):
        views[n][..., :D].copy_(data[n])
    ptr = {n: v.data_ptr() for n, v in views.items()}
    rs = {n: v.stride(1) for n, v in views.items()}
    bs = {n: v.stride(0) for n, v in views.items()}
    lse = torch.full((B, H, _pad64(Lq)), -77.0, device=dev, dtype=F32)
    steps = _attention_launches(lib, L, c, ptr, rs, bs, lse)
    out = {}

    def take(names, tag):
        torch.cuda.synchronize()
        for n in names:
            assert bool((views[n][..., D:] == SENT).all()), (f"{n}: the sentinel behind its rows was overwritten", tag, c["name"])
            out[n + tag] = views[n][..., :D].cpu()
            views[n].fill_(SENT)

    for n in IC.ATTN_OUTPUTS:
        views[n].fill_(SENT)
    steps["fwd"]()
    take(["o"], "")
    steps["fwd_lse"]()
    torch.cuda.synchronize()
    assert bool((views["o"][..., D:] == SENT).all()), ("o: the sentinel behind its rows was overwritten", "lse", c["name"])
    out["o_lse"] = views["o"][..., :D].cpu()                   # stays in place: the backward reads it
    assert bool((lse[..., Lq:] == -77.0).all()), ("forward wrote LSE rows beyond Lq", c["name"])
    lse[..., Lq:] = 0.0
    out["lse"] = lse.cpu()
    steps["bwd_lse"]()
    take(["dq", "dk", "dv"], "_lse")
    steps["bwd_none"]()
    take(["dq", "dk", "dv"], "_none")
    return out


def _attention_case(dev, arena, c):
    B, H, dh, Lq, Lkv = c["B"], c["H"], c["dh"], c["Lq"], c["Lkv"]
    D = H * dh
    g = torch.Generator().manual_seed(c["seed"])
    data = {n: torch.randn(B, IC.attn_rows(c, n), D, generator=g).to(BF) for n in ("q", "k", "v", "do")}
    dev_data = {n: t.to(dev) for n, t in data.items()}
    # compact launch. K | V of one buffer where the far launch takes the buffer-form DMAs (head width 64), else two buffers of unequal row
    # strides (the pointer form): the compact launch runs the far launch's kernel
    W = D + IC.SENT_COLS
    new = lambda rows, w=W: torch.empty(B, rows + 1, w, dtype=BF, device=dev)[:, :rows]
    compact = {n: new(IC.attn_rows(c, n)) for n in IC.ATTN_OPERANDS if n not in ("k", "v")}
    if dh == 128 or IC.bufd_ok(c["rs"], c["rs"], Lkv):
        KV = new(Lkv, 2 * W)
        compact["k"], compact["v"] = KV[..., :W], KV[..., W:]
    else:
        compact["k"], compact["v"] = new(Lkv), new(Lkv, W + 8)[..., :W]
    if dh == 64:
        assert IC.bufd_ok(compact["k"].stride(1), compact["v"].stride(1), Lkv) == IC.bufd_ok(c["rs"], c["rs"], Lkv), "the compact launch takes another DMA form"
    near = _attention_run(dev, c, compact, dev_data)
    # (b) the compact launch against float64, by the backward sweep's judge
    heads = lambda t, rows: t.reshape(B, rows, H, dh).transpose(1, 2).double()
    ref = BR.attention(heads(data["q"], Lq), heads(data["k"], Lkv), heads(data["v"], Lkv), heads(data["do"], Lq), dh ** -0.5, o=heads(near["o_lse"], Lq),
                       lsum_bf16=dh == 64, fwd_tile=None)
    assert torch.equal(near["o"], near["o_lse"]), ("ug_flash_attn_fwd and ug_flash_attn_fwd_lse differ", c["name"])
    _check("compact forward O", heads(near["o_lse"], Lq), ref["O"], c, var=ref["O_r"], rows_from=_tail(Lq))
    for mode in ("lse", "none"):
        for n, rows in (("dq", Lq), ("dk", Lkv), ("dv", Lkv)):
            _check(f"compact bwd[{mode}] {n}", heads(near[f"{n}_{mode}"], rows), ref[n], dict(c, mode=mode), var=ref[n + "_r"], mag=ref.get(n + "_m"),
                   rows_from=_tail(rows))
    # (a) the far launch: the same bits
    el = arena.view(BF)
    far_views = {n: IC.far_view(el, off, c["rs"], c["bs"], B, IC.attn_rows(c, n), W) for n, off in IC.attn_layout(c).items()}
    far = _attention_run(dev, c, far_views, dev_data)
    for n in near:
        assert torch.equal(far[n], near[n]), (f"{n} at row stride {c['rs']}, batch stride {c['bs']} differs from the compact launch", c["name"],
                                              int((far[n] != near[n]).sum()), "elements")


@pytest.mark.parametrize("c", IC.ATTN_FAR_CASES, ids=lambda c: c["name"])
def test_attention_at_the_largest_row_stride(gpu, arena, c):
    """q, k, v, o, dout, dq, dk, dv at row stride 2^24 - 16, batch 1 past byte offset 2^32: forward (with and without the LSE) and backward (with the
    forward's LSE and without). Head width 64: Lkv = 64 is the last length on the buffer-form DMAs at this stride, 65 the first on the pointer form"""
    assert c["rs"] == IC.ATTN_RS_FAR and 2 * c["bs"] >= 1 << 32
    _attention_case(gpu, arena, c)


@pytest.mark.parametrize("c", IC.ATTN_BATCH_CASES, ids=lambda c: c["name"])
def test_attention_with_the_last_batch_past_4_gib(gpu, arena, c):
    """compact rows, a batch stride above 2^31 elements: batch 0 of every operand below byte offset 2^32, batch 1 beyond it"""
    assert 2 * c["bs"] >= 1 << 32 and c["rs"] < 4096
    _attention_case(gpu, arena, c)


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_flash_attn_fwd_wide and its fp32 twin
# ----------------------------------------------------------------------------------------------------------------------------------
def _wide_launch(fn, c, views, scale):
    from unigen_amd import lib as L
    args = [v for n in "qkv" for v in (views[n].data_ptr(), views[n].stride(1), views[n].stride(0))]
    o = views["o"]
    L.check(fn(*args, o.data_ptr(), o.stride(1), o.stride(0), c["B"], c["H"], c["Lq"], c["Lkv"], WR.DH, scale, _st()), "ug_flash_attn_fwd_wide")
    torch.cuda.synchronize()
    assert bool((o[..., WR.DH:] == SENT).all()), ("the sentinel behind the output rows was overwritten", c["name"])
    return o[..., :WR.DH].cpu()


@pytest.mark.parametrize("c", IC.WIDE_FAR_CASES, ids=lambda c: c["name"])
def test_wide_attention_at_the_largest_kv_row_stride(gpu, arena, c):
    """head width 512, K / V (and Q, O) at row stride 2^24 - 8, batch 1 past byte offset 2^32 of the arena (from the operand's base: 2^31 in bf16,
    2^32 in fp32); one whole 32-key tile, one key more, two tiles and a ragged third. The bf16 kernel, then the fp32 twin at the same stride in
    its own elements."""
    from unigen_amd import lib as L
    lib = L.load()
    B, Lq, Lkv, scale = c["B"], c["Lq"], c["Lkv"], WR.DH ** -0.5
    g = torch.Generator().manual_seed(c["seed"])
    data = {n: torch.randn(B, Lkv if n in "kv" else Lq, WR.DH, generator=g).to(BF) for n in "qkv"}
    h = lambda t: t.reshape(B, -1, 1, WR.DH).transpose(1, 2)                    # [B, 1, L, 512]
    ref = WR.reference(h(data["q"]), h(data["k"]), h(data["v"]), scale)
    W = WR.DH + IC.SENT_COLS
    for dt, fn in ((BF, lib.ug_flash_attn_fwd_wide), (F32, lib.ug_flash_attn_fwd_wide_f32)):
        size = torch.empty(0, dtype=dt).element_size()
        rows = lambda n: Lkv if n in "kv" else Lq
        near = {n: torch.empty(B, rows(n) + 1, W, dtype=dt, device=gpu)[:, :rows(n)] for n in "qkvo"}
        lay = IC.wide_layout(c, size)
        far = {n: IC.far_view(arena.view(dt), lay[n], c["rs"], c["bs"], B, rows(n), W) for n in "qkvo"}
        assert size * far["k"].stride(0) >= 1 << 31 and far["k"].data_ptr() + size * far["k"].stride(0) - arena.data_ptr() >= 1 << 32
        got = []
        for views in (near, far):
            for n in "qkv":
                views[n][..., :WR.DH].copy_(data[n].to(gpu))
            views["o"].fill_(SENT)
            got.append(_wide_launch(fn, c, views, scale))
        total, worst, _ = BR.err(h(got[0]), ref["O"])
        b_total, b_row = WR.bounds(ref) if dt == BF else (F32_TOTAL, F32_ROW)
        print(f"{c['name']} {str(dt)[6:]} compact: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
        assert total <= b_total and worst <= b_row, (c["name"], dt, total, worst)
        assert torch.equal(got[1], got[0]), (f"row stride {c['rs']} differs from the compact launch", c["name"], dt, int((got[1] != got[0]).sum()))


def test_wide_attention_over_the_keys_of_a_4096_canvas(gpu):
    """Lkv = 262 144, the mid block of a 4096^2 decode, 130 queries: against attn_wide_ref with its own bound (the variant walks the same 8192
    tiles, so its error carries whatever the key count does to the kernel's)"""
    from unigen_amd import lib as L
    lib = L.load()
    c = IC.WIDE_CANVAS
    g = torch.Generator().manual_seed(c["seed"])
    q = torch.randn(1, 1, c["Lq"], WR.DH, generator=g).to(BF)
    k = torch.randn(1, 1, c["Lkv"], WR.DH, generator=g).to(BF)
    v = torch.randn(1, 1, c["Lkv"], WR.DH, generator=g).to(BF)
    scale = WR.DH ** -0.5
    views = {n: t[0].to(gpu) for n, t in (("q", q), ("k", k), ("v", v))}
    views["o"] = torch.full((1, c["Lq"], WR.DH + IC.SENT_COLS), SENT, dtype=BF, device=gpu)
    got = _wide_launch(lib.ug_flash_attn_fwd_wide, c, views, scale)[None]
    ref = WR.reference(q, k, v, scale)
    b_total, b_row = WR.bounds(ref)
    total, worst, _ = BR.err(got, ref["O"])
    print(f"{c['name']}: rel-L2 {total:.3e} (bound {b_total:.3e}), worst row {worst:.3e} ({b_row:.3e})")
    assert bool(torch.isfinite(got).all()) and total <= b_total and worst <= b_row, (total, b_total, worst, b_row)


# ----------------------------------------------------------------------------------------------------------------------------------
# convolution geometries just outside the packed-coordinate route (the cases inside it: vae_kernel_ref.CONV256_CASES, run on both kernels by
# tests/test_fuzz_vae_gpu.py::test_conv2d_on_the_256_route)
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(IC.CONV256_OUTSIDE)))
def test_conv2d_just_outside_the_256_route(gpu, i):
    """W = 2048 with Wo = 4096, and B = 256: conv_takes_256 is false, the 128^2 kernel and the fp32 twin take the call"""
    c = IC.CONV256_OUTSIDE[i]
    assert not VR.conv_takes_256(c), c
    for dt in (BF, F32):
        _conv_judge(f"conv2d {str(dt)[6:]} outside the 256^2 route, case {i}", _conv_once(c, dt, gpu, c["Cin"], c["Cout"]), c)


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_adaln_modulate and the row-wise glue kernels: the last row of every strided operand past byte offset 2^32
# ----------------------------------------------------------------------------------------------------------------------------------
def _flat_index(off, phys_rows, ld, width, dev):
    """[rows, width] element indices of rows `phys_rows` of leading dimension `ld` in a flat buffer"""
    return (off + phys_rows.to(dev) * ld)[:, None] + torch.arange(width, device=dev)[None, :]


@pytest.mark.parametrize("case", IC.ADALN_FAR_CASES, ids=lambda c: f"D{c[0]}-{c[1]}rows-{c[3] or 'ld'}")
def test_adaln_modulate_with_rows_past_4_gib(gpu, arena, case):
    """the fast kernel (D 1536, 3072) and the generic one (D 520): ldx and ldo large enough for the last row to start past byte offset 2^32, or
    compact rows under an x row map whose batch stride does the same. The compact launch is judged by the GEMM sweep's AdaLN judge
    (fwd_ref.judge against fwd_ref.adaln_modulate); the far launch must give its bits."""
    from tests import fwd_ref as FR
    from tests.test_fuzz_gemm_gpu import adaln_data
    from unigen_amd import lib as L
    lib = L.load()
    D, rows, rps, how = case
    geo = IC.adaln_far_geometry(case)
    cmap = (0, 0) if how is None else (geo["x_map"][0], geo["x_map"][0] + 5)
    compact = (D, rows, rps, cmap, 8, 8, False)
    xb, mod, const = adaln_data(compact, 9400 + D + rows, BF)
    exact, var = FR.adaln_modulate(xb, mod, mod.reshape(-1)[D:], rows=rows, D=D, rows_per_sample=rps, mod_ld=2 * D + 8, ldx=D + 8, x_map=cmap)
    xd, md = xb.to(BF).to(gpu), mod.to(BF).to(gpu)
    r = torch.arange(rows)
    el = arena.view(BF)
    W = D + IC.SENT_COLS

    def launch(x_ptr, ldx, x_map, out):
        out.fill_(SENT)
        L.check(lib.ug_adaln_modulate(x_ptr, ldx, x_map[0], x_map[1], md.data_ptr(), md.data_ptr() + 2 * D, 2 * D + 8, rps, out.data_ptr(), out.stride(0),
                                      rows, D, 1e-6, _st()), "ug_adaln_modulate")
        torch.cuda.synchronize()
        assert bool((out[:, D:] == SENT).all()), ("the sentinel behind the output rows was overwritten", case)
        return out[:, :D].cpu()

    near = launch(xd.data_ptr(), D + 8, cmap, torch.empty(rows + 1, W, dtype=BF, device=gpu)[:rows])
    fig, bound, ok = FR.judge(near, exact, var=var, rows_from=(rows - 1) // 4 * 4)
    print(f"adaln {case} compact: {fig} (bounds {bound})")
    assert ok, (case, fig, bound)
    x_off, o_off = IC.ARENA_BASE, IC.ARENA_BASE + 200000            # the output rows start behind a compact batch of x rows
    phys = FR.rowmap(r, *geo["x_map"])
    IC.assert_disjoint([(x_off + int(p_) * geo["ldx"], x_off + int(p_) * geo["ldx"] + D) for p_ in phys] + [(o_off + k * geo["ldo"], o_off + k * geo["ldo"] + W) for k in range(rows)])
    assert 2 * int(phys.max()) * geo["ldx"] >= 1 << 32 and 2 * (rows - 1) * geo["ldo"] >= 1 << 32
    logical = xd.view(-1)[_flat_index(0, FR.rowmap(r, *cmap), D + 8, D, gpu)]                  # [rows, D]
    rpb = geo["x_map"][0] or rows
    assert rows % rpb == 0
    xfar = el.as_strided((rows // rpb, rpb, D), ((geo["x_map"][1] or rows) * geo["ldx"], geo["ldx"], 1), x_off)
    xfar.copy_(logical.view(rows // rpb, rpb, D))
    far = launch(el[x_off:].data_ptr(), geo["ldx"], geo["x_map"], IC.far_view(el, o_off, geo["ldo"], 0, 1, rows, W)[0])
    assert torch.equal(xfar.reshape(rows, D), logical), "the far x changed"
    bad = (far != near).any(1).nonzero().flatten().tolist()
    assert not bad, (case, geo, "rows that differ from the compact launch", bad, int((far != near).sum()))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_glue_kernels_with_rows_past_4_gib(gpu, arena, dt):
    """ug_add_bf16, ug_add_rowbcast_f32, ug_gather_rows (source and output stride) and ug_transpose (source ld, and source batch stride) with the
    last row of every strided operand past byte offset 2^32: these kernels are exact, so each far result is compared bit for bit with
    tests/step_kernel_ref.py; 64 sentinel elements behind every output row"""
    from tests import step_kernel_ref as SR
    from unigen_amd import ops
    size = torch.empty(0, dtype=dt).element_size()
    rows, D = IC.GLUE_FAR_ROWS[size], IC.GLUE_FAR_D
    ld = IC.far_ld(rows, size)
    assert size * (rows - 1) * ld >= 1 << 32
    el = arena.view(dt)
    base = (1 << 31) // size + 4096
    W = D + IC.SENT_COLS
    view = lambda k: el.as_strided((rows, W), (ld, 1), base + 1024 * k)          # interleaved in the same rows, 1024 columns apart
    assert base + 3 * 1024 + (rows - 1) * ld + W <= el.numel() and W <= 1024 < ld
    g = torch.Generator().manual_seed(6600 + size)
    a, b = torch.randn(rows, D, generator=g).to(dt), torch.randn(rows, D, generator=g).to(dt)
    A, B_, O = view(0), view(1), view(2)

    def ready():
        A[:, :D].copy_(a.to(gpu)); B_[:, :D].copy_(b.to(gpu)); O.fill_(SENT)

    def taken(name, want):
        torch.cuda.synchronize()
        assert bool((O[:, D:] == SENT).all()), (name, "the sentinel behind the output rows was overwritten")
        assert torch.equal(O[:, :D].cpu(), want), (name, "differs from the exact reference", int((O[:, :D].cpu() != want).sum()))

    ready()
    ops.add(A[:, :D], B_[:, :D], O[:, :D])
    taken("ug_add_bf16", SR.add(a, b))
    if dt == BF:                                            # in place on bf16 rows, the table fp32 and compact
        rpb = 130
        table = torch.randn(rpb, D, generator=g)
        ready()
        O[:, :D].copy_(a.to(gpu))
        ops.add_rowbcast_f32(O[:, :D], table.to(gpu), rpb)
        taken("ug_add_rowbcast_f32", SR.add_rowbcast(a, table, rpb))
    idx = torch.randint(-1, rows, (rows,), generator=g, dtype=torch.int32)
    idx[:4] = torch.tensor([rows - 1, 0, -1, rows - 1], dtype=torch.int32)
    ready()
    ops.gather_rows(A[:, :D], idx.to(gpu), O[:, :D])
    taken("ug_gather_rows", SR.gather_rows(a, idx))
    # transpose: the source's row stride far; then compact rows and a far batch stride
    ready()
    got = ops.transpose(A[:, :D], rows_pad=rows + 8)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), SR.transpose(a[None], rows + 8)[0]), "ug_transpose, far source ld"
    nb, rb = 4, rows // 4
    bstride = -(-(1 << 32) // (size * (nb - 1))) // 8 * 8 + 8
    src = el.as_strided((nb, rb, D), (bstride, D + 8, 1), base)
    assert size * (nb - 1) * bstride >= 1 << 32 and base + (nb - 1) * bstride + rb * (D + 8) <= el.numel()
    src.copy_(a[:nb * rb].reshape(nb, rb, D).to(gpu))
    got = ops.transpose(src, rows_pad=rb + 3)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), SR.transpose(a[:nb * rb].reshape(nb, rb, D), rb + 3)), "ug_transpose, far source batch stride"


# ----------------------------------------------------------------------------------------------------------------------------------
# the 128^2 convolution kernel and the fp32 twin at large-canvas layers: tensors that cross 2^31 and 2^32 bytes
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IC.CONV_WINDOW_CASES, ids=lambda c: c["name"].split(" at ")[0].split(",")[0].replace(" ", "_"))
def test_conv2d_at_large_canvas_sizes(gpu, arena, c):
    """One launch on activations of several GiB drawn on the device (seeded per 256-row chunk: nothing periodic), then (1) windows of output rows
    - the first, the last, those on either side of byte offsets 2^31 and 2^32 of the input and of the output - against float64 with the
    convolution sweep's judge, and (2) every output element bit for bit against the same kernel replayed band by band, each band a problem
    of 256 output rows with its own small input and output: a row displaced in the large launch differs from its band."""
    from unigen_amd import ops
    dt = F32 if c["f32"] else BF
    es = 4 if c["f32"] else 2
    H, W, Cin, Cout, st, pad = c["H"], c["W"], c["Cin"], c["Cout"], c["stride"], c["pad"]
    Ho, Wo = IC.conv_window_out(c)
    BH = IC.CONV_BAND_ROWS
    el = arena.view(dt)
    nx, no = H * W * Cin, Ho * Wo * Cout
    guard = Wo * Cout
    assert (nx + no + 2 * guard) * es <= arena.numel()
    x, out_all = el[:nx].view(H * W, Cin), el[nx:nx + guard + no + guard]
    out = out_all[guard:guard + no].view(Ho * Wo, Cout)
    kw = dict(B=1, W=W, Wo=Wo, KH=3, KW=3, stride=st, pad_l=pad, up=0)

    def chunk(t, rows_per, i, seed):                     # rows [i rows_per, (i + 1) rows_per) of t [rows, width, C], N(0, 1) from their own seed
        sl = t[i * rows_per:(i + 1) * rows_per]
        sl.normal_(generator=torch.Generator(device=gpu).manual_seed(seed + i))
        return sl

    x3 = x.view(H, W, Cin)
    for i in range(-(-H // BH)):
        chunk(x3, BH, i, c["seed"] * 1000)
    g = torch.Generator().manual_seed(c["seed"])
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * (9 * Cin) ** -0.5).to(dt)
    b = (0.3 * torch.randn(Cout, generator=g)).to(dt)
    wd, bd = w.to(gpu), b.to(gpu)
    alias = c["res"] == "alias"
    out_all.fill_(SENT)
    o3 = out.view(Ho, Wo, Cout)

    def residual(i, into):                                # chunk i of the residual the output buffer holds before the call
        return chunk(into, BH, i, c["seed"] * 1000 + 500)
    if alias:
        for i in range(-(-Ho // BH)):
            residual(i, o3)
    ops.conv2d_nhwc(x, wd, bd, out, H=H, Ho=Ho, pad_t=pad, residual=out if alias else None, **kw)
    torch.cuda.synchronize()
    assert bool((out_all[:guard] == SENT).all()) and bool((out_all[guard + no:] == SENT).all()), ("written outside its [Ho Wo, Cout] rows", c["name"])
    # (2) the band screen
    band_out = torch.empty(BH + 1, Wo, Cout, dtype=dt, device=gpu)
    bad = []
    for i in range(-(-Ho // BH)):
        y0, y1 = i * BH, min((i + 1) * BH, Ho)
        bnd = IC.conv_band(c, y0, y1)
        ob = band_out[:y1 - y0]
        band_out.fill_(SENT)
        if alias:
            ob.normal_(generator=torch.Generator(device=gpu).manual_seed(c["seed"] * 1000 + 500 + i))
        ops.conv2d_nhwc(x3[bnd["x0"]:bnd["x1"]].view(-1, Cin), wd, bd, ob.view(-1, Cout), H=bnd["H"], Ho=bnd["Ho"], pad_t=bnd["pad_t"],
                        residual=ob.view(-1, Cout) if alias else None, **kw)
        torch.cuda.synchronize()
        assert bool((band_out[y1 - y0:] == SENT).all())
        rows_bad = (ob != o3[y0:y1]).any(-1).any(-1).nonzero().flatten()
        bad += [y0 + int(r) for r in rows_bad[:4]]
    assert not bad, (c["name"], "output rows of the large launch that differ from their band's replay", bad[:16])
    # (1) the windows against float64
    for y0, y1 in IC.conv_windows(c):
        bnd = IC.conv_band(c, y0, y1)
        xh = x3[bnd["x0"]:bnd["x1"]].cpu()[None]
        Rh = None
        if alias:                                          # regenerate the chunks that hold these rows
            tmp = torch.empty(BH, Wo, Cout, dtype=dt, device=gpu)
            rows = []
            for i in range(y0 // BH, (y1 - 1) // BH + 1):
                n = min((i + 1) * BH, Ho) - i * BH
                tmp[:n].normal_(generator=torch.Generator(device=gpu).manual_seed(c["seed"] * 1000 + 500 + i))
                rows.append(tmp[max(y0 - i * BH, 0):min(y1 - i * BH, n)].cpu())
            Rh = torch.cat(rows)[None]
        truth, var, border = VR.conv2d(xh, w, b, Rh, Ho=y1 - y0, Wo=Wo, stride=st, pad_t=bnd["pad_t"], pad_l=pad, up=0)
        got = o3[y0:y1].cpu().to(torch.float64)[None]
        r = dict(guard=True, finite=bool(torch.isfinite(got).all()), m=VR.conv_metrics(got, truth, border),
                 b=VR.bounds(VR.conv_metrics(VR.bf16(var), truth, border), not c["f32"]),
                 mismatch=VR.mismatch(got, var) if alias else None)
        _conv_judge(f"{c['name']}, output rows [{y0}, {y1})", r, c)


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU) on more than 2^31 elements
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IC.GN_FAR_CASES, ids=lambda c: c["name"].replace(" ", "_"))
def test_groupnorm_past_4_gib(gpu, arena, c):
    """the fast pair (C 128, G 32, with SiLU) and the generic pair (C 64: never the fast pair's, with or without UG_GN_FAST) on one sample of
    more than 2^31 elements, drawn on the device per 2^18-row chunk, the last two chunks around another mean so that the tail of the tensor
    moves the statistics. Statistics: a chunked float64 reduction by torch on the device; windows (first rows, either side of byte offsets
    2^31 and 2^32, last rows): the float64 formula, judged with the GroupNorm sweep's metrics and bounds."""
    from unigen_amd import ops
    C, G, HW = c["C"], c["G"], c["HW"]
    assert VR.gn_fast(dict(C=C, G=G)) == (C == 128) and HW * C >= 1 << 31
    el = arena.view(BF)
    n = HW * C
    assert 2 * (2 * n + 2 * C * 64) <= arena.numel()
    x, out_all = el[:n].view(HW, C), el[n:n + (HW + 128) * C].view(HW + 128, C)
    out = out_all[64:64 + HW]
    CH = IC.GN_CHUNK_ROWS
    for i in range(-(-HW // CH)):
        sl = x[i * CH:(i + 1) * CH]
        sl.normal_(mean=IC.gn_chunk_mean(c, i), std=1.0, generator=torch.Generator(device=gpu).manual_seed(c["seed"] * 1000 + i))
    g = torch.Generator().manual_seed(c["seed"])
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).to(BF), (0.3 * torch.randn(C, generator=g)).to(BF)
    out_all.fill_(SENT)
    ops.groupnorm_nhwc(x, gamma.to(gpu), beta.to(gpu), out, B=1, HW=HW, groups=G, eps=c["eps"], silu=c["silu"])
    torch.cuda.synchronize()
    assert bool((out_all[:64] == SENT).all()) and bool((out_all[64 + HW:] == SENT).all()), ("written outside its [HW, C] rows", c["name"])
    mean, var = IC.group_stats_chunked(x, G, CH)
    head = IC.group_stats_chunked(x, G, CH, chunks=range(-(-HW // CH) - IC.GN_TAIL_CHUNKS))[0]
    assert float((mean - head).abs().min()) > 1e-3, "the tail chunks do not move the statistics"
    slab = 256 if C == 128 else 64
    for r0, r1 in IC.gn_windows(c):
        truth, v = IC.groupnorm_with_stats(x[r0:r1].cpu()[None], gamma, beta, G, c["eps"], c["silu"], mean, var)
        got = out[r0:r1].cpu().to(torch.float64)[None]
        assert bool(torch.isfinite(got).all())
        VR.judge(f"groupnorm {c['name']}, rows [{r0}, {r1})", VR.gn_metrics(got, truth, G, slab), VR.bounds(VR.gn_metrics(v, truth, G, slab), True), c)


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_qk_rmsnorm_rope, ug_small_linear_bf16, ug_qk_rmsnorm_rope_bwd, ug_adaln_modulate_bwd: strided operands past byte offset 2^32
# ----------------------------------------------------------------------------------------------------------------------------------
def test_qk_rmsnorm_rope_with_rows_past_4_gib(gpu, arena):
    """in place on q | k of a fused buffer: once with ld so large that the last row starts past byte offset 2^32, once with compact rows and a
    batch_stride_rows that puts the last batch there. Compact launch: fwd_ref.judge per head vector against fwd_ref.qk_rmsnorm_rope."""
    from tests import fwd_ref as FR
    from unigen_amd import ops
    q = IC.QK_FAR
    H, dh, B, L, W = q["heads"], q["dh"], q["batches"], q["rpb"], q["width"]
    HD, rows = H * dh, B * L
    g = torch.Generator().manual_seed(6900)
    buf = FR.bf16(torch.randn(rows, W, generator=g, dtype=torch.float64))
    wq, wk = FR.norm_weights(g, dh)[0], FR.norm_weights(g, dh)[0]
    ang = torch.rand(L + 7, dh // 2, generator=g) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    kw = dict(batches=B, rows_per_batch=L, q_off=0, k_off=HD, heads=H, dh=dh, pos_offset=7, split=0)
    exact, var = FR.qk_rmsnorm_rope(buf, wq_b=wq, wk_b=wk, cos=cos, sin=sin, **kw)
    dw = lambda t: t.to(BF).to(gpu)

    def launch(view, ld, bsr):                             # view [B, L, W]: q | k | sentinels
        view[..., :2 * HD].copy_(dw(buf[:, :2 * HD]).reshape(B, L, 2 * HD))
        view[..., 2 * HD:].fill_(SENT)
        ops.qk_rmsnorm_rope(view, ld=ld, batch_stride_rows=bsr, wq_b=dw(wq), wk_b=dw(wk), cos=cos.to(gpu), sin=sin.to(gpu), **kw)
        torch.cuda.synchronize()
        assert bool((view[..., 2 * HD:] == SENT).all()), "the sentinel behind q | k was overwritten"
        return view[..., :2 * HD].reshape(rows, 2 * HD).cpu()

    near = launch(torch.empty(B, L, W, dtype=BF, device=gpu), W, L)
    vec = lambda t: FR.qk_vectors(t.to(torch.float64), torch.arange(rows), 0, HD, H, dh)
    fig, bound, ok = FR.judge(vec(near), vec(exact), var=vec(var))
    print(f"qk_rmsnorm_rope compact: {fig} (bounds {bound})")
    assert ok, (fig, bound)
    el = arena.view(BF)
    for name, (ld, bsr) in IC.qk_far_geometries().items():
        assert 2 * ((B - 1) * bsr + L - 1) * ld >= 1 << 32
        far = launch(IC.far_view(el, IC.ARENA_BASE, ld, bsr * ld, B, L, W), ld, bsr)
        assert torch.equal(far, near), (name, ld, bsr, int((far != near).sum()), "elements differ from the compact launch")


def test_small_linear_with_rows_past_4_gib(gpu, arena):
    """x, residual and out with a row stride that puts row 47 past byte offset 2^32 (three launches of 16 rows, each from its own row pointer),
    W with a row stride that puts row 519 there. Compact launch: the small-linear sweep's judge."""
    from tests import fwd_ref as FR
    from tests.test_fuzz_gemm_gpu import small_linear_data
    from unigen_amd import ops
    case = IC.SMALL_LINEAR_FAR
    M, N, K, act, _, _ = case
    x, w, b, r = small_linear_data(case, 11900)
    exact, var = FR.small_linear_bf16(x, w, b, M=M, N=N, K=K, act_in=int(act), residual=r, ldx=K + 8, ldw=K + 16, ldr=N + 8)
    d = lambda t: t.to(BF).to(gpu)
    xd, wd, bd, rd = d(x)[:, :K], d(w)[:, :K], d(b), d(r)[:, :N]

    def launch(xv, wv, rv, ov):
        xv.copy_(xd); wv.copy_(wd); rv.copy_(rd); ov.fill_(SENT)
        ops.small_linear(xv, wv, bd, ov[:, :N], silu_in=act, residual=rv)
        torch.cuda.synchronize()
        assert bool((ov[:, N:] == SENT).all()), "the sentinel behind the output rows was overwritten"
        assert torch.equal(xv, xd) and torch.equal(wv, wd) and torch.equal(rv, rd), "a read-only operand changed"
        return ov[:, :N].cpu()

    e = lambda *s: torch.empty(*s, dtype=BF, device=gpu)
    near = launch(e(M, K + 8)[:, :K], e(N, K + 16)[:, :K], e(M, N + 8)[:, :N], e(M, N + IC.SENT_COLS))
    fig, bound, ok = FR.judge(near, exact, var=var, rows_from=(M - 1) // 16 * 16)
    print(f"small_linear compact: {fig} (bounds {bound})")
    assert ok, (fig, bound)
    el = arena.view(BF)
    ldm, ldw = IC.far_ld(M), IC.far_ld(N)
    b0 = IC.ARENA_BASE
    b1 = b0 + (M - 1) * ldm + 4096                           # W's rows start behind the last row of x | residual | out
    assert 2 * (M - 1) * ldm >= 1 << 32 and 2 * (N - 1) * ldw >= 1 << 32 and b1 + (N - 1) * ldw + K <= el.numel()
    sv = lambda off, rows, ld, width: el.as_strided((rows, width), (ld, 1), off)
    far = launch(sv(b0, M, ldm, K), sv(b1, N, ldw, K), sv(b0 + 1024, M, ldm, N), sv(b0 + 2048, M, ldm, N + IC.SENT_COLS))
    assert torch.equal(far, near), (int((far != near).sum()), "elements differ from the compact launch")


def test_backward_glue_kernels_with_rows_past_4_gib(gpu, arena):
    """ug_qk_rmsnorm_rope_bwd (x, dy) and ug_adaln_modulate_bwd (x, dy, and the scale's row stride) with the last row of each strided operand
    past byte offset 2^32; the outputs are the wrappers' own compact tensors. Compact launches: the backward sweep's judge."""
    from unigen_amd import ops
    el = arena.view(BF)
    g = torch.Generator().manual_seed(6950)
    sv = lambda off, rows, ld, width: el.as_strided((rows, width), (ld, 1), IC.ARENA_BASE + off)
    # q/k RMSNorm + RoPE backward
    H, dh, L, B = 2, 128, 100, 3
    HD, rows = H * dh, B * L
    xb, dyb = torch.randn(rows, HD, generator=g).to(BF), torch.randn(rows, HD, generator=g).to(BF)
    w = (1 + 0.2 * torch.randn(dh, generator=g)).to(BF)
    ang = torch.rand(5 + L, dh // 2, generator=g) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    run = lambda xv, dyv: ops.qk_rmsnorm_rope_bwd(xv, dyv, w.to(gpu), cos.to(gpu), sin.to(gpu), rows_per_batch=L, pos_offset=5, heads=H, dh=dh)
    dx, dwt = run(xb.to(gpu), dyb.to(gpu))
    torch.cuda.synchronize()
    ref_dx, ref_dw = BR.qk_rmsnorm_rope_bwd(xb, dyb, w, cos, sin, L, 5, H, dh)
    per_vec = lambda t: t.reshape(rows, H, dh).transpose(0, 1)
    _check("qk dx compact", per_vec(dx.cpu()), per_vec(ref_dx), "qk bwd", var=per_vec(BR.bf16(ref_dx)), rows_from=_tail(rows))
    _check("qk dw compact", dwt.cpu(), ref_dw, "qk bwd", var=BR.bf16(ref_dw))
    ld = IC.far_ld(rows)
    assert 2 * (rows - 1) * ld >= 1 << 32
    xv, dyv = sv(0, rows, ld, HD), sv(1024, rows, ld, HD)
    xv.copy_(xb.to(gpu)); dyv.copy_(dyb.to(gpu))
    fdx, fdw = run(xv, dyv)
    torch.cuda.synchronize()
    assert torch.equal(fdx, dx) and torch.equal(fdw, dwt), "ug_qk_rmsnorm_rope_bwd: the far launch differs from the compact launch"
    # AdaLN modulate backward
    a = IC.ADALN_BWD_FAR
    D, rps, S = a["D"], a["rps"], a["samples"]
    rows = rps * S
    xb, dyb = torch.randn(rows, D, generator=g).to(BF), torch.randn(rows, D, generator=g).to(BF)
    sc = (0.3 * torch.randn(S, D, generator=g)).to(BF)
    outs = ops.adaln_modulate_bwd(xb.to(gpu), dyb.to(gpu), sc.to(gpu), rows_per_sample=rps)
    torch.cuda.synchronize()
    refs = BR.adaln_modulate_bwd(xb, dyb, sc, rps)
    for name, got, ref, rf in zip(("dx", "d shift", "d scale"), outs, refs, (_tail(rows), None, None)):
        _check(f"adaln {name} compact", got.cpu(), ref, "adaln bwd", var=BR.bf16(ref), rows_from=rf)
    ld, lds = IC.far_ld(rows), IC.far_ld(S)
    assert 2 * (rows - 1) * ld >= 1 << 32 and 2 * (S - 1) * lds >= 1 << 32
    IC.assert_disjoint([(o + r * ld, o + r * ld + D) for o in (0, 2048) for r in range(rows)] + [(16384 + s * lds, 16384 + s * lds + D) for s in range(S)])
    xv, dyv, scv = sv(0, rows, ld, D), sv(2048, rows, ld, D), sv(16384, S, lds, D)
    xv.copy_(xb.to(gpu)); dyv.copy_(dyb.to(gpu)); scv.copy_(sc.to(gpu))
    fouts = ops.adaln_modulate_bwd(xv, dyv, scv, rows_per_sample=rps)
    torch.cuda.synchronize()
    for name, f, n_ in zip(("dx", "d shift", "d scale"), fouts, outs):
        assert torch.equal(f, n_), f"ug_adaln_modulate_bwd {name}: the far launch differs from the compact launch"
