"""What a kernel leaves behind for the next launch, and what it assumes about the scratch memory it is handed (include/unigen_hip.h states these
contracts; docs/PARITY_TOLERANCES.md, "Workspace and launch-state contracts: exact"). Every comparison is bitwise.

GEMM (ug_gemm_desc.workspace: "first 4096 bytes (arrival tickets) must be ZERO before the first call; every call leaves them zero again. The rest
needs no initialisation. One workspace per stream."): the launch sequence of tests/workspace_cases.py - split-K launches of 8, 5, 3 and 8 K-slices
over 24, 48, 72, 24 and 8 tail tiles with one unsplit launch in between - on ONE workspace whose slabs are poisoned (0xFF bytes: NaN; 0x7F bytes:
3.4e38), forwards and backwards; 16 times over without a synchronisation; on two streams at once; through ops.gemm under two streams; inside a
captured graph. Each case's baseline (its own fresh zeroed workspace, alone on the device) is first judged against the fp64 truth with the sweep's
judging function, so "bitwise equal to garbage" cannot pass.

The other workspaces (tests/workspace_cases.WORKSPACES): through the C ABI, guard regions round the workspace and every output, the workspace of
exactly the reported size pre-filled with zeros, 0xFF and 0x7F bytes, then shape a, shape b, shape a on one workspace; an undersized workspace is
refused before anything is launched (each host function read: the size check precedes every launch and every memset). The partial-sum outputs
the caller reduces are pre-filled with NaN: every row is written. The LSE padding of the attention backward is NaN on the product path.

No test here provokes a fault: poison goes only into memory the contract says needs no initialisation, every refusal is one the host code makes
before launching."""
import ctypes as C

import pytest
import torch

from tests import fwd_ref as FR
from tests import workspace_cases as WC
from tests.test_fuzz_gemm_gpu import GEMM_CASES, PAD, SENT, _desc, case_rows, gemm_operands, gemm_reference

pytestmark = pytest.mark.gpu
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
GUARD, PATTERN = 4096, 0xA5
FILLS = (0x00, 0xFF, 0x7F)


class Guarded:
    """`nbytes` of device memory, 256-byte aligned, pre-filled with `fill` bytes, with at least 4096 guard bytes of PATTERN on either side"""

    def __init__(self, nbytes, dev, fill=PATTERN):
        self.buf = torch.full((GUARD + 256 + nbytes + GUARD,), PATTERN, dtype=U8, device=dev)
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.n = nbytes
        self.mem = self.buf[self.off:self.off + nbytes]
        self.mem.fill_(fill)
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0

    def intact(self):
        return bool((self.buf[:self.off] == PATTERN).all()) and bool((self.buf[self.off + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


def _st():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------------------------------------------------------------
def _launch(S, i, ws, out=None, stream=None):
    """one ug_gemm_bf16 launch of GEMM_CASES[i] into `out` (a fresh copy of the case's C buffer when None) on `stream` (the current one)"""
    e = S["cases"][i]
    cb = e["o"]["c0"].clone() if out is None else out
    d = _desc(S["L"], e["c"], e["o"], cb, ws)
    rc = S["lib"].ug_gemm_bf16(C.byref(d), _st() if stream is None else stream)
    assert rc == 0, (e["c"]["name"], rc, S["lib"].ug_last_error())
    return cb


def _zero_ws(dev):
    return torch.zeros(WC.GEMM_WORKSPACE_BYTES, dtype=U8, device=dev)


@pytest.fixture(scope="module")
def gemm(gpu):
    """operands and the baseline of every case of the sequence: own fresh zeroed workspace, alone on the device, judged against the fp64 truth"""
    from unigen_amd import lib as L
    lib = L.load()
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    paths = [FR.gemm_path(GEMM_CASES[i], ncu) for i in WC.GEMM_SEQUENCE]
    pairs = [WC.slice_tail(p) for p in paths]
    ring = pairs + pairs[:1]
    assert len(set(pairs)) >= 3 and all(a != b for a, b in zip(ring, ring[1:])) and sum(n == 1 for n, _ in pairs) == 1, \
        f"on {ncu} CUs the sequence does not alternate between (K-slices, padded tail tiles): {pairs}"
    assert int(lib.ug_gemm_workspace_bytes()) == WC.GEMM_WORKSPACE_BYTES
    S = dict(lib=lib, L=L, ncu=ncu, cases={}, dev=gpu)
    for i, path in zip(WC.GEMM_SEQUENCE, paths):
        c = GEMM_CASES[i]
        assert WC.gemm_touched_bytes(path) <= WC.GEMM_WORKSPACE_BYTES
        o = gemm_operands(c, 7000 + i, gpu)
        S["cases"][i] = dict(c=c, o=o, path=path)
        torch.cuda.synchronize()
        ws = _zero_ws(gpu)
        base = _launch(S, i, ws)
        torch.cuda.synchronize()
        assert not bool(ws[:WC.TICKET_BYTES].any()), (c["name"], "arrival tickets not left at zero")
        assert bool(ws[4096:].any()) == (path[2] > 1), (c["name"], "a split launch writes slabs, an unsplit one does not touch the workspace")
        rows = case_rows(c, i)
        exact, var = gemm_reference(c, o, rows)
        dest_all = FR.gemm_dest(torch.arange(c["M"], device=gpu), **c) + PAD + c["c_off"]
        k, b, ok = FR.judge(base[dest_all[:, rows.to(gpu)]].cpu(), exact, var=var, rows_from=FR.tail_from(rows, c["M"]))
        print(f"baseline [{c['name']}] path {path}: rel-L2, worst row, worst tail row {k} (bounds {b})")
        assert ok, (c["name"], k, b)
        written = torch.zeros(base.numel(), dtype=torch.bool, device=gpu)
        written[dest_all.reshape(-1)] = True
        assert bool((base[~written] == SENT).all()), (c["name"], "written outside its rows / columns")
        S["cases"][i]["base"] = base
        del ws, written, dest_all
    return S


@pytest.mark.parametrize("fill", [0xFF, 0x7F], ids=["nan", "3.4e38"])
def test_gemm_shared_workspace_with_poisoned_slabs(gpu, gemm, fill):
    """one guarded workspace, tickets zero, every slab byte `fill`; the sequence forwards, then backwards. After EACH launch: the output is the
    baseline's, the tickets are zero, the guards intact, and every byte beyond the launch's own slabs holds what it held before"""
    g = Guarded(WC.GEMM_WORKSPACE_BYTES, gpu, fill)
    ws = g.mem
    ws[:WC.TICKET_BYTES] = 0
    prev = None
    for order in (WC.GEMM_SEQUENCE, WC.GEMM_SEQUENCE[::-1]):
        for i in order:
            e = gemm["cases"][i]
            name, t = e["c"]["name"], WC.gemm_touched_bytes(e["path"])
            before = ws.clone()
            out = _launch(gemm, i, ws)
            torch.cuda.synchronize()
            assert torch.equal(out, e["base"]), (name, "differs from its baseline on the shared, poisoned workspace")
            assert not bool(ws[:WC.TICKET_BYTES].any()), (name, "arrival tickets not left at zero")
            assert g.intact(), (name, "written outside the workspace")
            assert torch.equal(ws[t:], before[t:]), (name, f"wrote beyond its own slabs (byte {t} on)")
            if e["path"][2] > 1 and prev != i:        # (the turn of the walk repeats a case: its slabs already hold these very partial sums)
                assert not torch.equal(ws[WC.TICKET_BYTES:t], before[WC.TICKET_BYTES:t]), (name, "a split launch left its slabs as they were")
            prev = i


def test_gemm_back_to_back_without_synchronisation(gpu, gemm):
    """the sequence 16 times over on one stream and one workspace into 96 distinct outputs, one synchronisation at the end"""
    ws = _zero_ws(gpu)
    outs = [(i, gemm["cases"][i]["o"]["c0"].clone()) for _ in range(16) for i in WC.GEMM_SEQUENCE]
    torch.cuda.synchronize()
    for i, cb in outs:
        _launch(gemm, i, ws, out=cb)
    torch.cuda.synchronize()
    bad = [(n, gemm["cases"][i]["c"]["name"]) for n, (i, cb) in enumerate(outs) if not torch.equal(cb, gemm["cases"][i]["base"])]
    assert not bad, ("launches that differ from their baseline", bad)
    assert not bool(ws[:WC.TICKET_BYTES].any()), "arrival tickets not left at zero"


def test_gemm_two_streams_each_with_its_own_workspace(gpu, gemm):
    """64 launches per stream, enqueued alternately from one host thread: stream A walks the sequence forwards, stream B backwards, so launches
    of different slice counts overlap; each stream has its own zeroed workspace and outputs. One synchronisation, run once. (Measured on an
    MI355X: see docs/PARITY_TOLERANCES.md; well under ten seconds, so the count stays at 64.)"""
    n = 64
    seq = WC.GEMM_SEQUENCE
    plan = {"A": [seq[j % len(seq)] for j in range(n)], "B": [seq[::-1][j % len(seq)] for j in range(n)]}
    streams = {k: torch.cuda.Stream(device=gpu) for k in plan}
    wss = {k: _zero_ws(gpu) for k in plan}
    outs = {k: [gemm["cases"][i]["o"]["c0"].clone() for i in plan[k]] for k in plan}
    torch.cuda.synchronize()
    for j in range(n):
        for k in ("A", "B"):
            _launch(gemm, plan[k][j], wss[k], out=outs[k][j], stream=streams[k].cuda_stream)
    for s in streams.values():
        s.synchronize()
    torch.cuda.synchronize()
    bad = [(k, j, gemm["cases"][i]["c"]["name"]) for k in plan for j, i in enumerate(plan[k]) if not torch.equal(outs[k][j], gemm["cases"][i]["base"])]
    assert not bad, ("launches that differ from their baseline", bad)
    for k in plan:
        assert not bool(wss[k][:WC.TICKET_BYTES].any()), (k, "arrival tickets not left at zero")


def test_ops_gemm_keeps_one_workspace_per_stream(gpu, gemm):
    """ops.gemm under torch.cuda.stream(s1) and (s2): ops._gemm_ws holds two different tensors for the two stream handles, the results are the
    baseline's, both ticket areas are zero afterwards"""
    from unigen_amd import ops
    e = gemm["cases"][WC.SMALL_M]
    c, o = e["c"], e["o"]
    assert e["path"][2] > 1 and not c["alias"] and c["a_map"] == (0, 0) and c["c_map"] == (0, 0)
    a = o["a"].view(c["a_rows"], c["lda"])[:, :c["K"]]
    w = o["w"].view(c["N"], c["ldw"])[:, :c["K"]]
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    assert s1.cuda_stream != s2.cuda_stream
    outs = [o["c0"].clone() for _ in range(4)]
    torch.cuda.synchronize()
    for n, cb in enumerate(outs):
        with torch.cuda.stream((s1, s2)[n % 2]):
            ops.gemm(a, w, o["bias"], cb[PAD + c["c_off"]:], M=c["M"], epilogue=c["epilogue"], lda=c["lda"], ldc=c["ldc"], residual=o["r"][c["r_off"]:],
                     ldr=c["ldr"], gate=o["gate"], gate_ld=c["gate_ld"], rows_per_sample=c["rows_per_sample"], alpha=c["alpha"])
    s1.synchronize(); s2.synchronize()
    torch.cuda.synchronize()
    w1, w2 = (next(v for (dev, st), v in ops._gemm_ws.items() if st == s.cuda_stream and torch.device(dev) == a.device) for s in (s1, s2))
    assert w1.data_ptr() != w2.data_ptr() and w1.numel() == w2.numel() == WC.GEMM_WORKSPACE_BYTES
    for cb in outs:
        assert torch.equal(cb, e["base"]), "ops.gemm on a side stream differs from the baseline"
    for ws in (w1, w2):
        assert bool(ws[4096:].any()), "the launch did not use this stream's workspace"
        assert not bool(ws[:WC.TICKET_BYTES].any()), "arrival tickets not left at zero"


def test_gemm_split_k_launches_in_a_captured_graph(gpu, gemm):
    """two split-K launches of different slice counts on one stream (a single branch) in a torch.cuda.graph, replayed twice"""
    i0, i1 = WC.GEMM_SEQUENCE[0], WC.GEMM_SEQUENCE[1]
    assert gemm["cases"][i0]["path"][2] > 1 and gemm["cases"][i1]["path"][2] > 1 and gemm["cases"][i0]["path"][2] != gemm["cases"][i1]["path"][2]
    ws = _zero_ws(gpu)
    outs = [gemm["cases"][i]["o"]["c0"].clone() for i in (i0, i1)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i, cb in zip((i0, i1), outs):
            _launch(gemm, i, ws, out=cb)
    for _ in range(2):
        for i, cb in zip((i0, i1), outs):
            cb.copy_(gemm["cases"][i]["o"]["c0"])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for i, cb in zip((i0, i1), outs):
            assert torch.equal(cb, gemm["cases"][i]["base"]), (gemm["cases"][i]["c"]["name"], "a replay differs from the baseline")
        assert not bool(ws[:WC.TICKET_BYTES].any()), "arrival tickets not left at zero after a replay"


def test_gemm_too_small_workspace_selects_the_unsplit_path(gpu, gemm):
    """ug_gemm_bf16 is different by contract: a workspace 16 bytes short of what the launch's slabs need is not refused, the launch runs unsplit
    and does not touch it - the result is the no-workspace result, bit for bit (and within the sweep's bound of the split baseline's truth)"""
    i = WC.SMALL_M
    e = gemm["cases"][i]
    need = WC.gemm_touched_bytes(e["path"])
    g = Guarded(need, gpu, 0xFF)
    plain = _launch(gemm, i, None)
    short = _launch(gemm, i, g.mem[:need - 16])
    torch.cuda.synchronize()
    assert torch.equal(short, plain), "a too-small workspace does not give the no-workspace result"
    assert bool((g.mem == 0xFF).all()) and g.intact(), "an unsplit launch touched the workspace"
    ok = _launch(gemm, i, _zero_ws(gpu)[:need])          # exactly the bytes this launch needs: split again
    torch.cuda.synchronize()
    assert torch.equal(ok, e["base"])


# ----------------------------------------------------------------------------------------------------------------------------------
# the other workspace-taking entry points: name -> (inputs(shape, dt, dev), outputs(shape, dt) -> {name: bytes}, call(...) -> rc)
# ----------------------------------------------------------------------------------------------------------------------------------
_DT = {"bf16": BF, "f32": F32, "u8": U8, "mixed": None}


def _rn(g, *shape, dt=BF, s=1.0):
    return (torch.randn(*shape, generator=g, device=g.device) * s).to(dt)


def _es(dt):
    return 2 if dt == BF else 4


def _gn_in(s, dt, dev, g):
    return dict(x=_rn(g, s["B"] * s["HW"], s["C"], dt=dt), gamma=(1 + 0.2 * torch.randn(s["C"], generator=g, device=dev)).to(dt), beta=_rn(g, s["C"], dt=dt, s=0.1))


def _gn_call(lib, s, dt, i, o, ws, wsb, extra):
    fn = lib.ug_groupnorm_nhwc if dt == BF else lib.ug_groupnorm_nhwc_f32
    return fn(i["x"].data_ptr(), i["gamma"].data_ptr(), i["beta"].data_ptr(), o["out"], ws, wsb, s["B"], s["HW"], s["C"], s["G"], 1e-6, 1, _st())


def _colsum_in(s, dt, dev, g):
    return dict(a=_rn(g, s["rows"], s["cols"] + 8, dt=dt), b=_rn(g, s["rows"], s["cols"], dt=dt) if s["with_b"] else None)


def _colsum_call(lib, s, dt, i, o, ws, wsb, extra):
    fn = lib.ug_colsum if dt == BF else lib.ug_colsum_f32
    b = i["b"]
    return fn(i["a"].data_ptr(), s["cols"] + 8, None if b is None else b.data_ptr(), 0 if b is None else s["cols"], o["out"], s["cols"], s["rows"], s["cols"],
              s["rpg"], 0.5, ws, wsb, _st())


def _lw_in(s, dt, dev, g):
    return dict(p=_rn(g, s["M"], s["R"] + 8, dt=dt, s=0.5), q=_rn(g, s["M"], s["J"] + 8, dt=dt))


def _lw_call(lib, s, dt, i, o, ws, wsb, extra):
    fn = lib.ug_lora_wgrad_bf16 if dt == BF else lib.ug_lora_wgrad_f32
    return fn(i["p"].data_ptr(), s["R"] + 8, i["q"].data_ptr(), s["J"] + 8, o["out"], s["J"], s["M"], s["R"], s["J"], 0.75, ws, wsb, _st())


def _attn_in(s, dt, dev, g):
    """q, k, v, dO, and the forward's O and base-2 LSE (zero padding up to a multiple of 64 queries, as autograd.FlashAttention allocates it)"""
    from unigen_amd import ops
    B, H, Lq, Lkv, dh = s["B"], s["H"], s["Lq"], s["Lkv"], s["dh"]
    HD = H * dh
    i = dict(q=_rn(g, B, Lq, HD), k=_rn(g, B, Lkv, HD), v=_rn(g, B, Lkv, HD), do=_rn(g, B, Lq, HD), o=torch.empty(B, Lq, HD, dtype=BF, device=dev),
             lse=torch.zeros(B, H, (Lq + 63) // 64 * 64, dtype=F32, device=dev))
    ops.flash_attn(i["q"], i["k"], i["v"], i["o"], batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(HD, Lq * HD), k_strides=(HD, Lkv * HD),
                   v_strides=(HD, Lkv * HD), o_strides=(HD, Lq * HD), lse=i["lse"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(i["o"].float()).all()) and not bool(i["lse"][..., Lq:].any())
    return i


def _attn_call(lib, s, dt, i, o, ws, wsb, extra, with_lse=True):
    B, H, Lq, Lkv, dh = s["B"], s["H"], s["Lq"], s["Lkv"], s["dh"]
    HD = H * dh
    q3 = lambda p, L_: (p, HD, L_ * HD)
    return lib.ug_flash_attn_bwd(*q3(i["q"].data_ptr(), Lq), *q3(i["k"].data_ptr(), Lkv), *q3(i["v"].data_ptr(), Lkv), *q3(i["o"].data_ptr(), Lq),
                                 *q3(i["do"].data_ptr(), Lq), *q3(o["dq"], Lq), *q3(o["dk"], Lkv), *q3(o["dv"], Lkv), B, H, Lq, Lkv, dh, dh ** -0.5,
                                 i["lse"].data_ptr() if with_lse else None, ws, wsb, _st())


def _attn_call_nolse(*a):
    return _attn_call(*a, with_lse=False)


def _attn_out(s, dt):
    HD = s["H"] * s["dh"]
    return dict(dq=s["B"] * s["Lq"] * HD * 2, dk=s["B"] * s["Lkv"] * HD * 2, dv=s["B"] * s["Lkv"] * HD * 2)


def _sumsq_in(s, dt, dev, g):
    from unigen_amd import optim
    grads = [_rn(g, n, dt=_DT[d]) for n, d in s["numels"]]
    wl = optim._WorkList([(None, t, None, None, None, 0) for t in grads], dev, 0)
    torch.cuda.synchronize()
    assert wl.n_chunks == WC.grad_sumsq_chunks(s["numels"])
    return dict(grads=grads, wl=wl)


def _sumsq_call(lib, s, dt, i, o, ws, wsb, extra):
    wl = i["wl"]
    return lib.ug_grad_sumsq(wl.table.data_ptr(), wl.n_tensors, wl.chunks.data_ptr(), wl.n_chunks, 1.0, o["norm_coef"], ws, wsb, _st())


def _img_in(s, dt, dev, g):
    """low-amplitude noise (gradient magnitudes on both sides of Canny's thresholds) with one bright rectangle (strong edges)"""
    img = torch.randint(96, 144, (s["B"], s["H"], s["W"], s["C"]), generator=g, device=dev, dtype=torch.int32)
    img[:, s["H"] // 4:s["H"] // 2, s["W"] // 3:2 * s["W"] // 3] += 90
    return dict(img=img.to(U8).contiguous())


def _canny_call(lib, s, dt, i, o, ws, wsb, extra):
    B, H, W, Cc = s["B"], s["H"], s["W"], s["C"]
    sweeps = C.c_int32(-1)
    rc = lib.ug_canny_u8(i["img"].data_ptr(), H * W * Cc, W * Cc, B, H, W, Cc, 100, 200, o["out"], H * W, W, ws, wsb, C.byref(sweeps), _st())
    extra["sweeps"] = sweeps.value
    return rc


def _blur_call(lib, s, dt, i, o, ws, wsb, extra):
    from unigen_amd import image
    B, H, W, Cc = s["B"], s["H"], s["W"], s["C"]
    k = [int(v) for v in image.box_blur_constants(s["radius"])]
    return lib.ug_img_box_blur_u8(i["img"].data_ptr(), H * W * Cc, W * Cc, B, H, W, Cc, o["out"], H * W * Cc, W * Cc, *k, *k, s["passes"], s["fuse"], ws, wsb, _st())


ENTRIES = {
    "ug_groupnorm_nhwc": (_gn_in, lambda s, dt: dict(out=s["B"] * s["HW"] * s["C"] * _es(dt)), _gn_call),
    "ug_colsum": (_colsum_in, lambda s, dt: dict(out=s["rows"] // s["rpg"] * s["cols"] * _es(dt)), _colsum_call),
    "ug_lora_wgrad": (_lw_in, lambda s, dt: dict(out=s["R"] * s["J"] * _es(dt)), _lw_call),
    "ug_flash_attn_bwd": (_attn_in, _attn_out, _attn_call),
    "ug_flash_attn_bwd:lse=NULL": (_attn_in, _attn_out, _attn_call_nolse),
    "ug_grad_sumsq": (_sumsq_in, lambda s, dt: dict(norm_coef=8), _sumsq_call),
    "ug_canny_u8": (_img_in, lambda s, dt: dict(out=s["B"] * s["H"] * s["W"]), _canny_call),
    "ug_img_box_blur_u8": (_img_in, lambda s, dt: dict(out=s["B"] * s["H"] * s["W"] * s["C"]), _blur_call),
}


def _variants():
    """(id, table key, ENTRIES key, dtype)"""
    v = []
    for key, e in WC.WORKSPACES.items():
        base = key.split("/")[0]
        for d in e["dtypes"]:
            for ek in ([base, base + ":lse=NULL"] if base == "ug_flash_attn_bwd" else [base]):
                v.append((f"{key}{ek[len(base):]}-{d}", key, ek, d))
    return v


VARIANTS = _variants()


def _nbytes(lib, key, s):
    """the library's own answer (tests/test_workspace_cases_cpu.py ties the table's formulas to it)"""
    base = key.split("/")[0]
    if base == "ug_groupnorm_nhwc":
        return int(lib.ug_groupnorm_workspace_bytes(s["B"], s["HW"], s["G"]))
    if base == "ug_colsum":
        return int(lib.ug_colsum_workspace_bytes(s["rows"], s["cols"], s["rpg"]))
    if base == "ug_lora_wgrad":
        return int(lib.ug_lora_wgrad_workspace_bytes(s["M"], s["R"], s["J"]))
    if base == "ug_flash_attn_bwd":
        return int(lib.ug_flash_attn_bwd_workspace_bytes(s["B"], s["H"], s["Lq"]))
    if base == "ug_grad_sumsq":
        return int(lib.ug_grad_sumsq_workspace_bytes(WC.grad_sumsq_chunks(s["numels"])))
    if base == "ug_canny_u8":
        return int(lib.ug_canny_workspace_bytes(s["B"], s["H"], s["W"]))
    return int(lib.ug_img_blur_workspace_bytes(s["B"], s["H"], s["W"], s["C"]))


def _run(lib, ek, s, dt, inp, dev, ws, wsb=None, null_ws=False, expect=0):
    """one call into fresh guarded outputs (every byte PATTERN) -> {output: bytes as uint8, extras}; guards checked"""
    _, outs_of, call = ENTRIES[ek]
    outs = {k: Guarded(n, dev) for k, n in outs_of(s, dt).items()}
    extra = {}
    rc = call(lib, s, dt, inp, {k: g.ptr for k, g in outs.items()}, None if null_ws else ws.ptr, ws.n if wsb is None else wsb, extra)
    torch.cuda.synchronize()
    assert rc == expect, (ek, s, rc, lib.ug_last_error())
    assert ws.intact(), (ek, s, "written outside the workspace")
    if expect != 0:
        assert all(g.untouched() for g in outs.values()), (ek, s, "a refused call wrote an output")
        return None
    assert all(g.intact() for g in outs.values()), (ek, s, "written outside an output")
    res = {k: g.mem.clone() for k, g in outs.items()}
    res.update(extra)
    return res


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


@pytest.fixture(scope="module")
def lib(gpu):
    from unigen_amd import lib as L
    return L.load()


@pytest.mark.parametrize("vid,key,ek,dname", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_workspace_needs_no_initialisation_and_can_be_reused(gpu, lib, vid, key, ek, dname):
    """a workspace of exactly the reported size filled with zeros, 0xFF and 0x7F bytes: identical outputs (ug_canny_u8: and sweeps), guards intact;
    then shape a, shape b, shape a again on one workspace sized for the larger, never refilled: each equals its own zero-filled result"""
    e, dt = WC.WORKSPACES[key], _DT[dname]
    g = torch.Generator(device=gpu).manual_seed(len(vid) * 131 + sum(map(ord, vid)))
    zero = {}
    inps = {}
    for tag in ("a", "b"):
        s = e[tag]
        inps[tag] = ENTRIES[ek][0](s, dt, gpu, g)
        n = _nbytes(lib, key, s)
        runs = [_run(lib, ek, s, dt, inps[tag], gpu, Guarded(n, gpu, f)) for f in FILLS]
        for f, r in zip(FILLS[1:], runs[1:]):
            assert _same(runs[0], r), (vid, tag, f"workspace filled with {f:#x} bytes: not the zero-filled result")
        for k, t in runs[0].items():                     # not garbage: no output is left at its fill, floating-point outputs are finite
            if torch.is_tensor(t):
                assert not bool((t == PATTERN).all()), (vid, tag, k, "the output was not written")
                if dt in (BF, F32) or key == "ug_grad_sumsq":
                    assert bool(torch.isfinite(t.view(F32 if (dt == F32 or key == "ug_grad_sumsq") else BF).float()).all()), (vid, tag, k)
        if key == "ug_canny_u8":
            assert runs[0]["sweeps"] >= 1 and 0 < int((runs[0]["out"] == 255).sum()) < runs[0]["out"].numel()
        zero[tag] = runs[0]
    shared = Guarded(max(_nbytes(lib, key, e["a"]), _nbytes(lib, key, e["b"])), gpu, 0x7F)
    for tag in ("a", "b", "a"):
        assert _same(_run(lib, ek, e[tag], dt, inps[tag], gpu, shared), zero[tag]), (vid, tag, "on a workspace another shape has used")


@pytest.mark.parametrize("vid,key,ek,dname", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_undersized_or_missing_workspace_is_refused_before_any_launch(gpu, lib, vid, key, ek, dname):
    """the reported size minus the alignment unit, and a NULL workspace: UG_ERR_BAD_SHAPE, every output byte still its fill. (The memory behind
    the pointer has the full size: the call is refused on the number alone.)"""
    from unigen_amd import lib as L
    e, dt = WC.WORKSPACES[key], _DT[dname]
    g = torch.Generator(device=gpu).manual_seed(17)
    for tag in ("a", "b"):
        s = e[tag]
        inp = ENTRIES[ek][0](s, dt, gpu, g)
        n = _nbytes(lib, key, s)
        ws = Guarded(n, gpu, 0x7F)
        _run(lib, ek, s, dt, inp, gpu, ws, wsb=n - e["unit"], expect=L.UG_ERR_BAD_SHAPE)
        _run(lib, ek, s, dt, inp, gpu, ws, null_ws=True, expect=L.UG_ERR_BAD_SHAPE)
        assert bool((ws.mem == 0x7F).all()), (vid, tag, "a refused call wrote its workspace")


# ----------------------------------------------------------------------------------------------------------------------------------
# partial-sum outputs the caller reduces (ops.py allocates them with torch.empty and sums every row)
# ----------------------------------------------------------------------------------------------------------------------------------
def _partials_twice(call, part_bytes, out_bytes, dev, what):
    """call(partials pointer, dx pointer) with the partial buffer pre-filled with 0xFF bytes (NaN), then with zeros -> the two partial buffers
    (fp32); dx identical, no element NaN, guards intact"""
    got = []
    for fill in (0xFF, 0x00):
        part, dx = Guarded(part_bytes, dev, fill), Guarded(out_bytes, dev)
        rc = call(part.ptr, dx.ptr)
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        assert part.intact() and dx.intact(), (what, "written outside a buffer")
        p = part.mem.clone().view(F32)
        assert not bool(torch.isnan(p).any()), (what, f"{int(torch.isnan(p).sum())} elements of the partial buffer were not written")
        got.append((p, dx.mem.clone()))
    assert torch.equal(got[0][1], got[1][1]), (what, "dx depends on what the partial buffer held")
    return got[0][0], got[1][0]


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,rps,D", WC.ADALN_BWD_PARTIALS)
def test_adaln_modulate_bwd_writes_every_partial_row(gpu, lib, rows, rps, D, dt):
    g = torch.Generator(device=gpu).manual_seed(rows + D)
    samples, P = rows // rps, int(lib.ug_adaln_modulate_bwd_partials(rows, rps))
    x, dy, sc = _rn(g, rows, D + 8, dt=dt), _rn(g, rows, D, dt=dt), _rn(g, samples, D, dt=dt, s=0.3)
    fn = lib.ug_adaln_modulate_bwd if dt == BF else lib.ug_adaln_modulate_bwd_f32
    call = lambda part, dx: fn(x.data_ptr(), D + 8, dy.data_ptr(), D, sc.data_ptr(), D, rps, dx, D, part, rows, D, 1e-6, _st())
    a, b = _partials_twice(call, samples * P * 2 * D * 4, rows * D * _es(dt), gpu, ("adaln", rows, rps, D, str(dt)))
    red = lambda p: p.view(samples, P, 2, D).sum(1)          # ops.adaln_modulate_bwd's reduction
    assert torch.equal(red(a), red(b)) and bool(red(a).abs().sum() > 0)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,heads,dh", WC.QK_BWD_PARTIALS)
def test_qk_rmsnorm_rope_bwd_writes_every_partial_row(gpu, lib, rows, heads, dh, dt):
    g = torch.Generator(device=gpu).manual_seed(rows + heads)
    HD, P = heads * dh, int(lib.ug_qk_rmsnorm_rope_bwd_partials(rows, heads))
    x, dy, w = _rn(g, rows, HD, dt=dt), _rn(g, rows, HD, dt=dt), (1 + 0.2 * torch.randn(dh, generator=g, device=gpu)).to(dt)
    ang = torch.rand(rows, dh // 2, generator=g, device=gpu) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    fn = lib.ug_qk_rmsnorm_rope_bwd if dt == BF else lib.ug_qk_rmsnorm_rope_bwd_f32
    call = lambda part, dx: fn(x.data_ptr(), HD, dy.data_ptr(), HD, dx, HD, part, w.data_ptr(), cos.data_ptr(), sin.data_ptr(), rows, rows, 0, heads, dh,
                               1e-6, _st())
    a, b = _partials_twice(call, P * dh * 4, rows * HD * _es(dt), gpu, ("qk", rows, heads, dh, str(dt)))
    red = lambda p: p.view(P, dh).sum(0)                      # ops.qk_rmsnorm_rope_bwd's reduction
    assert torch.equal(red(a), red(b)) and bool(red(a).abs().sum() > 0)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("S,D,E", WC.MOE_GATE_BWD_PARTIALS)
def test_moe_gate_bwd_writes_every_partial_row(gpu, lib, S, D, E, dt):
    g = torch.Generator(device=gpu).manual_seed(S + D + E)
    P = int(lib.ug_moe_gate_bwd_slices(S))
    x, c, wg = _rn(g, S, D + 8, dt=dt), _rn(g, S, D + 8, dt=dt), _rn(g, E, D, dt=dt, s=D ** -0.5)
    gates = torch.softmax(_rn(g, S, E, dt=F32, s=2.0), -1).contiguous()
    dgates = _rn(g, S, E, dt=F32)
    fn = lib.ug_moe_gate_bwd if dt == BF else lib.ug_moe_gate_bwd_f32
    call = lambda part, dx: fn(gates.data_ptr(), dgates.data_ptr(), x.data_ptr(), c.data_ptr(), D + 8, wg.data_ptr(), S, D, E, dx, D, part, _st())
    a, b = _partials_twice(call, P * E * D * 4, S * D * _es(dt), gpu, ("gate", S, D, E, str(dt)))
    red = lambda p: p.view(P, E, D).sum(0)                    # ops.moe_gate_bwd's reduction
    assert torch.equal(red(a), red(b)) and bool(red(a).abs().sum() > 0)


# ----------------------------------------------------------------------------------------------------------------------------------
# the LSE padding on the product path
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,Lq,Lkv", [(64, 333, 520), (128, 333, 520), (128, 2049, 520)])
def test_flash_attn_bwd_does_not_read_the_lse_padding_into_a_result(gpu, dh, Lq, Lkv):
    """ops.flash_attn(lse=) then ops.flash_attn_bwd(lse=) on an LSE buffer allocated as NaN, [..., Lq:] included: the forward writes rows < Lq only,
    and every backward kernel selects 0 for a query row >= Lq (attn_bwd_dkv_kernel's `valid`; the dQ kernels clamp their own row) instead of
    multiplying by it, so dq / dk / dv are bit-identical to the run on a torch.zeros buffer. The padding must exist (whole 64-row tiles of
    statistics are loaded); its values reach no product."""
    from unigen_amd import ops
    B, H = 2, 2
    HD = H * dh
    g = torch.Generator(device=gpu).manual_seed(dh + Lq)
    q, k, v, do = _rn(g, B, Lq, HD), _rn(g, B, Lkv, HD), _rn(g, B, Lkv, HD), _rn(g, B, Lq, HD)
    res = {}
    for name, fill in (("zeros", 0.0), ("nan", float("nan"))):
        lse = torch.full((B, H, (Lq + 63) // 64 * 64), fill, dtype=F32, device=gpu)
        o = torch.empty(B, Lq, HD, dtype=BF, device=gpu)
        ops.flash_attn(q, k, v, o, batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(HD, Lq * HD), k_strides=(HD, Lkv * HD), v_strides=(HD, Lkv * HD),
                       o_strides=(HD, Lq * HD), lse=lse)
        grads = ops.flash_attn_bwd(q, k, v, o, do, heads=H, lse=lse)
        torch.cuda.synchronize()
        if name == "nan":
            assert bool(torch.isnan(lse[..., Lq:]).all()) and bool(torch.isfinite(lse[..., :Lq]).all())
        res[name] = (o, *grads)
    for n, a, b in zip(("o", "dq", "dk", "dv"), res["zeros"], res["nan"]):
        assert bool(torch.isfinite(b.float()).all()), (n, "the NaN padding of the statistics reached a result")
        assert torch.equal(a, b), (n, "depends on the LSE padding")
