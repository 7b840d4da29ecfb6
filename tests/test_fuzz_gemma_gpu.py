"""The head-width-256 soft-cap attention (ug_flash_attn_fwd_softcap: attn_plain_kernel<256, 32, false, true, CAP, true>) and its fp32 twin
(ug_flash_attn_fwd_softcap_f32: flash_attn_f32_kernel<256, 4, false, true>) through the C ABI over the case grid of tests/gemma_attn_cases.py, against
gemma_ref.attention in float64 (tests/test_gemma_attn_cases_cpu.py checks on the host what the grid promises and that it catches every mutant).

Bounds (docs/PARITY_TOLERANCES.md, "Gemma-2 text encoder"; the rules of test_gemma_gpu.test_flash_attn_softcap, computed here from the references):
  bf16       rel-L2 and the worst query row <= max(1.5 x the same metric of the rounding-point variant, 2^-9)
  fp32 twin  rel-L2 <= 1e-5, every row <= 1e-4; with a cap <= max(that, 4 x the error of the float32 host evaluation)
Rows that legitimately see a V of 1e4 ("dirty") are judged apart from the clean ones; rows without a live key are exactly zero in both dtypes and all
others finite.

Layouts. Every case runs the bf16 entry in two of three layouts and the twin in the third, rotating over the list: `packed` [q | k | v] as the model
has it; `separate`, q, k and v in buffers of their own with 8 pad columns per row and 3 spare rows behind every sample; `kv_first`, packed with the K/V
heads ahead of the q heads. Every element that is not an operand is NaN; the rows in [kv_len, L) are operands (the kernel multiplies them by zero).
The output has 8 pad columns, a spare row per sample and a base offset of 4 elements, pre-filled with a sentinel that must survive outside [L, H 256].
A second launch gives the same bits; once per instantiation another launch in between does not change them either. window = L, L + 5 and 4096 give
the bits of window = 0. The refusals of attn_softcap_check (kv_heads not dividing heads, a negative window, dh != 256) are pinned for both entries by
tests/test_gemma_code_object_cpu.py::test_attn_softcap_abi_rejections and not repeated here. Nothing outside the repository is read."""
import pytest
import torch

from tests import gemma_attn_cases as G

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DH = G.DH
SENT = -768.0                                         # exact in bf16; no output of these cases equals it
LAYOUTS = ("packed", "separate", "kv_first")
PAD, SPARE, SPARE_O, O_OFFSET = 8, 3, 1, 4
ENTRY = {BF: "ug_flash_attn_fwd_softcap", F32: "ug_flash_attn_fwd_softcap_f32"}


def alloc(c, layout, dt, dev):
    """-> dict: q, k, v: [B, L, heads 256] views of NaN-filled device buffers in the layout (operands are copied into them); flat / o: the output's
    sentinel-filled storage and its [B, L + 1, H 256 + 8] view 4 elements in"""
    B, L, H, KV = c["B"], c["L"], c["H"], c["KV"]
    nan = float("nan")
    if layout == "separate":
        bufs = [torch.full((B, L + SPARE, n * DH + PAD), nan, dtype=dt, device=dev) for n in (H, KV, KV)]
        q, k, v = (X[:, :L, :n * DH] for X, n in zip(bufs, (H, KV, KV)))
    else:
        X = torch.full((B, L, (H + 2 * KV) * DH), nan, dtype=dt, device=dev)
        cols = (2 * KV * DH, 0, KV * DH) if layout == "kv_first" else (0, H * DH, (H + KV) * DH)
        q, k, v = (X[:, :, c0:c0 + n * DH] for c0, n in zip(cols, (H, KV, KV)))
    flat = torch.full((O_OFFSET + B * (L + SPARE_O) * (H * DH + PAD),), SENT, dtype=dt, device=dev)
    return dict(q=q, k=k, v=v, flat=flat, o=flat[O_OFFSET:].view(B, L + SPARE_O, H * DH + PAD))


def fill(buf, d):
    for n in "qkv":
        t = d[n]
        buf[n].copy_(t.reshape(t.shape[0], t.shape[1], -1).to(buf[n].dtype))


def launch(cdll, buf, c, window=None, kv_len="case"):
    from unigen_amd import lib as ULIB
    dt, o = buf["o"].dtype, buf["o"]
    kv_len = c["kv_len"] if kv_len == "case" else kv_len
    kvl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=o.device)
    args = []
    for n in "qkv":
        args += [buf[n].data_ptr(), buf[n].stride(1), buf[n].stride(0)]
    rc = getattr(cdll, ENTRY[dt])(*args, o.data_ptr(), o.stride(1), o.stride(0), c["B"], c["H"], c["KV"], c["L"], DH, G.SCALE, c["cap"],
                                  c["window"] if window is None else window, None if kvl is None else kvl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ULIB.check(rc, ENTRY[dt])
    torch.cuda.synchronize()


def read(buf, c):
    """-> (the [B, L, H, 256] window on the host, whether the sentinel is intact everywhere else)"""
    B, L, H = c["B"], c["L"], c["H"]
    flat = buf["flat"].cpu()
    win = flat[O_OFFSET:].view(B, L + SPARE_O, H * DH + PAD)[:, :L, :H * DH]
    got = win.clone().view(B, L, H, DH)
    win.fill_(SENT)
    return got, bool((flat == SENT).all())


def run_checked(cdll, gpu, c, d, rf, layout, dt):
    tag = (c["id"], layout, dt)
    buf = alloc(c, layout, dt, gpu)
    fill(buf, d)
    launch(cdll, buf, c)
    got, intact = read(buf, c)
    assert intact, ("the output sentinel outside the [L, H 256] window was overwritten", tag)
    assert bool((got[rf["dead"]] == 0).all()), ("a row without a live key is not exactly zero", tag)
    assert bool(torch.isfinite(got[~rf["dead"]]).all()), ("a NaN of the padding, or an infinity, reached the output", tag)
    ratio, lines = G.judge(c, rf, got, dt == BF)
    for line in lines:
        print(f"GEMMA sweep [{layout}] {line}")
    print(f"GEMMA sweep ratio {c['kind']} {'bf16' if dt == BF else 'f32'} {c['id']} [{layout}]: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (tag, lines)
    first = buf["flat"].clone()
    launch(cdll, buf, c)
    assert torch.equal(buf["flat"], first), ("a second launch on the same buffers differs", tag)
    return got


@pytest.mark.parametrize("case_id", G.case_ids())
def test_softcap_attention_against_fp64(gpu, case_id):
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    c, d, rf = G.case(case_id), G.case_data(case_id), G.refs(case_id)
    i = G.case_ids().index(case_id)
    for j in (0, 1):
        run_checked(cdll, gpu, c, d, rf, LAYOUTS[(i + j) % 3], BF)
    run_checked(cdll, gpu, c, d, rf, LAYOUTS[(i + 2) % 3], F32)


WIDE = [c["id"] for c in G.cases() if c["kind"] == "geometry" and c["window_spec"] in ("L", "L+5", 4096)]


@pytest.mark.parametrize("case_id", WIDE)
def test_a_window_of_the_length_or_more_is_no_window(gpu, case_id):
    """window = L, L + 5 and 4096 (the table's own rows with them) give the bits of window = 0"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    c, d = G.case(case_id), G.case_data(case_id)
    assert c["window"] >= c["L"]
    for dt in (BF, F32):
        buf = alloc(c, "packed", dt, gpu)
        fill(buf, d)
        launch(cdll, buf, c, window=0)
        want = buf["flat"].clone()
        buf["flat"].fill_(SENT)
        for w in (c["window"], c["L"], c["L"] + 5, 4096):
            launch(cdll, buf, c, window=w)
            assert torch.equal(buf["flat"], want), (case_id, dt, w)


assert len(WIDE) >= 6 and {G.case(i)["window_spec"] for i in WIDE} == {"L", "L+5", 4096}

# (instantiation, dtype, the case, a second case of the same shape): bf16 with the cap, bf16 without, the twin
STATE = (("cap", BF, "rising-L300-cap50-w0-h3kv1", "spike_diag-L300-cap50-w0-h3kv1"), ("nocap", BF, "rising-L300-cap0-w0-h2kv1", "spike_diag-L300-cap0-w0-h2kv1"),
         ("twin", F32, "spike_diag-L300-cap50-w0-h3kv1", "rising-L300-cap50-w0-h3kv1"))


@pytest.mark.parametrize("inst", STATE, ids=lambda t: t[0])
def test_no_state_between_launches(gpu, inst):
    """the first case, then a second case's operands in the same buffers (with a window and key lengths of its own, so that it takes other paths), then
    the first again: the first result's bits"""
    from unigen_amd import lib as ULIB
    cdll = ULIB.load()
    _, dt, first_id, second_id = inst
    c, c2 = G.case(first_id), G.case(second_id)
    assert all(c[n] == c2[n] for n in ("B", "L", "H", "KV")) and bool(c["cap"]) == bool(c2["cap"])
    d, d2 = dict(G.case_data(first_id)), dict(G.case_data(second_id))
    buf = alloc(c, "separate", dt, gpu)
    fill(buf, d)
    launch(cdll, buf, c)
    want = buf["flat"].clone()
    fill(buf, d2)
    launch(cdll, buf, c2, window=33, kv_len=[c["L"] // 2, 1])
    assert not torch.equal(buf["flat"], want)
    fill(buf, d)
    launch(cdll, buf, c)
    assert torch.equal(buf["flat"], want), inst[0]
