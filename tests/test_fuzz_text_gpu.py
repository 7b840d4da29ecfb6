"""Sweep of the text-encoder kernels (csrc/text.hip: attention with T5's bias table and / or the causal mask, the bias table, the row norms, the
two activations, and the fp32 twin of each) against the float64 references, case builders and judges of tests/text_ref.py, which
tests/test_text_ref_cpu.py pins to transformers and shows to be sharp: every named index slip of the attention reference misses the bound used here.

What is asserted (docs/PARITY_TOLERANCES.md, "Text sweep"; no number is new - the rules are those of tests/test_text_gpu.py):
  - attention: bf16 rel-L2 and the worst query row <= max(1.5 x the rounding-point variant's own, 2^-9), the fp32 twin rel-L2 <= 1e-5 and every row
    <= 1e-4, for the full 128-query workgroups and for the last partial one separately; every output value finite although every spare row and pad
    column of q, k and v holds NaN; every sentinel round the output untouched;
  - rel table: bit-exact;
  - norms and activations: per element within one bf16 ulp of the float64 value plus 2^-20 of the magnitudes that enter in fp32 (the twins: that term
    alone), outputs strided with sentinels in the pad columns, a spare row and both guards;
  - refused argument sets raise and write nothing; empty problems return and write nothing;
  - T5EncoderModel's per-length table cache follows the lengths and the weights, bit for bit.
Each test prints its worst error / bound as `TEXTSWEEP <family> ...`; the run recorded in the document lists the worst per family."""
import functools
import os

import pytest
import torch

from tests import text_ref as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTS = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
G = R.GUARD
SENT = R.SENT_O
WORST = {}


def _line(family, ident, dt, ratio):
    key = f"{family}/{'bf16' if dt == BF else 'f32'}"
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"TEXTSWEEP {key} {ident}: worst error / bound = {ratio:.3f} (family so far {WORST[key]:.3f})")


# ---- attention -------------------------------------------------------------------------------------------------------------------
def _launch_attn(gpu, c, dt):
    """case c in its own layout -> (result [B, Lq, H, 64] on the host, sentinels intact, read-only operands unchanged)"""
    from unigen_amd import ops
    bufs = R.attn_buffers(c, dt)
    dev = {}
    for n in "qkvo":
        key = id(bufs[n]["buf"])                                  # a packed q | k | v buffer goes to the device once
        if key not in dev:
            dev[key] = bufs[n]["buf"].to(gpu)
    t = {n: dev[id(bufs[n]["buf"])][bufs[n]["off"]:] for n in "qkvo"}
    before = {k: v.clone() for k, v in dev.items() if k != id(bufs["o"]["buf"])}
    if dt == BF:
        assert t["o"].data_ptr() % 16 == (8 if c["layout"]["o"]["off"] else 0)
    st = lambda n: (bufs[n]["rs"], bufs[n]["bs"])
    ops.flash_attn_bias(t["q"], t["k"], t["v"], t["o"], batches=c["B"], heads=c["H"], dh=64, Lq=c["Lq"], Lkv=c["Lkv"], q_strides=st("q"), k_strides=st("k"),
                        v_strides=st("v"), o_strides=st("o"), scale=c["scale"], rel_table=c["table"].to(gpu) if c["table"] is not None else None, causal=c["causal"])
    torch.cuda.synchronize()
    got, intact = R.attn_read_output(c, bufs["o"], dev[id(bufs["o"]["buf"])])
    same = all(torch.equal(v.view(torch.int16 if dt == BF else torch.int32), dev[k].view(torch.int16 if dt == BF else torch.int32)) for k, v in before.items())
    return got, intact, same


def _check_attn(gpu, c, dt, family):
    truth, variant = R.attn_refs(c)
    got, intact, same = _launch_attn(gpu, c, dt)
    assert intact, "the kernel wrote outside its output"
    assert same, "a read-only operand changed"
    assert torch.isfinite(got).all(), "a non-finite output: a row or column outside the operands was read"
    ratio, lines = R.attn_judge(got, truth, variant, dt == BF)
    for ln in lines:
        print(f"TEXTSWEEP attn {c['id']} {'bf16' if dt == BF else 'f32'} {ln}")
    _line(family, c["id"], dt, ratio)
    assert ratio <= 1.0, (c["id"], dt, lines)


SWEEP = [R.attn_sweep_spec(i) for i in range(R.N_ATTN_SWEEP)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("i", [pytest.param(s["i"], id=s["id"]) for s in SWEEP])
def test_attn_bias_sweep(gpu, i, dt):
    _check_attn(gpu, R.attn_sweep_case(i), dt, "attn-sweep")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(R.ATTN_FIXED))
def test_attn_bias_fixed(gpu, name, dt):
    """rel4096 is the launch with the largest LDS request (18 KiB of tiles + 32 KiB of table); its table's far entries hold large distinct values"""
    _check_attn(gpu, R.attn_fixed_case(name), dt, "attn-fixed")


def _plain_attn_args(gpu, dt, B=1, H=2, Lq=64, Lkv=64, dh=64, spare=64):
    """contiguous q, k, v with room to spare and a sentinel-filled output"""
    W = H * dh
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B * L + spare, W, generator=g).to(device=gpu, dtype=dt) for L in (Lq, Lkv, Lkv))
    out = torch.full((G + B * Lq * W + G,), SENT, device=gpu, dtype=dt)
    kw = dict(batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(W, Lq * W), k_strides=(W, Lkv * W), v_strides=(W, Lkv * W), o_strides=(W, Lq * W), scale=1.0)
    return q.view(-1), k.view(-1), v.view(-1), out, kw


@pytest.mark.parametrize("dt", DTS)
def test_attn_bias_refusals(gpu, dt):
    from unigen_amd import lib, ops
    tab = lambda H, rel_len: torch.zeros(H, 2 * rel_len - 1, device=gpu, dtype=F32)

    def refused(what, table=None, causal=False, q_off=0, o_off=G, exc=lib.UniGenHipError, shape=None, **over):
        q, k, v, out, kw = _plain_attn_args(gpu, dt, **(shape or {}))
        kw.update(over)
        with pytest.raises(exc):
            ops.flash_attn_bias(q[q_off:], k, v, out[o_off:], rel_table=table, causal=causal, **kw)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), f"{what}: refused, but the output was written"

    refused("dh = 128 with a table", table=tab(2, 64), shape=dict(dh=128))
    refused("dh = 128 with the mask", causal=True, shape=dict(dh=128))
    refused("rel_len below Lq", table=tab(2, 63), shape=dict(Lq=64, Lkv=32))
    refused("rel_len below Lkv", table=tab(2, 63), shape=dict(Lq=32, Lkv=64))
    refused("rel_len = 4097", table=tab(2, 4097))
    refused("q row stride not a multiple of 8 elements (4 for the twin)", causal=True, q_strides=(128 + (4 if dt == BF else 2), 64 * 128 + 8))
    refused("q base 2 bytes off (4 for the twin)", causal=True, q_off=1)
    refused("o row stride not a multiple of 4", causal=True, o_strides=(130, 64 * 130))
    refused("o base 4 bytes off (8 for the twin)", causal=True, o_off=G + 2)
    refused("table with an even width", table=torch.zeros(2, 128, device=gpu, dtype=F32), exc=ValueError)
    refused("table of another head count", table=tab(3, 64), exc=ValueError)
    refused("one-dimensional table", table=torch.zeros(127, device=gpu, dtype=F32), exc=ValueError)
    refused("no keys", causal=True, Lkv=0)
    refused("no heads", causal=True, heads=0)
    refused("sequence too long", causal=True, Lq=1 << 30)
    refused("grid too large", causal=True, batches=1 << 31, Lq=1)
    # a table that is not 4-byte aligned cannot be built from a torch tensor: the C entry point directly
    q, k, v, out, kw = _plain_attn_args(gpu, dt)
    t = tab(2, 65)
    fn = lib.load().ug_flash_attn_fwd_bias if dt == BF else lib.load().ug_flash_attn_fwd_bias_f32
    rc = fn(q.data_ptr(), 128, 64 * 128, k.data_ptr(), 128, 64 * 128, v.data_ptr(), 128, 64 * 128, out[G:].data_ptr(), 128, 64 * 128, 1, 2, 64, 64, 64, 1.0,
            t.data_ptr() + 2, 64, 0, None)
    assert rc == lib.UG_ERR_BAD_ALIGN and b"rel_table" in lib.load().ug_last_error()
    # empty problems return without writing
    for over in (dict(batches=0), dict(Lq=0)):
        for table, causal in ((tab(2, 64), False), (None, True)):
            ops.flash_attn_bias(q, k, v, out[G:], rel_table=table, causal=causal, **dict(kw, **over))
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- row norms -------------------------------------------------------------------------------------------------------------------
class Strided:
    """an output [rows, D] with leading dimension ld inside a sentinel-filled device buffer: guards, pad columns and one spare row"""

    def __init__(self, rows, D, ld, dt, dev):
        self.buf = torch.full((G + (rows + 1) * ld + G,), SENT, dtype=dt, device=dev)
        self.body = self.buf[G:G + (rows + 1) * ld].view(rows + 1, ld)
        self.t = self.body[:rows, :D]
        self.rows, self.D = rows, D

    def cpu(self):
        torch.cuda.synchronize()
        return self.t.cpu().double()

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.clone()
        b[G:-G].view(self.rows + 1, -1)[:self.rows, :self.D] = SENT
        return bool((b == SENT).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENT).all())


def _operand(values, ld, dt, dev):
    """a read-only [rows, D] operand with leading dimension ld; its pad columns hold NaN, which no sum survives"""
    rows, D = values.shape
    full = torch.full((rows, ld), float("nan"), dtype=dt)
    full[:, :D] = values.to(dt)
    return full.to(dev)[:, :D]


NORMS = [pytest.param(c, id=c["id"]) for c in R.norm_sweep_cases()]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", NORMS)
def test_norm_rows_sweep(gpu, c, dt):
    """D = 4608 is the last register-resident width, 4616 the first that reads its row again from memory"""
    from unigen_amd import ops
    x, w, b = R.norm_data(c)
    xd, wd, bd = _operand(x, c["ldx"], dt, gpu), w.to(device=gpu, dtype=dt), b.to(device=gpu, dtype=dt)
    for name, eps in (("rmsnorm", 1e-6), ("layernorm", 1e-5)):
        out = Strided(c["rows"], c["D"], c["ldo"], dt, gpu)
        if name == "rmsnorm":
            truth, bound = R.rmsnorm_bound(x, w, eps, dt == BF)
            ops.rmsnorm_rows(xd, wd, eps, out=out.t)
        else:
            truth, bound = R.layernorm_bound(x, w, b, eps, dt == BF)
            ops.layernorm_rows(xd, wd, bd, eps, out=out.t)
        assert out.intact(), f"{name} wrote outside its output"
        got = out.cpu()
        per_row = ((got - truth).abs() / bound).amax(-1)
        ratio = R.elementwise_excess(got, truth, bound, dt == BF)
        _line(name + ("-reg" if c["D"] <= 4608 else "-mem"), c["id"], dt, ratio)
        assert ratio <= 1.0, (name, c["id"], dt, dict(zip(R.norm_row_kinds(c), per_row.tolist())))
        if name == "layernorm" and dt == F32:
            for r, kind in enumerate(R.norm_row_kinds(c)):
                if kind in ("constant", "zero"):                  # variance exactly 0 in fp32 as well: the answer is b, to the bit
                    assert torch.equal(got[r], b), (c["id"], kind)


# ---- activations -----------------------------------------------------------------------------------------------------------------
ACTS = [pytest.param(c, id=c["id"]) for c in R.act_sweep_cases()]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", ACTS)
def test_gated_gelu_sweep(gpu, c, dt):
    from unigen_amd import ops
    ab = R.act_data(c)
    out = Strided(c["M"], c["F"], c["ldo"], dt, gpu)
    ops.gated_gelu(_operand(ab, c["ld"], dt, gpu), out=out.t)
    assert out.intact(), "gated_gelu wrote outside its output"
    truth, bound = R.gated_gelu_bound(ab, dt == BF)
    ratio = R.elementwise_excess(out.cpu(), truth, bound, dt == BF)
    _line("gated_gelu", c["id"], dt, ratio)
    assert ratio <= 1.0, (c["id"], dt)


@pytest.mark.parametrize("dt", DTS)
def test_activations_all_bf16_values(gpu, dt):
    """every finite bf16 value through both activations (the gate paired with 1, -3 and a full-mantissa value), in bf16 and, on the same values, in fp32"""
    from unigen_amd import ops
    x = R.all_finite_bf16()
    n = x.numel()
    ab = torch.cat([x[None].expand(3, n), torch.tensor(R.GATE_B, dtype=F64)[:, None].expand(3, n)], -1)
    out = Strided(3, n, n, dt, gpu)
    ops.gated_gelu(ab.to(device=gpu, dtype=dt), out=out.t)
    assert out.intact()
    truth, bound = R.gated_gelu_bound(ab, dt == BF)
    ratio = R.elementwise_excess(out.cpu(), truth, bound, dt == BF)
    _line("gated_gelu-all", "65280x3", dt, ratio)
    assert ratio <= 1.0
    xd = x.to(device=gpu, dtype=dt)
    y = Strided(1, n, n, dt, gpu)
    ops.quick_gelu(xd, out=y.t.view(-1))
    assert y.intact()
    truth, bound = R.quick_gelu_bound(x, dt == BF)
    ratio = R.elementwise_excess(y.cpu()[0], truth, bound, dt == BF)
    _line("quick_gelu-all", "65280", dt, ratio)
    assert ratio <= 1.0
    z = Strided(1, n, n, dt, gpu)
    z.t.copy_(xd[None])
    ops.quick_gelu(z.t.view(-1), out=z.t.view(-1))                # in place, as text.py calls it
    assert z.intact()
    bits = torch.int16 if dt == BF else torch.int32
    assert torch.equal(z.t.contiguous().view(bits), y.t.contiguous().view(bits)), "in place and out of place differ"


@pytest.mark.parametrize("dt", DTS)
def test_norm_and_activation_refusals(gpu, dt):
    from unigen_amd import lib
    cdll = lib.load()
    tw = "" if dt == BF else "_f32"
    per16 = 8 if dt == BF else 4
    x = torch.ones(4096, device=gpu, dtype=dt)
    w = torch.ones(4096, device=gpu, dtype=dt)
    out = torch.full((4096,), SENT, device=gpu, dtype=dt)
    xp, wp, op, es = x.data_ptr(), w.data_ptr(), out.data_ptr(), x.element_size()
    rms = lambda *a: getattr(cdll, "ug_rmsnorm_rows" + tw)(*a, 1e-6, None)            # (x, ldx, w, out, ldo, rows, D)
    ln = lambda *a: getattr(cdll, "ug_layernorm_rows" + tw)(*a, 1e-5, None)           # (x, ldx, w, b, out, ldo, rows, D)
    gg = lambda *a: getattr(cdll, "ug_gated_gelu" + tw)(*a, None)                     # (ab, ld, out, ldo, M, F)
    qg = lambda *a: getattr(cdll, "ug_quick_gelu" + tw)(*a, None)                     # (x, y, n)
    refusals = {
        "norm D % 8": (rms(xp, 64, wp, op, 64, 4, 12), ln(xp, 64, wp, wp, op, 64, 4, 12)),
        "norm ldx < D": (rms(xp, 56, wp, op, 64, 4, 64), ln(xp, 56, wp, wp, op, 64, 4, 64)),
        "norm ldo < D": (rms(xp, 64, wp, op, 56, 4, 64), ln(xp, 64, wp, wp, op, 56, 4, 64)),
        "norm ldx not 16-byte aligned": (rms(xp, 64 + per16 // 2, wp, op, 64, 4, 64), ln(xp, 64 + per16 // 2, wp, wp, op, 64, 4, 64)),
        "norm ldo not 16-byte aligned": (rms(xp, 64, wp, op, 64 + per16 // 2, 4, 64), ln(xp, 64, wp, wp, op, 64 + per16 // 2, 4, 64)),
        "norm x base not 16-byte aligned": (rms(xp + es, 64, wp, op, 64, 4, 64), ln(xp + es, 64, wp, wp, op, 64, 4, 64)),
        "norm D = 0": (rms(xp, 64, wp, op, 64, 4, 0), ln(xp, 64, wp, wp, op, 64, 4, 0)),
        "norm without a weight": (rms(xp, 64, None, op, 64, 4, 64), ln(xp, 64, wp, None, op, 64, 4, 64)),
        "norm too many rows": (rms(xp, 64, wp, op, 64, 1 << 33, 64), ln(xp, 64, wp, wp, op, 64, 1 << 33, 64)),
        "gate F % 8": (gg(xp, 64, op, 64, 4, 12),),
        "gate ld < 2F": (gg(xp, 56, op, 32, 4, 32),),
        "gate ldo < F": (gg(xp, 64, op, 24, 4, 32),),
        "gate ld not 16-byte aligned": (gg(xp, 64 + per16 // 2, op, 32, 4, 32),),
        "gate out base not 16-byte aligned": (gg(xp, 64, op + es, 32, 4, 32),),
        "gate F = 0": (gg(xp, 64, op, 32, 4, 0),),
        "gate too many elements": (gg(xp, 16, op, 8, 1 << 39, 8),),
        "quick n % 8": (qg(xp, op, 12),),
        "quick base not 16-byte aligned": (qg(xp + es, op, 64),),
        "quick without an output": (qg(xp, None, 64),),
        "quick too many elements": (qg(xp, op, 1 << 42),),
    }
    for what, codes in refusals.items():
        for rc in codes:
            assert rc in (lib.UG_ERR_BAD_SHAPE, lib.UG_ERR_BAD_ALIGN, lib.UG_ERR_UNSUPPORTED), (what, rc)
            with pytest.raises(lib.UniGenHipError):
                lib.check(rc, what)
    # empty problems return without writing
    assert rms(xp, 64, wp, op, 64, 0, 64) == lib.UG_OK and ln(xp, 64, wp, wp, op, 64, 0, 64) == lib.UG_OK
    assert gg(xp, 64, op, 32, 0, 32) == lib.UG_OK and qg(xp, op, 0) == lib.UG_OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused or empty call wrote its output"


# ---- the bias table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", (3, 64))
@pytest.mark.parametrize("L", (2, 9, 129, 1000, 4096))
def test_t5_rel_table_more_lengths(gpu, L, heads):
    from unigen_amd import lib, ops
    w = torch.randn(32, heads, generator=torch.Generator().manual_seed(heads * 7 + L)).to(BF)
    want = R.t5_rel_table(w.float(), L, 32, 128)
    for dt in (BF, F32):
        got = ops.t5_rel_table(w.to(device=gpu, dtype=dt), L, num_buckets=32, max_distance=128).cpu()
        assert got.shape == (heads, 2 * L - 1) and got.dtype == F32 and torch.equal(got, want)
        if L == 2:
            with pytest.raises(lib.UniGenHipError):
                ops.t5_rel_table(torch.zeros(30, heads, device=gpu, dtype=dt), L, num_buckets=30, max_distance=128)
            with pytest.raises(lib.UniGenHipError):
                ops.t5_rel_table(w.to(device=gpu, dtype=dt), L, num_buckets=32, max_distance=8)             # max_distance = num_buckets / 4
            fn = lib.load().ug_t5_rel_table if dt == BF else lib.load().ug_t5_rel_table_f32                  # L = 0: no table that ops could allocate
            assert fn(w.to(device=gpu, dtype=dt).data_ptr(), 32, 128, heads, 0, got.to(gpu).data_ptr(), None) == lib.UG_ERR_BAD_SHAPE


# ---- the model's table cache -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_t5_state():
    from safetensors.torch import load_file
    return R.decode_state(load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_tiny.safetensors")), "t5.w.")


def _fresh_t5(gpu, sd):
    from unigen_amd.text import T5EncoderModel
    m = T5EncoderModel.from_config(R.T5_TINY, device=gpu, dtype=BF)
    m.load_state_dict(sd)
    return m


def test_t5_table_cache_follows_the_weights(gpu):
    sd = _tiny_t5_state()
    g = torch.Generator().manual_seed(11)
    ids = {L: torch.randint(2, 64, (2, L), generator=g) for L in (77, 200)}
    bits = lambda t: t.cpu().view(torch.int16)
    m = _fresh_t5(gpu, sd)
    a77, a200, b77 = (bits(m(ids[L])[0]) for L in (77, 200, 77))
    assert sorted(m._tables) == [77, 200]
    assert torch.equal(a77, b77), "the second run at length 77 differs from the first"
    for L, got in ((77, a77), (200, a200)):
        assert torch.equal(got, bits(_fresh_t5(gpu, sd)(ids[L])[0])), f"length {L} differs from a fresh model's"
    name = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    sd2 = dict(sd)
    sd2[name] = R.bf(sd[name].double().flip(0) * 1.5 + 0.25).float()
    m.load_state_dict(sd2)
    assert not m._tables
    for L in (77, 200):
        got = bits(m(ids[L])[0])
        assert torch.equal(got, bits(_fresh_t5(gpu, sd2)(ids[L])[0])), f"length {L} after load_state_dict differs from a fresh model with those weights"
        assert not torch.equal(got, a77 if L == 77 else a200), "the new bias weights changed nothing: the test has no teeth"
