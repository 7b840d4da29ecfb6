"""GPU tests of the Gemma-2 text encoder (unigen_amd/csrc/text.hip, unigen_amd/gemma.py) against the float64 references of tests/gemma_ref.py, which
tests/test_gemma_ref_cpu.py pins against transformers. No test here imports transformers or reads anything outside the repository.

Bounds (docs/PARITY_TOLERANCES.md, "Gemma-2 text encoder"):
  attention   bf16: rel-L2 and the worst query row <= max(1.5 x the same metric of the rounding-point variant - P rounded to bf16 as the P.V operand,
              the output rounded - against the same float64 truth, 2^-9). fp32 twin without a cap: rel-L2 <= 1e-5, every row <= 1e-4 (the existing
              twin bound); with a cap: <= max(that, 4 x the error of a float32 host evaluation of gemma_ref's formula against the float64 truth) - the
              factor 4 is room for the device's tanhf beside the host's. Rows that must not see the 1e4 values planted in V (the future, beyond
              kv_len, behind the window) are measured apart from the rows that legitimately see some.
  element-wise (RoPE, norm, scaled gather): per element half a bf16 ulp per rounding point, the inner ones carried through what follows them (the outer
              half ulp is taken at |truth| + the inner terms: the rounded operands may lie in the next binade), plus 2^-20 of the magnitudes that
              enter in fp32. fp32 twins: the 2^-20 term alone.
  models      fp32 path against the fixture's transformers outputs: rel-L2 <= 1e-5; bf16 path against the same truth: <= 1.5 x the error of a
              bf16-rounded run of gemma_ref. All rows count: a padded row depends on the mask.
"""
import functools
import os

import pytest
import torch

from tests import gemma_ref as R
from tests.text_ref import FP32_TERM, half_ulp, worst_row
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemma_tiny.safetensors")
TINY = 2.0 ** -126
DH, SCALE = 256, 256 ** -0.5


# ---- attention -------------------------------------------------------------------------------------------------------------------
ATT_L = (1, 31, 32, 33, 63, 64, 65, 129, 300)
LAYOUTS = ((4, 2), (2, 2), (2, 1))
CAPS, WINDOWS = (0.0, 50.0, 4.0), (0, 8)


@functools.lru_cache(maxsize=None)
def attn_case(L: int, H: int, KV: int):
    """bf16-representable q [2, L, H, 256] and k [2, L, KV, 256] at standard deviation 2 (q.k / 16 then has standard deviation about 4), v at 1; the K/V
    heads are independent draws, so a wrong group mapping reads different numbers."""
    g = torch.Generator().manual_seed(1000 * L + 10 * H + KV)
    q = R.bf(torch.randn(2, L, H, DH, generator=g, dtype=F64) * 2.0)
    k = R.bf(torch.randn(2, L, KV, DH, generator=g, dtype=F64) * 2.0)
    v = R.bf(torch.randn(2, L, KV, DH, generator=g, dtype=F64))
    return q, k, v


def leak_v(v, L: int, window: int, kv_len):
    """-> (v with 1e4 at keys some rows must not see, clean rows, dirty rows). The future: keys above q0 = L / 2; behind the window: keys below
    a = q0 - window - 3; beyond kv_len: keys from kv_len[b] on (no row sees those). Rows in [a + window - 1, q0] see none of them."""
    v = v.clone()
    q0 = L // 2
    big = R.bf(torch.tensor(1e4, dtype=F64))
    v[:, q0 + 1:] = big
    a = max(q0 - window - 3, 0) if window else 0
    v[:, :a] = big
    if kv_len is not None:
        for b, n in enumerate(kv_len):
            v[b, n:] = big
    first = a + window - 1 if a else 0
    clean = torch.arange(first, q0 + 1)
    dirty = torch.tensor([r for r in range(L) if r < first or r > q0], dtype=torch.int64)
    return v, clean, dirty


def run_attn(gpu, dt, q, k, v, cap, window, kv_len):
    from unigen_amd import ops
    B, L, H, _ = q.shape
    KV = k.shape[2]
    W = (H + 2 * KV) * DH
    qkv = torch.cat([q.reshape(B, L, H * DH), k.reshape(B, L, KV * DH), v.reshape(B, L, KV * DH)], -1).to(device=gpu, dtype=dt).contiguous()
    out = torch.full((B, L, H * DH), float("nan"), device=gpu, dtype=dt)
    flat = qkv.view(B * L, W)
    kvl = None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32, device=gpu)
    s3 = (W, L * W)
    ops.flash_attn_softcap(flat, flat[:, H * DH:], flat[:, (H + KV) * DH:], out, batches=B, heads=H, kv_heads=KV, dh=DH, L_=L, q_strides=s3, k_strides=s3,
                           v_strides=s3, o_strides=(H * DH, L * H * DH), scale=SCALE, softcap=cap, window=window, kv_len=kvl)
    torch.cuda.synchronize()
    return out.cpu().view(B, L, H, DH)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda t: f"h{t[0]}kv{t[1]}")
@pytest.mark.parametrize("L", ATT_L)
def test_flash_attn_softcap(gpu, L, layout):
    """Every (cap, window, kv_len) of the sweep on one shape. fp32 figures measured on an MI355X, worst over the sweep, are in
    docs/PARITY_TOLERANCES.md."""
    H, KV = layout
    q, k, v0 = attn_case(L, H, KV)
    if L >= 31:          # a row of one key has no softmax; from 31 keys on the cap of 4 must be visible in the truth itself
        on, off = R.attention(q, k, v0, SCALE, 4.0), R.attention(q, k, v0, SCALE, 0.0)
        bound = max(1.5 * rel_l2(R.attention(q, k, v0, SCALE, 4.0, rnd=R.bf), on), 2.0 ** -9)
        assert rel_l2(on, off) > 10 * bound, (rel_l2(on, off), bound)
    first = True
    for kv_len in (None, [L, max(1, 2 * L // 3)]):
        for window in WINDOWS:
            v, clean, dirty = leak_v(v0, L, window, kv_len)
            for cap in CAPS:
                truth = R.attention(q, k, v, SCALE, cap, window, kv_len)
                variant = R.attention(q, k, v, SCALE, cap, window, kv_len, rnd=R.bf)
                host32 = R.attention(q, k, v, SCALE, cap, window, kv_len, dtype=F32) if cap else None
                for dt in (BF, F32):
                    got = run_attn(gpu, dt, q, k, v, cap, window, kv_len)
                    assert torch.isfinite(got).all()
                    if first and dt == BF:
                        assert torch.equal(got, run_attn(gpu, dt, q, k, v, cap, window, kv_len)), "two runs differ"
                        first = False
                    for name, rows in (("clean", clean), ("dirty", dirty)):
                        if rows.numel() == 0:
                            continue
                        g, t = got[:, rows], truth[:, rows]
                        e, ew = rel_l2(g, t), worst_row(g, t)
                        if dt == BF:
                            va = variant[:, rows]
                            b, bw = max(1.5 * rel_l2(va, t), 2.0 ** -9), max(1.5 * worst_row(va, t), 2.0 ** -9)
                        elif cap:
                            h32 = host32[:, rows]
                            he, hew = rel_l2(h32, t), worst_row(h32, t)
                            b, bw = max(1e-5, 4 * he), max(1e-4, 4 * hew)
                            print(f"GEMMA attn L={L} H={H}/{KV} cap={cap} window={window} kv_len={kv_len} host-f32 {name}: rel_l2 {he:.3e} worst row {hew:.3e}")
                        else:
                            b, bw = 1e-5, 1e-4
                        print(f"GEMMA attn L={L} H={H}/{KV} cap={cap} window={window} kv_len={kv_len} {'bf16' if dt == BF else 'f32'} {name}: "
                              f"rel_l2 {e:.3e} (bound {b:.3e}) worst row {ew:.3e} (bound {bw:.3e})")
                        assert e <= b and ew <= bw, (L, layout, cap, window, kv_len, dt, name, e, b, ew, bw)


# ---- RoPE, norm, scaled gather -----------------------------------------------------------------------------------------------------------
def row_magnitudes(rows):
    return torch.tensor([1.0, 1e-3, 1e3], dtype=F64)[torch.arange(rows) % 3][:, None]


@pytest.mark.parametrize("layout", ((8, 4), (2, 1)), ids=lambda t: f"h{t[0]}kv{t[1]}")
@pytest.mark.parametrize("L", (1, 24, 300))
def test_rope_half(gpu, L, layout):
    from unigen_amd import ops
    from unigen_amd.gemma import rope_table
    H, KV = layout
    B, nh, W = 2, H + KV, (H + 2 * KV) * DH
    g = torch.Generator().manual_seed(31 * L + H)
    x = R.bf(torch.randn(B * L, W, generator=g, dtype=F64) * row_magnitudes(B * L))
    for dt in (BF, F32):
        cos, sin = rope_table(L, DH, 10000.0, dt)
        assert all(torch.equal(a, b.to(dt)) for a, b in zip((cos, sin), R.rope_table(L, DH)))
        buf = x.to(device=gpu, dtype=dt)
        ops.rope_half(buf, cos.to(gpu), sin.to(gpu), rows_per_batch=L, col0=0, nheads=nh, dh=DH)
        torch.cuda.synchronize()
        got = buf.cpu()
        assert torch.equal(got[:, nh * DH:].view(torch.int16 if dt == BF else torch.int32), x[:, nh * DH:].to(dt).view(torch.int16 if dt == BF else torch.int32)), \
            "the v columns changed"
        xs = x[:, :nh * DH].view(B, L, nh, DH)
        c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
        lo, hi = xs[..., :DH // 2], xs[..., DH // 2:]
        terms = ((lo * c, -(hi * s)), (hi * c, lo * s))
        truth = torch.cat([a + b for a, b in terms], -1)
        fp32 = torch.cat([FP32_TERM * (a.abs() + b.abs()) for a, b in terms], -1)
        inner = torch.cat([half_ulp(a) + half_ulp(b) for a, b in terms], -1)
        bound = fp32 + ((inner + half_ulp(truth.abs() + inner)) if dt == BF else 0) + TINY
        assert torch.equal(R.rope(xs, cos, sin), truth)
        excess = ((got[:, :nh * DH].double().view(B, L, nh, DH) - truth).abs() / bound).max()
        print(f"GEMMA rope L={L} heads={H}+{KV} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


@pytest.mark.parametrize("rows", (1, 77, 600))
@pytest.mark.parametrize("D", (8, 128, 2304, 4608, 4616))          # 4616: past the one-pass width, the row is read twice
@pytest.mark.parametrize("residual", (False, True))
def test_gemma_rmsnorm_rows(gpu, residual, D, rows):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(rows * 7919 + D)
    mag = row_magnitudes(rows)
    x = R.bf(torch.randn(rows, D, generator=g, dtype=F64) * mag)
    w = R.bf(0.3 * torch.randn(D, generator=g, dtype=F64))
    res = R.bf(torch.randn(rows, D, generator=g, dtype=F64) * row_magnitudes(rows + 1)[1:]) if residual else None
    eps = 1e-6
    t = R.rmsnorm(x, w, eps)
    truth = t if res is None else res + t
    assert torch.equal(truth, R.rmsnorm(x, w, eps, res))
    fp32 = FP32_TERM * (t.abs() + (res.abs() if residual else 0))
    for dt in (BF, F32):
        got = ops.gemma_rmsnorm_rows(x.to(device=gpu, dtype=dt), w.to(device=gpu, dtype=dt), eps,
                                     residual=res.to(device=gpu, dtype=dt) if residual else None).cpu().double()
        if dt == BF:
            bf = (half_ulp(t) + half_ulp(truth.abs() + half_ulp(t))) if residual else half_ulp(t)
        else:
            bf = 0
        excess = ((got - truth).abs() / (fp32 + bf + TINY)).max()
        print(f"GEMMA rmsnorm D={D} rows={rows} residual={residual} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


def test_gemma_rmsnorm_in_place(gpu):
    """out may be x, or the residual: the same bits as with a fresh output (the model's layers write both sums over the projection's output)"""
    from unigen_amd import ops
    g = torch.Generator().manual_seed(5)
    for D in (2304, 4616):
        x, res = (torch.randn(77, D, generator=g).to(device=gpu, dtype=BF) for _ in range(2))
        w = (0.3 * torch.randn(D, generator=g)).to(device=gpu, dtype=BF)
        want = ops.gemma_rmsnorm_rows(x, w, 1e-6, residual=res)
        x2, res2 = x.clone(), res.clone()
        assert torch.equal(ops.gemma_rmsnorm_rows(x2, w, 1e-6, residual=res, out=x2), want)
        assert torch.equal(ops.gemma_rmsnorm_rows(x, w, 1e-6, residual=res2, out=res2), want)


@pytest.mark.parametrize("rows", (1, 77, 600))
@pytest.mark.parametrize("D", (8, 128, 2304, 4608))
def test_gather_rows_scaled(gpu, D, rows):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(rows + D)
    src = R.bf(torch.randn(50, D, generator=g, dtype=F64) * row_magnitudes(50))
    idx = torch.randint(0, 50, (rows,), generator=g, dtype=torch.int32)
    idx[rows // 2] = -1
    for dt in (BF, F32):
        scale = float(torch.tensor(D ** 0.5).to(dt))
        truth = R.embed(src, idx.clamp_min(0), scale)
        truth[idx < 0] = 0
        out = torch.full((rows, D), float("nan"), device=gpu, dtype=dt)
        got = ops.gather_rows_scaled(src.to(device=gpu, dtype=dt), idx.to(gpu), scale, out).cpu().double()
        bound = FP32_TERM * truth.abs() + (half_ulp(truth) if dt == BF else 0) + TINY
        excess = ((got - truth).abs() / bound).max()
        print(f"GEMMA gather D={D} rows={rows} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0 and (got[idx < 0] == 0).all()


# ---- whole models ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


def build_model(gpu, tag, dt):
    from unigen_amd.gemma import Gemma2Model
    cfg, std, seed = R.TINY[tag]
    m = Gemma2Model.from_config(cfg, device=gpu, dtype=dt)
    m.load_state_dict(R.tiny_state(cfg, std, seed))
    return m


@pytest.mark.parametrize("tag", ("a", "b"))
def test_tiny_gemma_matches_transformers(gpu, tag):
    g = golden()
    cfg, std, seed = R.TINY[tag]
    ids, mask = g["ids"], g["mask"]
    truth, truth0 = g[f"{tag}.out.mask"].double(), g[f"{tag}.out.nomask"].double()
    e_var = rel_l2(R.model(R.tiny_state(cfg, std, seed), cfg, ids.long(), mask.long(), R.bf), truth)
    m32 = build_model(gpu, tag, F32)
    e32, e32_0 = rel_l2(m32(ids, attention_mask=mask)[0].cpu(), truth), rel_l2(m32(ids)[0].cpu(), truth0)
    out = build_model(gpu, tag, BF)(ids.to(gpu), attention_mask=mask.to(gpu))
    assert out.last_hidden_state.dtype == BF and tuple(out[0].shape) == (2, R.TINY_L, 128) and torch.isfinite(out[0]).all()
    e16 = rel_l2(out[0].cpu(), truth)
    print(f"GEMMA tiny {tag}: fp32 path {e32:.3e} with the mask, {e32_0:.3e} without (bound 1e-5); bf16 path {e16:.3e}, bf16-rounded reference {e_var:.3e}, "
          f"ratio {e16 / e_var:.3f} (bound 1.5)")
    assert e32 <= 1e-5 and e32_0 <= 1e-5 and e16 <= 1.5 * e_var


def test_tiny_gemma_window_matches_transformers(gpu):
    """gemma_ref.TINY_WINDOW: sliding layers with a window of 40 on 100 tokens (more than a 32-key tile, less than the prompt), the second sample with 37
    live tokens, under the model bounds above. The truth is the fixture's transformers output; on the 24 padded rows of the second sample that have
    no live key in a sliding layer the module (float64) has NaN, and the truth there is gemma_ref's float64 run with its defined zero attention
    (tests/test_gemma_ref_cpu.py pins that run against the module on every other row). All rows count."""
    from safetensors.torch import load_file
    from unigen_amd.gemma import Gemma2Model
    g = load_file(os.path.join(os.path.dirname(GOLDEN), "gemma_tiny_window.safetensors"))
    cfg, std, seed = R.TINY_WINDOW
    sd = R.tiny_state(cfg, std, seed)
    ids, mask = g["ids"], g["mask"]
    ref = R.model(sd, cfg, ids.long(), mask.long())
    dead = R.window_dead_rows(cfg, mask.long())
    truth, truth0 = g["c.out.mask"].double(), g["c.out.nomask"].double()
    assert torch.equal(torch.isnan(truth).any(-1), dead) and int(dead.sum()) == 24
    truth = torch.where(dead[..., None], ref, truth)
    e_var = rel_l2(R.model(sd, cfg, ids.long(), mask.long(), R.bf), truth)

    def build(dt):
        m = Gemma2Model.from_config(cfg, device=gpu, dtype=dt)
        m.load_state_dict(sd)
        return m
    m32 = build(F32)
    o32 = m32(ids, attention_mask=mask)[0].cpu()
    e32, e32_0, e32_dead = rel_l2(o32, truth), rel_l2(m32(ids)[0].cpu(), truth0), rel_l2(o32[dead], truth[dead])
    out = build(BF)(ids.to(gpu), attention_mask=mask.to(gpu))
    assert out.last_hidden_state.dtype == BF and tuple(out[0].shape) == (2, R.WINDOW_L, 128) and torch.isfinite(out[0]).all()
    e16 = rel_l2(out[0].cpu(), truth)
    print(f"GEMMA tiny window: fp32 path {e32:.3e} with the mask ({e32_dead:.3e} on the rows without a live key), {e32_0:.3e} without (bound 1e-5); "
          f"bf16 path {e16:.3e}, bf16-rounded reference {e_var:.3e}, ratio {e16 / e_var:.3f} (bound 1.5)")
    assert e32 <= 1e-5 and e32_0 <= 1e-5 and e32_dead <= 1e-5 and e16 <= 1.5 * e_var


def test_gemma_layer_at_2b_geometry(gpu):
    """One gemma-2-2b layer (hidden 2304, 8 query heads over 4 K/V heads of 256, feed-forward 9216) on B = 2, L = 300, the second sample with 211 live
    tokens: the packed GEMMs, the RoPE launch and the grouped attention at their real shapes, checked on 26 rows of each sample (first, last, tile
    and key-length edges, random) against float64 with fp32 key / value projections."""
    from unigen_amd.gemma import Gemma2Model
    cfg = dict(R.TINY_A, hidden_size=2304, num_attention_heads=8, num_key_value_heads=4, intermediate_size=9216, num_hidden_layers=1, vocab_size=8,
               layer_types=["sliding_attention"])
    B, L, live = 2, 300, 211
    m = Gemma2Model.from_config(cfg, device=gpu, dtype=BF)
    g = torch.Generator(device=gpu).manual_seed(5)
    for name, t in m.state_dict().items():
        t.copy_(torch.randn(t.shape, generator=g, device=gpu) * ((0.7 / t.shape[1] ** 0.5) if t.dim() == 2 else 0.1))
    x = torch.randn(B * L, 2304, generator=g, device=gpu).to(BF)
    kv_len = torch.tensor([L, live], dtype=torch.int32, device=gpu)
    got = m.layer(x.clone(), 0, B, L, m.rope(L), kv_len)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    rows = torch.tensor(sorted({0, 1, 31, 32, 127, 128, 210, 211, 212, 255, 256, 287, 288, 299} |
                               set(torch.randint(0, L, (12,), generator=torch.Generator().manual_seed(1)).tolist())))
    x64 = x.cpu().double().view(B, L, -1)
    cos, sin = (t.to(BF).double() for t in R.rope_table(L, DH))
    truth = R.layer_rows(sd, cfg, 0, x64, cos, sin, rows, kv_len.cpu(), None, F32)
    var = R.layer_rows(sd, cfg, 0, x64, cos, sin, rows, kv_len.cpu(), R.bf, F32)
    gr = got.cpu().view(B, L, -1)[:, rows]
    e, ew, e_var, ew_var = rel_l2(gr, truth), worst_row(gr, truth), rel_l2(var, truth), worst_row(var, truth)
    print(f"GEMMA 2b layer: bf16 path rel_l2 {e:.3e} worst row {ew:.3e}; bf16-rounded reference {e_var:.3e} / {ew_var:.3e}, ratios {e / e_var:.3f} / "
          f"{ew / ew_var:.3f} (bound 1.5)")
    assert e <= 1.5 * e_var and ew <= 1.5 * ew_var


def test_sana_takes_the_encoded_prompt(gpu):
    """A tiny Gemma2Model (hidden 128) feeds a tiny SanaTransformer2DModel with caption_channels = 128: encode_prompt_sana from ids + mask gives the
    model's own rows [0] + [-T + 1 .. -1], and the Sana forward takes them with the returned mask."""
    from tests import sana_ref as S
    from unigen_amd.gemma import encode_prompt_sana
    from unigen_amd.sana import SanaTransformer2DModel
    g = golden()
    enc = build_model(gpu, "a", BF)
    ids, mask = g["ids"], g["mask"]
    T = 16
    embeds, emask = encode_prompt_sana(enc, None, None, max_sequence_length=T, text_input_ids=ids, attention_mask=mask)
    sel = [0] + list(range(-T + 1, 0))
    direct = enc(ids, attention_mask=mask)[0]
    assert embeds.dtype == BF and tuple(embeds.shape) == (2, T, 128) and torch.equal(embeds, direct[:, sel])
    assert torch.equal(emask.cpu(), mask[:, sel]) and emask[1].sum() == R.TINY_LIVE - (R.TINY_L - T)
    e2, m2 = encode_prompt_sana(enc, None, None, max_sequence_length=T, text_input_ids=ids, attention_mask=mask, num_images_per_prompt=2)
    assert torch.equal(e2, embeds.repeat_interleave(2, 0)) and torch.equal(m2, emask.repeat_interleave(2, 0))
    cfg = dict(S.TINY["a"], caption_channels=128)
    sana = SanaTransformer2DModel(cfg, device=gpu, dtype=BF).init_synthetic_(3)
    lat = torch.randn(2, cfg["in_channels"], 4, 6, generator=torch.Generator().manual_seed(2)).to(device=gpu, dtype=BF)
    out = sana.forward(lat, encoder_hidden_states=embeds, timestep=torch.tensor([999.0, 37.0], device=gpu), encoder_attention_mask=emask)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, cfg["out_channels"], 4, 6) and torch.isfinite(out).all()
