"""GPU tests of the text encoders (unigen_amd/csrc/text.hip, unigen_amd/text.py) against the float64 references of tests/text_ref.py, which
tests/test_text_ref_cpu.py pins against transformers.

Bounds (docs/PARITY_TOLERANCES.md, "Text encoders"):
  attention   bf16: rel-L2 and the worst query row <= max(1.5 x the same metric of the rounding-point variant - P rounded to bf16 as the P.V operand,
              the output rounded - against the same float64 truth, 2^-9); fp32 twin: rel-L2 <= 1e-5, every row <= 1e-4 (the existing twin bound).
              With neither a table nor the mask the result is bit-identical to ug_flash_attn_fwd.
  rel table   bit-exact.
  element-wise (norms, activations): per element within one bf16 ulp of the float64 value plus 2^-20 of the magnitudes that enter in fp32. One ulp is
              two roundings of half an ulp: where the module itself rounds twice (T5LayerNorm: bf16(x rs) then bf16(w .); gated GELU: bf16(gelu) then
              bf16(. b)) the inner half ulp is taken at the inner value and carried through the factor that multiplies it. fp32 twins: the 2^-20 term alone.
  models      fp32 path against the fixture's transformers outputs: rel-L2 <= 1e-5; bf16 path against the same truth: <= 1.5 x the error of a
              bf16-rounded run of text_ref.
"""
import functools
import math
import os

import pytest
import torch

from tests import text_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_tiny.safetensors")
FP32_TERM, half_ulp, worst_row = R.FP32_TERM, R.half_ulp, R.worst_row       # shared with the sweep (tests/test_fuzz_text_gpu.py)


# ---- attention -------------------------------------------------------------------------------------------------------------------
ATT_L = (1, 63, 64, 65, 77, 200, 512)
MODES = {"bias": (True, False), "causal": (False, True), "bias_causal": (True, True), "neither": (False, False)}


@functools.lru_cache(maxsize=None)
def attn_case(Lq: int):
    """bf16-representable q, k, v [2, L, 2, 64], a table [2, 2L - 1] with distinct large values where an index slip would land, and float64 truths."""
    g = torch.Generator().manual_seed(100 + Lq)
    q, k, v = (R.bf(torch.randn(2, Lq, 2, 64, generator=g, dtype=F64) * s) for s in (0.5, 1.0, 1.0))
    table = torch.randn(2, 2 * Lq - 1, generator=g, dtype=F32)
    c = Lq - 1
    for off, val in ((0, 4.0), (1, -5.0), (-1, 6.0), (Lq - 1, -7.0), (-(Lq - 1), 8.0)):
        if abs(off) <= Lq - 1:
            table[0, c + off] = val
            table[1, c + off] = -val + 0.5
    q0 = Lq // 2
    v_leak = v.clone()
    v_leak[:, q0 + 1:] = R.bf(torch.tensor(1e4, dtype=F64))       # keys a causal row q <= q0 must not see
    return dict(q=q, k=k, v=v, v_leak=v_leak, table=table, q0=q0)


@functools.lru_cache(maxsize=None)
def attn_truth(Lq: int, mode: str):
    c = attn_case(Lq)
    bias, causal = MODES[mode]
    scale = 1.0 if bias and not causal else 64 ** -0.5
    v = c["v_leak"] if causal else c["v"]
    args = (c["q"], c["k"], v, scale, c["table"] if bias else None, causal)
    return scale, v, R.attention(*args), R.attention(*args, rnd=R.bf)


def run_attn(gpu, dt, q, k, v, scale, table, causal, plain=False):
    from unigen_amd import ops
    B, Lq, H, dh = q.shape
    qkv = torch.cat([q.reshape(B, Lq, H * dh), k.reshape(B, Lq, H * dh), v.reshape(B, Lq, H * dh)], -1).to(device=gpu, dtype=dt).contiguous()
    out = torch.full((B, Lq, H * dh), float("nan"), device=gpu, dtype=dt)
    W = 3 * H * dh
    kw = dict(batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lq, q_strides=(W, Lq * W), k_strides=(W, Lq * W), v_strides=(W, Lq * W), o_strides=(H * dh, Lq * H * dh), scale=scale)
    flat = qkv.view(B * Lq, W)
    if plain:
        ops.flash_attn(flat, flat[:, H * dh:], flat[:, 2 * H * dh:], out, **kw)
    else:
        ops.flash_attn_bias(flat, flat[:, H * dh:], flat[:, 2 * H * dh:], out, rel_table=table.to(gpu) if table is not None else None, causal=causal, **kw)
    torch.cuda.synchronize()
    return out.cpu().view(B, Lq, H, dh)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("Lq", ATT_L)
def test_flash_attn_bias(gpu, Lq, mode):
    c = attn_case(Lq)
    bias, causal = MODES[mode]
    scale, v, truth, variant = attn_truth(Lq, mode)
    table = c["table"] if bias else None
    for dt in (BF, F32):
        got = run_attn(gpu, dt, c["q"], c["k"], v, scale, table, causal)
        assert torch.isfinite(got).all()
        if mode == "neither":
            assert torch.equal(got, run_attn(gpu, dt, c["q"], c["k"], v, scale, None, False, plain=True)), "not bit-identical to ug_flash_attn_fwd"
        # with the mask, rows up to q0 must not see the 1e4 values behind them; measured separately from the rows that legitimately do
        parts = [("rows<=q0", slice(0, c["q0"] + 1)), ("rows>q0", slice(c["q0"] + 1, Lq))] if causal else [("all", slice(0, Lq))]
        for name, sl in parts:
            if sl.start >= min(sl.stop, Lq):
                continue
            g, t, va = got[:, sl], truth[:, sl], variant[:, sl]
            e, ew = rel_l2(g, t), worst_row(g, t)
            if dt == BF:
                b, bw = max(1.5 * rel_l2(va, t), 2.0 ** -9), max(1.5 * worst_row(va, t), 2.0 ** -9)
            else:
                b, bw = 1e-5, 1e-4
            print(f"TEXT attn L={Lq} {mode} {'bf16' if dt == BF else 'f32'} {name}: rel_l2 {e:.3e} (bound {b:.3e}) worst row {ew:.3e} (bound {bw:.3e})")
            assert e <= b and ew <= bw, (Lq, mode, dt, name, e, b, ew, bw)


def test_fp32_twin_with_a_zero_table_is_the_plain_fp32_reference(gpu):
    """ug_flash_attn_fwd_bias_f32 and ug_flash_attn_fwd_f32 are two instantiations of one kernel (csrc/verify_f32.hip): with an all-zero table and no
    mask the biased one gives the plain one's bits. B = 2, H = 3, Lq = 70, Lkv = 65 (a ragged last 64-row block whose spare lanes re-read the
    clamped row, keys past one 64-key tile), operands the column blocks of one packed [B, L, 3 H 64] buffer. With the mask added, the same call
    meets the float64 reference at the twin's bound (rel-L2 <= 1e-5, every row <= 1e-4)."""
    from unigen_amd import ops
    B, H, Lq, Lkv, dh = 2, 3, 70, 65, 64
    D, W = H * dh, 3 * H * dh
    g = torch.Generator().manual_seed(7065)
    qkv = torch.randn(B, Lq, W, generator=g, dtype=F32)
    dev = qkv.to(gpu)
    flat = dev.view(B * Lq, W)
    zero = torch.zeros(H, 2 * Lq - 1, dtype=F32, device=gpu)
    kw = dict(batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(W, Lq * W), k_strides=(W, Lq * W), v_strides=(W, Lq * W), o_strides=(D, Lq * D), scale=dh ** -0.5)

    def run(fn, **extra):
        out = torch.full((B, Lq, D), float("nan"), device=gpu, dtype=F32)
        fn(flat, flat[:, D:], flat[:, 2 * D:], out, **kw, **extra)
        torch.cuda.synchronize()
        return out.cpu()

    plain, biased = run(ops.flash_attn), run(ops.flash_attn_bias, rel_table=zero, causal=False)
    assert torch.isfinite(plain).all() and torch.equal(plain.view(torch.int32), biased.view(torch.int32)), "a zero table changed the plain reference's bits"
    q, k, v = (qkv[:, :L_, i * D:(i + 1) * D].reshape(B, L_, H, dh) for i, L_ in ((0, Lq), (1, Lkv), (2, Lkv)))
    truth = R.attention(q, k, v, dh ** -0.5, zero.cpu(), True)
    got = run(ops.flash_attn_bias, rel_table=zero, causal=True).view(B, Lq, H, dh)
    e, ew = rel_l2(got, truth), worst_row(got, truth)
    print(f"TEXT attn f32 zero table + causal Lq={Lq} Lkv={Lkv}: rel_l2 {e:.3e} (bound 1e-5) worst row {ew:.3e} (bound 1e-4)")
    assert e <= 1e-5 and ew <= 1e-4, (e, ew)


@pytest.mark.parametrize("heads", (2, 64))
@pytest.mark.parametrize("Lq", (1, 77, 512))
def test_t5_rel_table_bit_exact(gpu, Lq, heads):
    from unigen_amd import ops
    w = torch.randn(32, heads, generator=torch.Generator().manual_seed(heads + Lq)).to(BF)
    for dt in (BF, F32):
        got = ops.t5_rel_table(w.to(device=gpu, dtype=dt), Lq, num_buckets=32, max_distance=128).cpu()
        assert got.shape == (heads, 2 * Lq - 1) and torch.equal(got, R.t5_rel_table(w.float(), Lq, 32, 128))


# ---- norms -----------------------------------------------------------------------------------------------------------------------
def norm_inputs(rows, D):
    g = torch.Generator().manual_seed(rows * 7919 + D)
    mag = torch.tensor([1.0, 1e-3, 1e3])[torch.arange(rows) % 3][:, None]
    x = torch.randn(rows, D, generator=g) * mag
    x[rows // 2] += 3 * mag[rows // 2]                        # one row with a mean away from zero
    return R.bf(x.double()), R.bf(1 + 0.2 * torch.randn(D, generator=g).double()), R.bf(0.2 * torch.randn(D, generator=g).double())


@pytest.mark.parametrize("rows", (1, 77, 1030))
@pytest.mark.parametrize("D", (8, 128, 768, 4096, 4104))
def test_rmsnorm_rows(gpu, D, rows):
    from unigen_amd import ops
    x, w, _ = norm_inputs(rows, D)
    eps = 1e-6
    u = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    truth = w * u
    fp32 = FP32_TERM * truth.abs()
    for dt in (BF, F32):
        got = ops.rmsnorm_rows(x.to(device=gpu, dtype=dt), w.to(device=gpu, dtype=dt), eps).cpu().double()
        bound = fp32 + ((half_ulp(truth) + w.abs() * half_ulp(u)) if dt == BF else 0) + 2.0 ** -126
        excess = ((got - truth).abs() / bound).max()
        print(f"TEXT rmsnorm D={D} rows={rows} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


@pytest.mark.parametrize("rows", (1, 77, 1030))
@pytest.mark.parametrize("D", (8, 128, 768, 4096, 4104))
def test_layernorm_rows(gpu, D, rows):
    from unigen_amd import ops
    x, w, b = norm_inputs(rows, D)
    eps = 1e-5
    truth = R.layernorm(x, w, b, eps)
    mu = x.mean(-1, keepdim=True)
    rs = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    fp32 = FP32_TERM * ((x.abs() + mu.abs()) * rs * w.abs() + b.abs())
    for dt in (BF, F32):
        got = ops.layernorm_rows(x.to(device=gpu, dtype=dt), w.to(device=gpu, dtype=dt), b.to(device=gpu, dtype=dt), eps).cpu().double()
        bound = fp32 + (half_ulp(truth) if dt == BF else 0) + 2.0 ** -126
        excess = ((got - truth).abs() / bound).max()
        print(f"TEXT layernorm D={D} rows={rows} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


# ---- activations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 8000, 8 * 1001))
def test_gated_gelu(gpu, n):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(n)
    ab = R.bf(torch.cat([torch.randn(3, n, generator=g) * 3, torch.randn(3, n, generator=g)], -1).double())
    a, b = ab[:, :n], ab[:, n:]
    gl = R.gelu_new(a)
    truth = gl * b
    for dt in (BF, F32):
        got = ops.gated_gelu(ab.to(device=gpu, dtype=dt)).cpu().double()
        bound = FP32_TERM * (a.abs() * b.abs()) + ((half_ulp(truth) + b.abs() * half_ulp(gl)) if dt == BF else 0) + 2.0 ** -126
        excess = ((got - truth).abs() / bound).max()
        print(f"TEXT gated_gelu n={n} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


@pytest.mark.parametrize("n", (8, 8000, 8 * 1001))
def test_quick_gelu(gpu, n):
    from unigen_amd import ops
    x = R.bf((torch.randn(n, generator=torch.Generator().manual_seed(n)) * 4).double())
    truth = R.quick_gelu(x)
    for dt in (BF, F32):
        got = ops.quick_gelu(x.to(device=gpu, dtype=dt)).cpu().double()
        bound = FP32_TERM * x.abs() + (R.bf16_ulp(truth) if dt == BF else 0) + 2.0 ** -126
        excess = ((got - truth).abs() / bound).max()
        print(f"TEXT quick_gelu n={n} {dt}: worst |err| / bound = {float(excess):.3f}")
        assert excess <= 1.0


# ---- whole models ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


def build_models(gpu, dt):
    from unigen_amd.text import CLIPTextModel, T5EncoderModel
    g = golden()
    t5 = T5EncoderModel.from_config(R.T5_TINY, device=gpu, dtype=dt)
    t5.load_state_dict(R.decode_state(g, "t5.w."))
    clip = CLIPTextModel.from_config(R.CLIP_TINY, device=gpu, dtype=dt)
    clip.load_state_dict(R.decode_state(g, "clip.w."))
    return t5, clip


def test_tiny_t5_matches_transformers(gpu):
    g = golden()
    truth = g["t5.out.last_hidden_state"].double()
    e_var = rel_l2(R.t5_encoder(R.decode_state(g, "t5.w."), R.T5_TINY, g["t5.ids"], R.bf), truth)
    e32 = rel_l2(build_models(gpu, F32)[0](g["t5.ids"])[0].cpu(), truth)
    out = build_models(gpu, BF)[0](g["t5.ids"])
    assert out.last_hidden_state.dtype == BF and tuple(out[0].shape) == (1, 200, 128)
    e16 = rel_l2(out[0].cpu(), truth)
    print(f"TEXT tiny T5: fp32 path {e32:.3e} (bound 1e-5); bf16 path {e16:.3e}, bf16-rounded reference {e_var:.3e}, ratio {e16 / e_var:.3f} (bound 1.5)")
    assert e32 <= 1e-5 and e16 <= 1.5 * e_var


def test_tiny_clip_matches_transformers(gpu):
    g = golden()
    names = (("last_hidden_state", "clip.out.last_hidden_state"), ("pooler_output", "clip.out.pooler_output"), ("hidden_m2", "clip.out.hidden_m2"))
    var = R.clip_text(R.decode_state(g, "clip.w."), R.CLIP_TINY, g["clip.ids"], R.bf)
    var["hidden_m2"] = var["hidden_states"][-2]
    for dt in (F32, BF):
        out = build_models(gpu, dt)[1](g["clip.ids"], output_hidden_states=True)
        assert len(out.hidden_states) == R.CLIP_TINY["num_hidden_layers"] + 1
        got = dict(last_hidden_state=out.last_hidden_state, pooler_output=out.pooler_output, hidden_m2=out.hidden_states[-2])
        for name, key in names:
            truth = g[key].double()
            e, e_var = rel_l2(got[name].cpu(), truth), rel_l2(var[name], truth)
            print(f"TEXT tiny CLIP {name} {dt}: {e:.3e}; bf16-rounded reference {e_var:.3e}, ratio {e / e_var:.3f}")
            assert e <= (1e-5 if dt == F32 else 1.5 * e_var), (name, dt, e, e_var)


def test_t5_layer_at_real_width(gpu):
    """One T5-XXL block (d_model 4096, 64 heads of 64, d_ff 10240, L = 512): the packed QKV / FF GEMMs and the 64-head bias launch at their real
    shapes, checked on 24 query rows (first, last, tile edges, random) against float64 with fp32 key / value projections."""
    from unigen_amd.text import T5EncoderModel
    cfg = dict(R.T5_TINY, d_model=4096, num_heads=64, d_ff=10240, num_layers=1, vocab_size=8)
    m = T5EncoderModel.from_config(cfg, device=gpu, dtype=BF)
    g = torch.Generator(device=gpu).manual_seed(5)
    for name, t in m.state_dict().items():
        if "relative_attention_bias" in name:
            t.copy_(torch.randn(t.shape, generator=g, device=gpu) * 2)
        elif t.dim() == 2:
            t.copy_(torch.randn(t.shape, generator=g, device=gpu) * (0.7 / math.sqrt(t.shape[1])))
        else:
            t.copy_(1 + 0.1 * torch.randn(t.shape, generator=g, device=gpu))
    x = torch.randn(512, 4096, generator=g, device=gpu).to(BF)
    got = m.layer(x, 0, 1, 512, m.rel_table(512))
    torch.cuda.synchronize()
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    rows = torch.tensor(sorted({0, 1, 63, 64, 127, 128, 255, 256, 383, 384, 510, 511} | set(torch.randint(0, 512, (12,), generator=torch.Generator().manual_seed(1)).tolist())))
    table = R.t5_rel_table(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], 512)
    x64 = x.cpu().double()[None]
    truth = R.t5_layer_rows(sd, cfg, 0, x64, table, rows, None, F32)
    e_var = rel_l2(R.t5_layer_rows(sd, cfg, 0, x64, table, rows, R.bf, F32), truth)
    e = rel_l2(got.cpu()[rows], truth)
    print(f"TEXT T5-XXL layer: bf16 path {e:.3e}, bf16-rounded reference {e_var:.3e}, ratio {e / e_var:.3f} (bound 1.5)")
    assert e <= 1.5 * e_var


# ---- encode_prompt and the pipeline ----------------------------------------------------------------------------------------------------
def test_encode_prompt_on_ids(gpu):
    from src.text_encoder import encode_prompt
    g = golden()
    t5, clip = build_models(gpu, BF)
    clip_ids = g["clip.ids"]
    t5_ids = torch.cat([g["t5.ids"], g["t5.ids"].flip(1)], 0)
    embeds, pooled, text_ids = encode_prompt([clip, t5], [None, None], None, 200, device=gpu, num_images_per_prompt=2, text_input_ids_list=[clip_ids, t5_ids])
    assert tuple(embeds.shape) == (4, 200, 128) and tuple(pooled.shape) == (4, 128) and embeds.dtype == BF and pooled.dtype == BF
    assert tuple(text_ids.shape) == (200, 3) and text_ids.dtype == BF and not text_ids.any()
    e1, p1, _ = encode_prompt([clip, t5], [None, None], None, 200, device=gpu, text_input_ids_list=[clip_ids, t5_ids])
    assert torch.equal(embeds, e1[[0, 0, 1, 1]]) and torch.equal(pooled, p1[[0, 1, 0, 1]])      # the reference's two repeat orders
    only = encode_prompt([clip], [None], None, 200, device=gpu, text_input_ids_list=[clip_ids])
    assert torch.equal(only, p1)
    with pytest.raises(ValueError, match="text_input_ids"):
        encode_prompt([clip], [None], "a prompt", 200, device=gpu)


def test_pipeline_denoises_with_attached_encoders(gpu):
    """One denoise step of the tiny FLUX model with the native encoders attached and no `encode_prompt` callable."""
    from unigen_amd.flux import UniGenFlux
    from unigen_amd.pipeline import UniGenFLUXPipeline
    g = golden()
    t5, clip = build_models(gpu, BF)
    cfg = dict(num_layers=2, num_single_layers=4, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=128, pooled_projection_dim=128)
    model = UniGenFlux.from_config(cfg, device=gpu, dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["canny"],
                               control_params=dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True, single_control_dev=2))
    model.init_synthetic_(seed=1, std=0.05, bias_std=0.02)
    pipe = UniGenFLUXPipeline(transformer=model, text_encoder=clip, text_encoder_2=t5)
    ids = (g["clip.ids"][:1], g["t5.ids"])
    control = torch.randn(1, 64, 64, generator=torch.Generator().manual_seed(2)).to(device=gpu, dtype=BF)
    kw = dict(control_image=control, height=128, width=128, num_inference_steps=1, guidance_scale=3.5, output_type="latent", max_sequence_length=200,
              latents=torch.randn(1, 64, 64, generator=torch.Generator().manual_seed(3)), return_dict=False)
    torch.manual_seed(0)                                       # the CoMoE's random token selection draws from the device generator
    out = pipe(prompt=ids, condition_prompt=ids, **kw)[0]
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 64, 64) and torch.isfinite(out.float()).all()
    # the same call on the embeds the encoders give: the hook adds nothing of its own
    pe, pp, _ = __import__("unigen_amd.text", fromlist=["x"]).encode_prompt([clip, t5], [None, None], None, 200, device=gpu, text_input_ids_list=list(ids))
    torch.manual_seed(0)
    ref = pipe(prompt_embeds=pe, pooled_prompt_embeds=pp, condition_pooled_prompt_embeds=pp, **kw)[0]
    assert torch.equal(out, ref)
    pipe.text_encoder_2 = None
    with pytest.raises(NotImplementedError, match="encode_prompt"):
        pipe(prompt=ids, condition_prompt=ids, **kw)
