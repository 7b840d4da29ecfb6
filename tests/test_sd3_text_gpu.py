"""GPU tests of SD3's prompt encoding (unigen_amd/csrc/text.hip: ug_gelu_erf; unigen_amd/text.py: CLIPTextModelWithProjection, encode_prompt_sd3,
encode_condition_prompt_sd3; UniGenSD3Pipeline with the native encoders attached) against the float64 references of tests/sd3_text_ref.py, which
tests/test_sd3_text_cpu.py pins against transformers.

Bounds (docs/PARITY_TOLERANCES.md, "Text encoders"):
  ug_gelu_erf   per element |err| <= 2^-20 |x| + 2^-126, plus one bf16 ulp of the float64 value for the bf16 entry (ug_quick_gelu's form)
  models        fp32 path against the fixture's transformers outputs: rel-L2 <= 1e-5; bf16 path against the same truth: <= 1.5 x the error of a
                bf16-rounded run of the restatement on the same weights
  assembly      encode_prompt_sd3 is plumbing: every block bit-identical to the models called directly
"""
import functools
import math
import os

import pytest
import torch

from tests import sd3_text_ref as S
from tests import text_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLIP_OUTPUTS = ("text_embeds", "last_hidden_state", "hidden_m2", "hidden_m3")


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------------
def _gelu_input(case):
    if case == "all_bf16":                                   # every finite bf16 value, padded to a multiple of 8
        x = R.all_finite_bf16()
        return torch.cat([x, torch.zeros(-x.numel() % 8, dtype=F64)])
    return R.bf((torch.randn(case, generator=torch.Generator().manual_seed(case)) * 4).double())


@pytest.mark.parametrize("case", (8, 8000, 8 * 1001, "all_bf16"))
def test_gelu_erf(gpu, case):
    from unigen_amd import ops
    x = _gelu_input(case)
    assert x.numel() % 8 == 0
    for dt in (BF, F32):
        truth, bound = S.gelu_erf_bound(x, dt == BF)
        xd = x.to(device=gpu, dtype=dt)
        got = ops.gelu_erf(xd)
        assert got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu().double(), x)               # out of place: the input is left alone
        alias = xd.clone()
        assert ops.gelu_erf(alias, alias) is alias and torch.equal(alias, got)                       # y aliasing x: the same values
        excess = R.elementwise_excess(got.cpu(), truth, bound, dt == BF)
        print(f"SD3TEXT gelu_erf {case} {dt}: worst |err| / bound = {excess:.3f}")
        assert excess <= 1.0


# ---- the tiny models against the fixture --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return {**load_file(os.path.join(GOLDEN_DIR, "sd3_text_tiny.safetensors")), **load_file(os.path.join(GOLDEN_DIR, "sd3_text_tiny_t5.safetensors"))}


CLIPS = {"clip_a": S.CLIP_A, "clip_b": S.CLIP_B}


def build_clip(gpu, name, dt):
    from unigen_amd.text import CLIPTextModelWithProjection
    m = CLIPTextModelWithProjection.from_config(CLIPS[name], device=gpu, dtype=dt)
    m.load_state_dict(R.decode_state(golden(), f"{name}.w."))
    return m


def build_t5(gpu, dt):
    from unigen_amd.text import T5EncoderModel
    m = T5EncoderModel.from_config(S.T5_SD3, device=gpu, dtype=dt)
    m.load_state_dict(R.decode_state(golden(), "t5.w."))
    return m


@functools.lru_cache(maxsize=None)
def rounded_reference(name):
    """the bf16-rounded run of the restatement, once per model"""
    g = golden()
    var = S.clip_text_proj(R.decode_state(g, f"{name}.w."), CLIPS[name], g[f"{name}.ids"], R.bf)
    return dict(text_embeds=var["text_embeds"], last_hidden_state=var["last_hidden_state"], hidden_m2=var["hidden_states"][-2], hidden_m3=var["hidden_states"][-3])


@pytest.mark.parametrize("name", list(CLIPS))
def test_tiny_projected_clip_matches_transformers(gpu, name):
    g, cfg = golden(), CLIPS[name]
    var = rounded_reference(name)
    for dt in (F32, BF):
        out = build_clip(gpu, name, dt)(g[f"{name}.ids"], output_hidden_states=True)
        assert len(out.hidden_states) == cfg["num_hidden_layers"] + 1 and out[0] is out.text_embeds and out[1] is out.last_hidden_state
        assert out.text_embeds.dtype == dt and tuple(out.text_embeds.shape) == (2, cfg["projection_dim"])
        got = dict(text_embeds=out.text_embeds, last_hidden_state=out.last_hidden_state, hidden_m2=out.hidden_states[-2], hidden_m3=out.hidden_states[-3])
        for key in CLIP_OUTPUTS:
            truth = g[f"{name}.out.{key}"].double()
            e, e_var = rel_l2(got[key].cpu(), truth), rel_l2(var[key], truth)
            print(f"SD3TEXT tiny {name} {key} {dt}: {e:.3e}; bf16-rounded reference {e_var:.3e}, ratio {e / e_var:.3f}")
            assert e <= (S.FP32_PATH if dt == F32 else S.BF16_RATIO * e_var), (name, key, dt, e, e_var)
    plain = build_clip(gpu, name, BF)(g[f"{name}.ids"])
    assert plain.hidden_states is None and torch.equal(plain[0], got["text_embeds"]) and torch.equal(plain[1], got["last_hidden_state"])


def test_bigg_layer_at_real_width(gpu):
    """One OpenCLIP bigG layer (hidden 1280, 20 heads of 64, MLP 5120, erf GELU) on 2 x 77 rows: the 20-head causal launch and the 1280 / 3840 / 5120
    GEMM shapes at their real sizes, every row against float64."""
    from unigen_amd.text import CLIPTextModelWithProjection
    cfg = dict(S.CLIP_B, hidden_size=1280, num_attention_heads=20, intermediate_size=5120, num_hidden_layers=1, vocab_size=8, projection_dim=8)
    m = CLIPTextModelWithProjection.from_config(cfg, device=gpu, dtype=BF)
    g = torch.Generator(device=gpu).manual_seed(5)
    for name, t in m.state_dict().items():
        if t.dim() == 2:
            t.copy_(torch.randn(t.shape, generator=g, device=gpu) * (0.7 / math.sqrt(t.shape[1])))
        elif name.endswith("weight"):                            # the norms
            t.copy_(1 + 0.1 * torch.randn(t.shape, generator=g, device=gpu))
        else:
            t.copy_(0.1 * torch.randn(t.shape, generator=g, device=gpu))
    x = torch.randn(2 * 77, 1280, generator=g, device=gpu).to(BF)
    got = m.layer(x, 0, 2, 77)
    torch.cuda.synchronize()
    sd = {k[len("text_model."):]: v.float().cpu() for k, v in m.state_dict().items() if k.startswith("text_model.")}
    x64 = x.cpu().double().view(2, 77, 1280)
    truth = S.clip_layer(sd, cfg, 0, x64)
    variant = S.clip_layer(sd, cfg, 0, x64, R.bf)
    e, e_var = rel_l2(got.cpu(), truth), rel_l2(variant, truth)
    w, w_var = R.worst_row(got.cpu(), truth.view(154, 1280)), R.worst_row(variant, truth)
    print(f"SD3TEXT bigG layer: bf16 path {e:.3e}, bf16-rounded reference {e_var:.3e}, ratio {e / e_var:.3f}; worst row {w:.3e} against {w_var:.3e}, "
          f"ratio {w / w_var:.3f} (bound {S.BF16_RATIO})")
    assert e <= S.BF16_RATIO * e_var and w <= S.BF16_RATIO * w_var


# ---- the encode functions on ids ----------------------------------------------------------------------------------------------------------------------
def _fixture_ids():
    g = golden()
    return [g["clip_a.ids"], g["clip_b.ids"], g["t5.ids"]]


def test_encode_prompt_sd3_on_ids(gpu):
    from unigen_amd.text import encode_condition_prompt_sd3, encode_prompt_sd3
    enc = [build_clip(gpu, "clip_a", BF), build_clip(gpu, "clip_b", BF), build_t5(gpu, BF)]
    ids = _fixture_ids()
    neg = S.negative_ids(ids)
    e, ne, p, npool = encode_prompt_sd3(enc, [None] * 3, None, num_images_per_prompt=2, max_sequence_length=S.T5_LEN, device=gpu, text_input_ids_list=ids,
                                        negative_text_input_ids_list=neg)
    L3 = S.T5_LEN
    assert tuple(e.shape) == tuple(ne.shape) == (4, 77 + L3, 256) and tuple(p.shape) == tuple(npool.shape) == (4, 48 + 96) and e.dtype == BF and p.dtype == BF
    seq_rows, pool_rows = [0, 0, 1, 1], [0, 1, 0, 1]
    for got, pooled, src in ((e, p, ids), (ne, npool, neg)):
        a, b = enc[0](src[0], output_hidden_states=True), enc[1](src[1], output_hidden_states=True)
        assert torch.equal(got[:, :77, :64], a.hidden_states[-2][seq_rows]) and torch.equal(got[:, :77, 64:192], b.hidden_states[-2][seq_rows])
        assert not got[:, :77, 192:].any()                                                          # the zero pad up to the T5 width
        assert torch.equal(got[:, 77:], enc[2](src[2])[0][seq_rows])
        assert torch.equal(pooled, torch.cat([a.text_embeds, b.text_embeds], -1)[pool_rows])
    assert not torch.equal(e, ne) and not torch.equal(p, npool)
    # clip_skip: one layer earlier for the prompt, not for the negatives; the condition prompt: the same assembly without negatives
    a, b = enc[0](ids[0], output_hidden_states=True), enc[1](ids[1], output_hidden_states=True)
    e1, ne1, p1, np1 = encode_prompt_sd3(enc, [None] * 3, None, clip_skip=1, max_sequence_length=L3, device=gpu, text_input_ids_list=ids, negative_text_input_ids_list=neg)
    assert torch.equal(e1[:, :77, :64], a.hidden_states[-3]) and torch.equal(e1[:, :77, 64:192], b.hidden_states[-3]) and torch.equal(e1[:, 77:], e[[0, 2], 77:])
    assert torch.equal(ne1, ne[[0, 2]]) and torch.equal(p1, p[:2]) and torch.equal(np1, npool[:2])
    ce, cp = encode_condition_prompt_sd3(enc, [None] * 3, None, num_images_per_prompt=2, max_sequence_length=L3, device=gpu, text_input_ids_list=ids)
    assert torch.equal(ce, e) and torch.equal(cp, p)
    # without a T5: zeros of the transformer's width
    z, nz, zp, _ = encode_prompt_sd3(enc[:2] + [None], [None] * 3, None, num_images_per_prompt=2, max_sequence_length=10, device=gpu, text_input_ids_list=ids[:2] + [None],
                                     negative_text_input_ids_list=neg[:2] + [None], joint_attention_dim=256)
    assert tuple(z.shape) == (4, 87, 256) and z.device.type == "cuda" and not z[:, 77:].any() and not nz[:, 77:].any()
    assert torch.equal(z[:, :77], e[:, :77]) and torch.equal(nz[:, :77], ne[:, :77]) and torch.equal(zp, p)
    with pytest.raises(ValueError, match="negative_text_input_ids_list"):
        encode_prompt_sd3(enc, [None] * 3, None, device=gpu, text_input_ids_list=ids)


def test_encode_prompt_sd3_matches_the_restatement(gpu):
    """the fp32 twins end to end against the float64 restatement of both functions"""
    from unigen_amd.text import encode_prompt_sd3
    g = golden()
    enc = [build_clip(gpu, "clip_a", F32), build_clip(gpu, "clip_b", F32), build_t5(gpu, F32)]
    ids = _fixture_ids()
    neg = S.negative_ids(ids)
    got = encode_prompt_sd3(enc, [None] * 3, None, num_images_per_prompt=2, clip_skip=1, max_sequence_length=S.T5_LEN, device=gpu, text_input_ids_list=ids,
                            negative_text_input_ids_list=neg)
    clips = [(R.decode_state(g, "clip_a.w."), S.CLIP_A), (R.decode_state(g, "clip_b.w."), S.CLIP_B)]
    want = S.encode_prompt_sd3(clips, (R.decode_state(g, "t5.w."), S.T5_SD3), ids, neg, n=2, clip_skip=1)
    for name, a, b in zip(("prompt_embeds", "negative_prompt_embeds", "pooled", "negative_pooled"), got, want):
        err = rel_l2(a.cpu(), b)
        print(f"SD3TEXT encode_prompt_sd3 fp32 {name}: {err:.3e} (bound {S.FP32_PATH})")
        assert a.shape == b.shape and err <= S.FP32_PATH


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------------------
def test_sd3_pipeline_denoises_from_token_ids(gpu):
    """One denoise step of a tiny UniGenSD3 with the three native encoders attached and no `encode_prompt` callable: from id triples to latents."""
    from unigen_amd.pipeline import UniGenSD3Pipeline
    from unigen_amd.sd3 import UniGenSD3
    from unigen_amd.text import encode_condition_prompt_sd3, encode_prompt_sd3
    enc = [build_clip(gpu, "clip_a", BF), build_clip(gpu, "clip_b", BF), build_t5(gpu, BF)]
    cfg = dict(sample_size=16, num_layers=3, attention_head_dim=64, num_attention_heads=2, joint_attention_dim=256, caption_projection_dim=128,
               pooled_projection_dim=144, pos_embed_max_size=12, dual_attention_layers=(0, 1))
    model = UniGenSD3.from_config(cfg, device=gpu, dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=True))
    model.init_synthetic_(seed=6, std=0.05, bias_std=0.02)
    pipe = UniGenSD3Pipeline(transformer=model, text_encoder=enc[0], text_encoder_2=enc[1], text_encoder_3=enc[2])
    ids = tuple(_fixture_ids())
    neg = tuple(S.negative_ids(ids))
    cond = tuple(i.roll(1, 0).contiguous() for i in ids)                # the other sample's ids: another prompt for the condition
    C = model.config.in_channels
    g = torch.Generator().manual_seed(3)
    kw = dict(control_image=torch.randn(2, C, 16, 16, generator=g).to(device=gpu, dtype=BF), latents=torch.randn(2, C, 16, 16, generator=g),
              num_inference_steps=1, max_sequence_length=S.T5_LEN, output_type="latent", return_dict=False)
    common = dict(max_sequence_length=S.T5_LEN, device=gpu, text_input_ids_list=list(ids))
    cp = encode_condition_prompt_sd3(enc, [None] * 3, None, max_sequence_length=S.T5_LEN, device=gpu, text_input_ids_list=list(cond))[1]
    for gs in (7.0, 1.0):
        torch.manual_seed(0)                                            # the CoMoE's random token selection draws from the device generator
        out = pipe(prompt=ids, condition_prompt=cond, negative_prompt=neg if gs > 1 else None, guidance_scale=gs, **kw)[0]
        torch.cuda.synchronize()
        assert tuple(out.shape) == (2, C, 16, 16) and torch.isfinite(out.float()).all()
        torch.manual_seed(0)
        again = pipe(prompt=ids, condition_prompt=cond, negative_prompt=neg if gs > 1 else None, guidance_scale=gs, **kw)[0]
        assert torch.equal(out, again)                                  # bitwise repeatable
        # the same call on the embeds computed by hand: the pipeline adds nothing of its own
        e, ne, p, npool = encode_prompt_sd3(enc, [None] * 3, None, do_classifier_free_guidance=gs > 1, negative_text_input_ids_list=list(neg) if gs > 1 else None, **common)
        assert tuple(e.shape) == (2, 77 + S.T5_LEN, 256) and tuple(p.shape) == (2, 144)
        torch.manual_seed(0)
        ref = pipe(prompt_embeds=e, negative_prompt_embeds=ne, pooled_prompt_embeds=p, negative_pooled_prompt_embeds=npool, condition_pooled_prompt_embeds=cp,
                   guidance_scale=gs, **kw)[0]
        assert torch.equal(out, ref)
    torch.manual_seed(0)
    assert not torch.equal(out, pipe(prompt=cond, condition_prompt=cond, guidance_scale=1.0, **kw)[0])      # and the prompt does reach the latents
    pipe.text_encoder_2 = None
    with pytest.raises(NotImplementedError, match="encode_prompt"):
        pipe(prompt=ids, condition_prompt=cond, guidance_scale=1.0, **kw)
