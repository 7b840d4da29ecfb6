"""float64 references of SD3's prompt encoding (unigen_amd/text.py: CLIPTextModelWithProjection, encode_prompt_sd3, encode_condition_prompt_sd3; the
ug_gelu_erf kernel of unigen_amd/csrc/text.hip), restated from the published semantics of transformers' CLIPTextModelWithProjection and of
diffusers' StableDiffusion3Pipeline.encode_prompt, on top of tests/text_ref.py. tests/test_sd3_text_cpu.py pins the model restatement against the
installed transformers and against tests/golden/sd3_text_tiny*.safetensors; diffusers is not installed, so the assembly is pinned by its written
description alone (docs/PARITY_TOLERANCES.md).

`rnd` is text_ref's: None evaluates in exact float64, `text_ref.bf` rounds where the bf16 product path rounds."""
import math

import torch

from tests import text_ref as R

F64 = torch.float64

# CLIP-A stands for CLIP-L (quick_gelu, first-EOS pooling), CLIP-B for OpenCLIP bigG: the erf GELU, more than one head, and eos_token_id = 2, the legacy
# value bigG's config really carries (pooling at the argmax of the ids). 64 + 128 = 192 CLIP columns against a T5 width of 256: a real zero pad.
CLIP_A = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=1, max_position_embeddings=77,
              hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=5, projection_dim=48)
CLIP_B = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, max_position_embeddings=77,
              hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2, projection_dim=96)
T5_SD3 = dict(R.T5_TINY, d_model=256)
T5_LEN = 24                       # tokens of the fixture's T5 ids (max_sequence_length of the encode tests)

# ---- bounds (docs/PARITY_TOLERANCES.md, "Text encoders") ----------------------------------------------------------------------------------------
FIXTURE_MARGIN = 1e-7             # restatement against the stored transformers outputs: fp32 storage of float64 values (tests/test_text_ref_cpu.py)
HF_MARGIN = 1e-13                 # restatement against transformers in float64, same process
FP32_PATH = 1e-5                  # the fp32 twins against the float64 truth, relative L2
BF16_RATIO = 1.5                  # the bf16 path: at most this times the error of the bf16-rounded restatement on the same weights


def gelu_erf(x, rnd=None):
    """0.5 x (1 + erf(x / sqrt 2)): hidden_act "gelu" (transformers' GELUActivation, torch.nn.functional.gelu)"""
    x = x.to(F64)
    return R._r(rnd, 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0))))


def gelu_erf_bound(x, bf16: bool):
    """-> (float64 truth, per-element bound): the form ug_quick_gelu is held to - 2^-20 of |x|, which enters in fp32, plus one bf16 ulp of the
    truth for the entry that stores bf16."""
    x = x.to(F64)
    truth = gelu_erf(x)
    return truth, R.FP32_TERM * x.abs() + (R.bf16_ulp(truth) if bf16 else 0) + R.TINY


_ACTS = {"quick_gelu": R.quick_gelu, "gelu": gelu_erf, "gelu_new": lambda t, r: R._r(r, R.gelu_new(t)), "gelu_pytorch_tanh": lambda t, r: R._r(r, R.gelu_new(t))}


def clip_layer(sd, cfg, i: int, x, rnd=None):
    """one encoder layer on x [B, L, D] (text_ref.clip_text's, with the erf GELU among the activations)"""
    B, L, D = x.shape
    H, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    dh = D // H
    p = f"encoder.layers.{i}."
    h = R.layernorm(x, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps, rnd)
    q, k, v = (R.linear(h, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"], rnd).view(B, L, H, dh) for n in "qkv")
    a = R.attention(q, k, v, dh ** -0.5, None, True, rnd).reshape(B, L, D)
    x = R._r(rnd, x + R.linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], rnd))
    h = R.layernorm(x, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps, rnd)
    f = _ACTS[cfg["hidden_act"]](R.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], rnd), rnd)
    return R._r(rnd, x + R.linear(f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], rnd))


def clip_text_proj(sd, cfg, ids, rnd=None):
    """-> dict(text_embeds [B, projection_dim], last_hidden_state, hidden_states: num_layers + 1 tensors before the final norm), float64. Keys of sd
    without the `text_model.` prefix, plus `text_projection.weight` [projection_dim, hidden] (no bias)."""
    B, L = ids.shape
    x = R._r(rnd, sd["embeddings.token_embedding.weight"].to(F64)[ids.long()] + sd["embeddings.position_embedding.weight"].to(F64)[:L][None])
    hidden = [x]
    for i in range(cfg["num_hidden_layers"]):
        x = clip_layer(sd, cfg, i, x, rnd)
        hidden.append(x)
    last = R.layernorm(x, sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], cfg["layer_norm_eps"], rnd)
    pooled = last[torch.arange(B), R.clip_pool_index(ids, cfg["eos_token_id"])]
    return dict(text_embeds=R.linear(pooled, sd["text_projection.weight"], None, rnd), last_hidden_state=last, hidden_states=tuple(hidden))


def clip_proj_keys(cfg):
    return {**R.clip_keys(cfg), "text_projection.weight": (cfg["projection_dim"], cfg["hidden_size"])}


# ---- the two encode functions --------------------------------------------------------------------------------------------------------------------
def sd3_embeds(clips, t5, ids, n: int = 1, clip_skip=None, rnd=None, max_sequence_length: int = 256, joint_attention_dim=None):
    """clips = [(state, config), (state, config)], t5 = (state, config) or None, ids = [ids_l, ids_g, ids_t5] -> (prompt_embeds [B n, 77 + L3, width],
    pooled [B n, p_l + p_g]). Per CLIP: hidden_states[-2] (or [-(clip_skip + 2)]) and text_embeds; the sequences repeat with a prompt's copies adjacent,
    the pooled vectors as a block (b0, b1, b0, b1); the CLIP columns are zero-padded on the right to the T5 width and come in front of the T5 rows."""
    seqs, pooled = [], []
    for (sd, cfg), i in zip(clips, ids[:2]):
        out = clip_text_proj(sd, cfg, i, rnd)
        seqs.append(out["hidden_states"][-2 if clip_skip is None else -(clip_skip + 2)].repeat_interleave(n, dim=0))
        pooled.append(out["text_embeds"].repeat(n, 1))
    clip_seq = torch.cat(seqs, -1)
    if t5 is None:
        tail = torch.zeros(clip_seq.shape[0], max_sequence_length, joint_attention_dim, dtype=F64)
    else:
        tail = R.t5_encoder(t5[0], t5[1], ids[2], rnd).repeat_interleave(n, dim=0)
    pad = torch.zeros(*clip_seq.shape[:2], tail.shape[-1] - clip_seq.shape[-1], dtype=F64)
    return torch.cat([torch.cat([clip_seq, pad], -1), tail], 1), torch.cat(pooled, -1)


def encode_prompt_sd3(clips, t5, ids, neg_ids=None, n: int = 1, clip_skip=None, rnd=None, **kw):
    """-> (prompt_embeds, negative_prompt_embeds, pooled, negative_pooled); the negatives (None without neg_ids) never take clip_skip"""
    e, p = sd3_embeds(clips, t5, ids, n, clip_skip, rnd, **kw)
    ne, np_ = sd3_embeds(clips, t5, neg_ids, n, None, rnd, **kw) if neg_ids is not None else (None, None)
    return e, ne, p, np_


def encode_condition_prompt_sd3(clips, t5, ids, n: int = 1, clip_skip=None, rnd=None, **kw):
    return sd3_embeds(clips, t5, ids, n, clip_skip, rnd, **kw)


# ---- the fixture's token ids -----------------------------------------------------------------------------------------------------------------------
def tiny_ids():
    """-> (CLIP-A ids [2, 77]: text_ref's, first EOS (id 5) at 9 and 30; CLIP-B ids [2, 77]: the highest id (63, the EOS of a legacy config) at 12,
    zero padding behind it, and at 40 and again at 60 (the first one counts); T5 ids [2, T5_LEN], the second row padded with zeros)."""
    clip_a = R.tiny_ids()[1]
    g = torch.Generator().manual_seed(21)
    clip_b = torch.randint(3, 63, (2, 77), generator=g)
    clip_b[0, 12] = 63
    clip_b[0, 13:] = 0
    clip_b[1, 40] = 63
    clip_b[1, 60] = 63
    t5 = torch.randint(2, 64, (2, T5_LEN), generator=g)
    t5[1, 15] = 1
    t5[1, 16:] = 0
    return clip_a, clip_b, t5


def negative_ids(ids):
    """other token ids of the same shapes, for the negative prompt: each row reversed (the CLIP pooling positions move with it)"""
    return [i.flip(1).contiguous() for i in ids]
