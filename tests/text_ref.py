"""float64 references of the text-encoder kernels and models (unigen_amd/csrc/text.hip, unigen_amd/text.py), restated from the published
semantics of T5 (Raffel et al. 2020; transformers' T5EncoderModel) and CLIP's text tower (transformers' CLIPTextModel).
tests/test_text_ref_cpu.py pins them against the installed transformers and against tests/golden/text_tiny.safetensors.

Every function takes `rnd`: None evaluates in exact float64; `bf` rounds where the bf16 product path rounds (every projection, residual sum,
norm and activation output, T5LayerNorm's and the gated GELU's inner rounding, the probabilities as the P.V operand) - the "rounding-point
variant" / "bf16-rounded run" that the GPU tests measure the kernels' error against."""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

T5_TINY = dict(vocab_size=64, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
               relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
CLIP_TINY = dict(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=3, num_attention_heads=2, max_position_embeddings=77,
                 hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=5)
GOLDEN_SCALE = 2.0 ** -10          # matrices of the fixture are int8 times this: exact in bf16, and half the bytes of bf16


def bf(x):
    """round to bf16, keep float64"""
    return x.to(F32).to(BF).to(F64)


def _r(rnd, x):
    return x if rnd is None else rnd(x)


def bf16_ulp(truth64):
    """one bf16 ulp at the magnitude of each value"""
    e = torch.floor(torch.log2(truth64.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 7)


# ---- T5 relative-position bias ---------------------------------------------------------------------------------------------------
def t5_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """Bidirectional bucket of rel = k - q (int64 tensor): the upper half of the buckets for k > q; in each half the distances below
    max_exact = num_buckets / 4 get their own bucket, the rest logarithmic ones up to max_distance, clamped to the last. fp32, truncation."""
    nb = num_buckets // 2
    max_exact = nb // 2
    out = (rel > 0).to(torch.int64) * nb
    n = rel.abs()
    large = max_exact + (torch.log(n.to(F32) / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.int64)
    large = torch.clamp(large, max=nb - 1)
    return out + torch.where(n < max_exact, n, large)


def t5_rel_table(weight: torch.Tensor, L: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """[heads, 2L - 1]: table[h][j] = weight[bucket(j - (L - 1))][h], in weight's values."""
    rel = torch.arange(2 * L - 1, dtype=torch.int64) - (L - 1)
    return weight[t5_bucket(rel, num_buckets, max_distance)].t().contiguous()


def bias_from_table(table: torch.Tensor, Lq: int, Lkv: int) -> torch.Tensor:
    """[heads, Lq, Lkv]: table[h][(k - q) + rel_len - 1]"""
    rel_len = (table.shape[1] + 1) // 2
    idx = torch.arange(Lkv)[None, :] - torch.arange(Lq)[:, None] + rel_len - 1
    return table[:, idx]


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, scale: float, table=None, causal: bool = False, rnd=None):
    """q [B, Lq, H, dh], k / v [B, Lkv, H, dh] -> [B, Lq, H, dh], float64. rnd: the probabilities exp(s - max) are rounded as the P.V operand
    (the row sum is of the unrounded ones) and the output is rounded."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    Lq, Lkv = s.shape[-2:]
    if table is not None:
        s = s + bias_from_table(table.to(F64), Lq, Lkv)[None]
    if causal:
        s = s.masked_fill(torch.arange(Lkv)[None, :] > torch.arange(Lq)[:, None], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = torch.einsum("bhqk,bkhd->bqhd", _r(rnd, p), v) / p.sum(-1).permute(0, 2, 1)[..., None]
    return _r(rnd, o)


# ---- norms and activations -------------------------------------------------------------------------------------------------------
def rmsnorm(x, w, eps: float, rnd=None):
    x, w = x.to(F64), w.to(F64)
    return _r(rnd, w * _r(rnd, x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)))


def layernorm(x, w, b, eps: float = 1e-5, rnd=None):
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return _r(rnd, (x - mu) * torch.rsqrt(var + eps) * w.to(F64) + b.to(F64))


def gelu_new(x):
    """0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) in the equal form that keeps the negative tail"""
    x = x.to(F64)
    return x / (1.0 + torch.exp(-2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gated_gelu(ab, rnd=None):
    F = ab.shape[-1] // 2
    return _r(rnd, _r(rnd, gelu_new(ab[..., :F])) * ab[..., F:].to(F64))


def quick_gelu(x, rnd=None):
    x = x.to(F64)
    return _r(rnd, x / (1.0 + torch.exp(-1.702 * x)))


def linear(x, w, b=None, rnd=None):
    y = x @ w.to(F64).t()
    return _r(rnd, y + b.to(F64) if b is not None else y)


# ---- whole models ----------------------------------------------------------------------------------------------------------------
def t5_layer(sd, cfg, i: int, x, table, rnd=None):
    B, L, D = x.shape
    H, dh, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    p = f"encoder.block.{i}.layer."
    h = rmsnorm(x, sd[p + "0.layer_norm.weight"], eps, rnd)
    q, k, v = (linear(h, sd[p + f"0.SelfAttention.{n}.weight"], None, rnd).view(B, L, H, dh) for n in "qkv")
    a = attention(q, k, v, 1.0, table, False, rnd).reshape(B, L, H * dh)                 # T5 does not scale the scores
    x = _r(rnd, x + linear(a, sd[p + "0.SelfAttention.o.weight"], None, rnd))
    h = rmsnorm(x, sd[p + "1.layer_norm.weight"], eps, rnd)
    ab = torch.cat([linear(h, sd[p + "1.DenseReluDense.wi_0.weight"], None, rnd), linear(h, sd[p + "1.DenseReluDense.wi_1.weight"], None, rnd)], -1)
    return _r(rnd, x + linear(gated_gelu(ab, rnd), sd[p + "1.DenseReluDense.wo.weight"], None, rnd))


def t5_encoder(sd, cfg, ids, rnd=None):
    """-> last_hidden_state [B, L, d_model] float64; no attention mask (padding is attended to, as in the reference's call)."""
    x = sd["shared.weight"].to(F64)[ids.long()]
    table = t5_rel_table(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].to(F64), ids.shape[1],
                         cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"])
    for i in range(cfg["num_layers"]):
        x = t5_layer(sd, cfg, i, x, table, rnd)
    return rmsnorm(x, sd["encoder.final_layer_norm.weight"], cfg["layer_norm_epsilon"], rnd)


def clip_pool_index(ids, eos_token_id: int):
    """legacy configs (eos_token_id == 2): the position of the highest token id; otherwise the first eos_token_id position"""
    return ids.argmax(-1) if eos_token_id == 2 else (ids == eos_token_id).to(torch.int32).argmax(-1)


def clip_text(sd, cfg, ids, rnd=None):
    """-> dict(last_hidden_state, pooler_output, hidden_states: tuple of num_layers + 1 tensors before the final norm), float64.
    Keys without the `text_model.` prefix."""
    B, L = ids.shape
    D, H, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    dh = D // H
    act = {"quick_gelu": quick_gelu, "gelu_new": lambda t, r: _r(r, gelu_new(t)), "gelu_pytorch_tanh": lambda t, r: _r(r, gelu_new(t))}[cfg["hidden_act"]]
    x = _r(rnd, sd["embeddings.token_embedding.weight"].to(F64)[ids.long()] + sd["embeddings.position_embedding.weight"].to(F64)[:L][None])
    hidden = [x]
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        h = layernorm(x, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps, rnd)
        q, k, v = (linear(h, sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"], rnd).view(B, L, H, dh) for n in "qkv")
        a = attention(q, k, v, dh ** -0.5, None, True, rnd).reshape(B, L, D)
        x = _r(rnd, x + linear(a, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], rnd))
        h = layernorm(x, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps, rnd)
        f = act(linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], rnd), rnd)
        x = _r(rnd, x + linear(f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], rnd))
        hidden.append(x)
    last = layernorm(x, sd["final_layer_norm.weight"], sd["final_layer_norm.bias"], eps, rnd)
    pooled = last[torch.arange(B), clip_pool_index(ids, cfg["eos_token_id"])]
    return dict(last_hidden_state=last, pooler_output=pooled, hidden_states=tuple(hidden))


# ---- the tiny models of the fixture ----------------------------------------------------------------------------------------------
def t5_keys(cfg):
    D, inner, F = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"]
    keys = {"shared.weight": (cfg["vocab_size"], D), "encoder.final_layer_norm.weight": (D,),
            "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": (cfg["relative_attention_num_buckets"], cfg["num_heads"])}
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        keys.update({p + "0.layer_norm.weight": (D,), p + "1.layer_norm.weight": (D,), p + "0.SelfAttention.o.weight": (D, inner),
                     p + "1.DenseReluDense.wi_0.weight": (F, D), p + "1.DenseReluDense.wi_1.weight": (F, D), p + "1.DenseReluDense.wo.weight": (D, F)})
        keys.update({p + f"0.SelfAttention.{n}.weight": (inner, D) for n in "qkv"})
    return keys


def clip_keys(cfg):
    D, F = cfg["hidden_size"], cfg["intermediate_size"]
    keys = {"embeddings.token_embedding.weight": (cfg["vocab_size"], D), "embeddings.position_embedding.weight": (cfg["max_position_embeddings"], D),
            "final_layer_norm.weight": (D,), "final_layer_norm.bias": (D,)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2", "self_attn.out_proj"):
            keys[p + n + ".bias"] = (D,)
        keys.update({p + "layer_norm1.weight": (D,), p + "layer_norm2.weight": (D,), p + "self_attn.out_proj.weight": (D, D),
                     p + "mlp.fc1.weight": (F, D), p + "mlp.fc1.bias": (F,), p + "mlp.fc2.weight": (D, F), p + "mlp.fc2.bias": (D,)})
        for n in "qkv":
            keys.update({p + f"self_attn.{n}_proj.weight": (D, D), p + f"self_attn.{n}_proj.bias": (D,)})
    return keys


def random_state(keys, seed: int):
    """Stored form: matrices int8 (value = int8 * GOLDEN_SCALE, standard deviation about 0.1), vectors bf16 (norm weights around 1) and T5's
    relative-attention bias bf16 with standard deviation 2, so that a wrong bias moves the output."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in keys.items():
        if "relative_attention_bias" in name:
            out[name] = (torch.randn(shape, generator=g) * 2.0).to(BF)
        elif len(shape) == 2:
            wide = "embed" in name or name == "shared.weight"
            fan = 1.0 if wide else (128.0 / shape[1]) ** 0.5
            out[name] = torch.clamp(torch.round(torch.randn(shape, generator=g) * (120.0 if wide else 90.0 * fan)), -127, 127).to(torch.int8)
        else:
            t = torch.randn(shape, generator=g) * 0.1
            out[name] = ((1.0 + t) if ("norm" in name and name.endswith("weight")) else t).to(BF)
    return out


def decode_state(stored, prefix: str):
    """stored fixture tensors with `prefix` -> {name: fp32 tensor} (bf16-representable values)"""
    out = {}
    for k, t in stored.items():
        if k.startswith(prefix):
            out[k[len(prefix):]] = t.to(F32) * GOLDEN_SCALE if t.dtype == torch.int8 else t.to(F32)
    return out


def tiny_ids():
    """T5: [1, 200] with padding zeros at the end (attended to); CLIP: [2, 77], EOS (id 5) first at positions 9 and 30, ids above it elsewhere."""
    g = torch.Generator().manual_seed(7)
    t5 = torch.randint(2, 64, (1, 200), generator=g)
    t5[0, 150] = 1
    t5[0, 151:] = 0
    clip = torch.randint(6, 64, (2, 77), generator=g)
    clip[0, 9:] = 5
    clip[1, 30] = 5
    clip[1, 50] = 5
    return t5, clip


def t5_layer_rows(sd, cfg, i: int, x, table, rows, rnd=None, mm=F64):
    """t5_layer for a subset of the query rows of ONE sample (x [1, L, D]) -> [len(rows), D]: what a test at the real width can afford. The key /
    value projections of all rows are the only large products; mm = torch.float32 takes them in fp32 (relative error 1e-6, three orders below bf16's)."""
    H, dh, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    p = f"encoder.block.{i}.layer."
    L = x.shape[1]
    h = rmsnorm(x[0], sd[p + "0.layer_norm.weight"], eps, rnd)
    k, v = (_r(rnd, (h.to(mm) @ sd[p + f"0.SelfAttention.{n}.weight"].to(mm).t()).to(F64)).view(L, H, dh) for n in "kv")
    q = linear(h[rows], sd[p + "0.SelfAttention.q.weight"], None, rnd).view(len(rows), H, dh)
    s = torch.einsum("qhd,khd->hqk", q, k) + bias_from_table(table.to(F64), L, L)[:, rows]
    pr = torch.exp(s - s.amax(-1, keepdim=True))
    a = _r(rnd, torch.einsum("hqk,khd->qhd", _r(rnd, pr), v) / pr.sum(-1).t()[..., None]).reshape(len(rows), H * dh)
    x1 = _r(rnd, x[0, rows].to(F64) + linear(a, sd[p + "0.SelfAttention.o.weight"], None, rnd))
    h = rmsnorm(x1, sd[p + "1.layer_norm.weight"], eps, rnd)
    ab = torch.cat([linear(h, sd[p + "1.DenseReluDense.wi_0.weight"], None, rnd), linear(h, sd[p + "1.DenseReluDense.wi_1.weight"], None, rnd)], -1)
    return _r(rnd, x1 + linear(gated_gelu(ab, rnd), sd[p + "1.DenseReluDense.wo.weight"], None, rnd))
