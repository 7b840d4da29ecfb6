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
ATTN_SLIPS = {            # slip -> the modes in which a kernel could commit it
    "bias_len_lkv": ("bias", "bias_causal"), "bias_len_lq": ("bias", "bias_causal"), "bias_sign": ("bias", "bias_causal"),
    "head_table_0": ("bias", "bias_causal"), "causal_off_by_one": ("causal", "bias_causal"),
    "causal_limit_lq": ("bias", "causal", "bias_causal"), "ragged_key_dup": ("bias", "causal", "bias_causal")}


def attention(q, k, v, scale: float, table=None, causal: bool = False, rnd=None, slip=None):
    """q [B, Lq, H, dh], k / v [B, Lkv, H, dh] -> [B, Lq, H, dh], float64. rnd: the probabilities exp(s - max) are rounded as the P.V operand
    (the row sum is of the unrounded ones) and the output is rounded.

    `slip` makes the reference commit one mistake that the kernel's index arithmetic could (tests/test_text_ref_cpu.py shows that the sweep's
    bounds catch each; a slipped table index is clamped into the table, as a kernel's LDS read would stay inside its allocation):
      bias_len_lkv / bias_len_lq   the table is centred with Lkv - 1 / Lq - 1 in place of rel_len - 1
      bias_sign                    the table is indexed by q - k
      head_table_0                 every head reads head 0's slice
      causal_off_by_one            the mask hides key >= q (the diagonal too; row 0 is emptied and comes out NaN)
      causal_limit_lq              the key loop ends at Lq: keys at or beyond Lq are dropped, in every mode (under the mask they are hidden anyway)
      ragged_key_dup               the padded slots of the ragged last 64-key tile are not masked: each counts the last key again, at its own position"""
    assert slip is None or slip in ATTN_SLIPS, slip
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    Lq, Lkv = q.shape[1], k.shape[1]
    if slip == "ragged_key_dup" and Lkv % 64:
        pad = 64 - Lkv % 64
        k, v = (torch.cat([t, t[:, -1:].expand(-1, pad, -1, -1)], 1) for t in (k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    kpos, qpos = torch.arange(s.shape[-1])[None, :], torch.arange(Lq)[:, None]
    if table is not None:
        tb = table.to(F64)
        rel_len = (tb.shape[1] + 1) // 2
        centre = {"bias_len_lkv": Lkv - 1, "bias_len_lq": Lq - 1}.get(slip, rel_len - 1)
        idx = ((qpos - kpos) if slip == "bias_sign" else (kpos - qpos)) + centre
        if slip is None:
            assert int(idx.min()) >= 0 and int(idx.max()) < tb.shape[1]
        if slip == "head_table_0":
            tb = tb[:1].expand_as(tb)
        s = s + tb[:, idx.clamp(0, tb.shape[1] - 1)][None]
    if causal:
        s = s.masked_fill((kpos >= qpos) if slip == "causal_off_by_one" else (kpos > qpos), float("-inf"))
    if slip == "causal_limit_lq":
        s = s.masked_fill((kpos >= Lq).expand(Lq, -1), float("-inf"))
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


# ==================================================================================================================================
# Sweep of the kernels (tests/test_fuzz_text_gpu.py): shared bounds, case builders and layouts. GPU-free; tests/test_text_ref_cpu.py shows that
# the attention cases tell a slipped kernel from a right one and that the data regimes do what they claim.
# ==================================================================================================================================
FP32_TERM = 2.0 ** -20           # of the magnitudes that enter an element-wise kernel in fp32 (docs/PARITY_TOLERANCES.md, "Text encoders")
TINY = 2.0 ** -126


def half_ulp(v):
    """half a bf16 ulp at the magnitude of v (taken a hair above it: an fp32 evaluation may sit on the other side of a power of two)"""
    return bf16_ulp(v.abs() * (1 + 2.0 ** -18)) / 2


def worst_row(got, ref):
    g, r = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return float(((g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-30)).max())


def _rel_l2(got, ref):
    g, r = got.double().flatten(), ref.double().flatten()
    return float((g - r).norm() / r.norm().clamp_min(1e-30))


# ---- per-element truths and bounds of the element-wise kernels (the rules of tests/test_text_gpu.py, stated once) ------------------------------
def rmsnorm_bound(x, w, eps: float, bf16: bool):
    """-> (float64 truth, per-element bound): 2^-20 of the value, and for bf16 the module's two roundings: half an ulp of the output plus half an ulp
    of the inner bf16(x rs) carried through w"""
    x, w = x.to(F64), w.to(F64)
    u = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    truth = w * u
    return truth, FP32_TERM * truth.abs() + ((half_ulp(truth) + w.abs() * half_ulp(u)) if bf16 else 0) + TINY


def layernorm_bound(x, w, b, eps: float, bf16: bool):
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    truth = layernorm(x, w, b, eps)
    mu = x.mean(-1, keepdim=True)
    rs = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return truth, FP32_TERM * ((x.abs() + mu.abs()) * rs * w.abs() + b.abs()) + (half_ulp(truth) if bf16 else 0) + TINY


def gated_gelu_bound(ab, bf16: bool):
    ab = ab.to(F64)
    F = ab.shape[-1] // 2
    a, b = ab[..., :F], ab[..., F:]
    gl = gelu_new(a)
    truth = gl * b
    return truth, FP32_TERM * (a.abs() * b.abs()) + ((half_ulp(truth) + b.abs() * half_ulp(gl)) if bf16 else 0) + TINY


def quick_gelu_bound(x, bf16: bool):
    x = x.to(F64)
    truth = quick_gelu(x)
    return truth, FP32_TERM * x.abs() + (bf16_ulp(truth) if bf16 else 0) + TINY


def elementwise_excess(got, truth, bound, bf16: bool) -> float:
    """worst |got - truth| / bound. Where the float64 value lies beyond the largest finite number of the storage type the product overflows in the
    module as well (fp32 arithmetic, IEEE rounding to the type): there the infinity of the right sign is the correct answer, and anything else
    is held to the bound as everywhere."""
    got, fmax = got.to(F64), float(torch.finfo(BF if bf16 else F32).max)
    err = (got - truth).abs() / bound
    over = (truth.abs() > fmax) & torch.isinf(got) & (torch.sign(got) == torch.sign(truth))
    err = torch.where(over, torch.zeros_like(err), err)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return float(err.max()) if err.numel() else 0.0


# ---- attention: judging one result ----------------------------------------------------------------------------------------------------
def attn_parts(Lq: int):
    """the full 128-query workgroups and the last partial one are bounded separately"""
    full = Lq // 128 * 128
    return ([("full", slice(0, full))] if full else []) + ([("tail", slice(full, Lq))] if Lq % 128 else [])


def attn_judge(got, truth, variant, bf16: bool):
    """-> (worst error / bound, lines). bf16: rel-L2 and the worst query row <= max(1.5 x the rounding-point variant's own, 2^-9); the fp32 twin:
    rel-L2 <= 1e-5, every row <= 1e-4. A NaN anywhere is an infinite ratio."""
    worst, lines = 0.0, []
    for name, sl in attn_parts(truth.shape[1]):
        g, t, va = got[:, sl], truth[:, sl], variant[:, sl]
        e, ew = _rel_l2(g, t), worst_row(g, t)
        b, bw = (max(1.5 * _rel_l2(va, t), 2.0 ** -9), max(1.5 * worst_row(va, t), 2.0 ** -9)) if bf16 else (1e-5, 1e-4)
        ratio = max(e / b, ew / bw)
        worst = max(worst, ratio if ratio == ratio else float("inf"))
        lines.append(f"{name}: rel_l2 {e:.3e} (bound {b:.3e}) worst row {ew:.3e} (bound {bw:.3e})")
    return worst, lines


# ---- attention: cases -----------------------------------------------------------------------------------------------------------------
import functools
import random

ATTN_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 200, 257, 333, 520)
ATTN_MODES = {"bias": (True, False), "causal": (False, True), "bias_causal": (True, True)}
ATTN_REGIMES = ("gaussian", "rising", "falling", "spike_tail", "far_bias")
ATTN_COMBOS = [(m, r) for r in ATTN_REGIMES for m in ATTN_MODES if not (r == "far_bias" and m == "causal")]     # far_bias needs a table
N_ATTN_SWEEP = 3 * len(ATTN_COMBOS)                   # every (mode, regime) pair three times
ATTN_CAP = 2_000_000                                  # B H Lq Lkv: truth and variant of one case stay well under a second on the host
ATTN_HEADS = (1, 3, 5, 3, 12, 5, 1)
SENT_O = -768.0                                       # exact in bf16; no attention output of these cases comes near it
GUARD = 64                                            # sentinel elements before and after every output buffer
REGIME_STEP = 4.0                                     # rising / falling: what a chosen row's score gains per 64-key tile
REGIME_SPIKE = 36.0                                   # spike_tail: what the dominant key's score gains in a chosen row


def _eligible(regime: str):
    """rising / falling need three full key tiles (and, under the mask, rows that see them), spike_tail a partial last tile"""
    if regime in ("rising", "falling"):
        return tuple(n for n in ATTN_LENGTHS if n > 192), tuple(n for n in ATTN_LENGTHS if n > 192)
    if regime == "spike_tail":
        return ATTN_LENGTHS, tuple(n for n in ATTN_LENGTHS if n % 64)
    return ATTN_LENGTHS, ATTN_LENGTHS


def _layout(rng, shared: bool):
    """column pads (elements; q / k / v multiples of 8, o a multiple of 4), spare rows per batch, and o's start 8 bytes past a 16-byte boundary"""
    lay = {n: dict(colpad=8 * rng.choice([0, 1, 2, 3, 8]), spare=rng.randint(0, 5)) for n in "qkv"}
    lay["o"] = dict(colpad=4 * rng.choice([0, 1, 2, 3, 5]), spare=rng.randint(0, 5), off=rng.choice([0, 4]))
    lay["shared"] = shared
    return lay


def attn_sweep_spec(i: int) -> dict:
    """the shape, mode, regime and layout of sweep case i (no data): cheap enough for a parametrize list"""
    rng = random.Random(9100 + i)
    mode, regime = ATTN_COMBOS[i % len(ATTN_COMBOS)]
    lq_set, lkv_set = _eligible(regime)
    B, H = rng.choice([1, 2, 3]), ATTN_HEADS[i % len(ATTN_HEADS)]
    Lq, Lkv = rng.choice(lq_set), rng.choice(lkv_set)
    causal = ATTN_MODES[mode][1]
    if regime == "far_bias" and Lq > Lkv:
        Lq, Lkv = Lkv, Lq                             # every query keeps keys near its diagonal: no row is emptied
    if regime == "spike_tail" and causal and Lq < Lkv:
        Lq = Lkv                                      # under the mask some rows must see the last key tile
    if B * H * Lq * Lkv > ATTN_CAP:
        B = 1
    while B * H * Lq * Lkv > ATTN_CAP:                # only 12 heads at the longest lengths
        Lq = max(n for n in lq_set if n < Lq)
    rel_len = max(Lq, Lkv) + (0, 1, 37)[(i // 3 + i) % 3]
    shared = rng.random() < 0.5
    return dict(id=f"{i:02d}-{mode}-{regime}-B{B}H{H}-{Lq}x{Lkv}-r{rel_len}-{'packed' if shared else 'split'}", i=i, B=B, H=H, Lq=Lq, Lkv=Lkv,
                rel_len=rel_len, mode=mode, bias=ATTN_MODES[mode][0], causal=causal, regime=regime, scale=1.0 if ATTN_MODES[mode][0] else 64 ** -0.5,
                layout=_layout(rng, shared))


def _attn_table(g, H, Lq, Lkv, rel_len, regime):
    """fp32 [H, 2 rel_len - 1]: entries within +-8; the entries no correct launch reads (k - q outside [-(Lq - 1), Lkv - 1]) hold distinct values
    above 32, which would dominate every row that read one"""
    n = 2 * rel_len - 1
    table = (torch.randn(H, n, generator=g, dtype=F64) * (1.0 if regime in ("rising", "falling") else 2.0)).clamp(-8, 8)
    rel = torch.arange(n) - (rel_len - 1)
    if regime == "far_bias":
        far = rel.abs() > 16
        table[:, far] = -60.0 + 0.25 * torch.randn(H, int(far.sum()), generator=g, dtype=F64)
    unread = (rel < -(Lq - 1)) | (rel > Lkv - 1)
    table[:, unread] = (32.0 + (torch.arange(n) % 97).to(F64) * 0.5)[unread][None] * (1 + 0.01 * torch.arange(H).to(F64))[:, None]
    return table.to(F32)


def attn_data(c: dict) -> dict:
    """c (a spec) with its data: bf16-representable float64 q [B, Lq, H, 64], k / v [B, Lkv, H, 64], the fp32 table (or None), and what the regime
    chose: `rows` (query rows it acts on), `spike_key`."""
    B, H, Lq, Lkv, regime, scale = c["B"], c["H"], c["Lq"], c["Lkv"], c["regime"], c["scale"]
    g = torch.Generator().manual_seed(77000 + c.get("i", 0) * 31 + Lq * 7 + Lkv)
    plain = regime in ("gaussian", "far_bias")
    q = torch.randn(B, Lq, H, 64, generator=g, dtype=F64) * (0.5 if plain else 0.125)    # quiet scores where a regime has to stand out of them
    k, v = (torch.randn(B, Lkv, H, 64, generator=g, dtype=F64) for _ in range(2))
    u = torch.randn(64, generator=g, dtype=F64)
    u = u / u.norm()
    rows, spike_key = torch.arange(0), None
    tile = torch.arange(Lkv) // 64
    if regime in ("rising", "falling"):
        rows = torch.arange(0, Lq, 2)                                                     # the fixed half: even rows
        q[:, rows] += 0.5 * u                                                             # small: it also multiplies k's own component along u
        step = REGIME_STEP / (0.5 * scale)
        mult = (tile + 1) if regime == "rising" else (int(tile.max()) + 1 - tile)
        k += (step * mult.to(F64))[None, :, None, None] * u
    elif regime == "spike_tail":
        start = Lkv // 64 * 64
        spike_key = start + int(torch.randint(0, Lkv - start, (1,), generator=g))
        if c["causal"]:
            spike_key = start                                                             # more rows see it
        rows = torch.arange(0, Lq, 4)                                                     # one row in four (row 0 among them: Lq = 1 has one)
        if c["causal"]:
            rows = rows[rows >= spike_key]
        q[:, rows] += 3.0 * u
        k[:, spike_key] += (REGIME_SPIKE / (3.0 * scale)) * u
    q, k, v = bf(q), bf(k), bf(v)
    table = _attn_table(g, H, Lq, Lkv, c["rel_len"], regime) if c["bias"] else None
    return dict(c, q=q, k=k, v=v, table=table, rows=rows, spike_key=spike_key)


@functools.lru_cache(maxsize=None)
def attn_sweep_case(i: int) -> dict:
    return attn_data(attn_sweep_spec(i))


def _fixed(name, B, H, Lq, Lkv, rel_len, mode, i):
    rng = random.Random(9900 + i)
    bias, causal = ATTN_MODES[mode]
    return dict(id=name, i=100 + i, B=B, H=H, Lq=Lq, Lkv=Lkv, rel_len=rel_len, mode=mode, bias=bias, causal=causal, regime="gaussian",
                scale=1.0 if bias else 64 ** -0.5, layout=_layout(rng, False))


ATTN_FIXED = {s["id"]: s for s in (
    _fixed("rel4096", 1, 3, 64, 64, 4096, "bias", 0),            # the largest LDS request: 18 KiB of tiles + 32 KiB of table; table [3, 8191]
    _fixed("q1_kv520", 2, 3, 1, 520, 520, "bias", 1),
    _fixed("q520_kv1", 2, 3, 520, 1, 520, "bias", 2),
    _fixed("causal_129x33", 2, 3, 129, 33, 129, "causal", 3),
    _fixed("causal_33x257", 2, 3, 33, 257, 257, "causal", 4))}


@functools.lru_cache(maxsize=None)
def attn_fixed_case(name: str) -> dict:
    return attn_data(ATTN_FIXED[name])


@functools.lru_cache(maxsize=None)
def _attn_refs_cached(key):
    c = attn_fixed_case(key) if isinstance(key, str) else attn_sweep_case(key)
    args = (c["q"], c["k"], c["v"], c["scale"], c["table"], c["causal"])
    return attention(*args), attention(*args, rnd=bf)


def attn_refs(c: dict):
    """(float64 truth, rounding-point variant) of a sweep or fixed case, computed once"""
    return _attn_refs_cached(c["id"] if c["id"] in ATTN_FIXED else c["i"])


# ---- attention: layouts ---------------------------------------------------------------------------------------------------------------
def attn_buffers(c: dict, dt):
    """CPU buffers of case c in storage type dt, laid out as c['layout'] says. -> {name: dict(buf, off, rs, bs, rows, width)} for q, k, v, o;
    the operand starts at element `off` of the flat `buf`, row stride rs, batch stride bs. q / k / v: everything outside the operand (pad columns,
    spare rows, the other operands' rows beyond its own length in a packed buffer) is NaN - in bounds, so a kernel that reads a row past Lq or
    Lkv and multiplies it by a zero probability produces NaN. o: sentinels everywhere, GUARD of them before and after. With layout['shared']
    q | k | v sit side by side in one buffer's rows, as text.py's packed projection does."""
    B, H, lay = c["B"], c["H"], c["layout"]
    W = H * 64
    L = dict(q=c["Lq"], k=c["Lkv"], v=c["Lkv"], o=c["Lq"])
    out = {}
    if lay["shared"]:
        rows = max(c["Lq"], c["Lkv"]) + lay["q"]["spare"]
        rs = 3 * W + lay["q"]["colpad"]
        buf = torch.full((B, rows, rs), float("nan"), dtype=dt)
        for j, n in enumerate("qkv"):
            buf[:, :L[n], j * W:(j + 1) * W] = c[n].reshape(B, L[n], W).to(dt)
            out[n] = dict(buf=buf.view(-1), off=j * W, rs=rs, bs=rows * rs, rows=L[n], width=W)
    else:
        for n in "qkv":
            rows, rs = L[n] + lay[n]["spare"], W + lay[n]["colpad"]
            buf = torch.full((B, rows, rs), float("nan"), dtype=dt)
            buf[:, :L[n], :W] = c[n].reshape(B, L[n], W).to(dt)
            out[n] = dict(buf=buf.view(-1), off=0, rs=rs, bs=rows * rs, rows=L[n], width=W)
    rows, rs = L["o"] + lay["o"]["spare"], W + lay["o"]["colpad"]
    out["o"] = dict(buf=torch.full((GUARD + lay["o"]["off"] + B * rows * rs + GUARD,), SENT_O, dtype=dt), off=GUARD + lay["o"]["off"], rs=rs, bs=rows * rs,
                    rows=L["o"], width=W)
    return out


def attn_read_output(c: dict, o: dict, buf: torch.Tensor):
    """-> (the [B, Lq, H, 64] result, whether every element outside it still holds the sentinel) from the flat output buffer after the launch"""
    B = c["B"]
    buf = buf.cpu()
    region = torch.as_strided(buf, (B, o["rows"], o["width"]), (o["bs"], o["rs"], 1), o["off"])
    got = region.clone().view(B, o["rows"], c["H"], 64)
    rest = buf.clone()
    torch.as_strided(rest, (B, o["rows"], o["width"]), (o["bs"], o["rs"], 1), o["off"]).fill_(SENT_O)
    return got, bool((rest == SENT_O).all())


# ---- norm and activation cases --------------------------------------------------------------------------------------------------------
NORM_D = (8, 512, 520, 4096, 4600, 4608, 4616, 8192, 10240)     # 4608 = 64 lanes x 9 chunks x 8: the last register-resident width; 4616 the first beyond
NORM_ROWS = (1, 2, 3, 5, 77)
NORM_PADS = (0, 8, 72)
NORM_KINDS = ("mag1", "mag1e-3", "mag1e3", "constant", "zero", "big_mean")


def norm_sweep_cases():
    """every D with every row count; the nine (ldx - D, ldo - D) pairs in turn; the row kinds rotate with the case so that one-row cases meet each"""
    cases = []
    for a, D in enumerate(NORM_D):
        for b, rows in enumerate(NORM_ROWS):
            n = a * len(NORM_ROWS) + b
            px, po = NORM_PADS[n % 3], NORM_PADS[n // 3 % 3]
            cases.append(dict(id=f"D{D}-rows{rows}-ldx+{px}-ldo+{po}-k{n % 6}", n=n, D=D, rows=rows, ldx=D + px, ldo=D + po))
    return cases


def norm_row_kinds(c: dict):
    return [NORM_KINDS[(r + c["n"]) % 6] for r in range(c["rows"])]


def norm_data(c: dict):
    """bf16-representable float64 x [rows, D], w, b. Row kinds: magnitude 1 / 1e-3 / 1e3; a constant row and an all-zero row (float64 variance exactly
    0: LayerNorm's truth is b); a row whose mean is about 1000 times its spread (bf16 values of one binade: most equal the mean, one in twenty
    sits an ulp away)."""
    rows, D = c["rows"], c["D"]
    g = torch.Generator().manual_seed(4200 + c["n"])
    x = torch.randn(rows, D, generator=g, dtype=F64)
    for r, kind in enumerate(norm_row_kinds(c)):
        if kind == "mag1e-3":
            x[r] *= 1e-3
        elif kind == "mag1e3":
            x[r] *= 1e3
        elif kind == "constant":
            x[r] = (-3.0, 1.5, 0.4375)[r % 3]
        elif kind == "zero":
            x[r] = 0.0
        elif kind == "big_mean":
            x[r] = (60.0, -1000.0)[r % 2] * (1 + 1e-3 * x[r])
    w, b = 1 + 0.2 * torch.randn(D, generator=g, dtype=F64), 0.2 * torch.randn(D, generator=g, dtype=F64)
    return bf(x), bf(w), bf(b)


ACT_M, ACT_F, ACT_PADS = (1, 5, 77), (8, 1000, 10240), (0, 8, 64)


def act_sweep_cases():
    """gated GELU: every (M, F) twice, the nine (ld - 2F, ldo - F) pairs in turn"""
    cases = []
    for n in range(18):
        M, F = ACT_M[n % 3], ACT_F[n // 3 % 3]
        pi, po = ACT_PADS[n % 3 if n < 9 else (n + 1) % 3], ACT_PADS[(n // 3 + n // 9) % 3]
        cases.append(dict(id=f"M{M}-F{F}-ld+{pi}-ldo+{po}", n=n, M=M, F=F, ld=2 * F + pi, ldo=F + po))
    return cases


def act_data(c: dict):
    """bf16-representable float64 ab [M, 2F]: Gaussian (a three times wider than b) with the tails sprinkled in: |x| >= 10, signed zeros, subnormals"""
    M, F = c["M"], c["F"]
    g = torch.Generator().manual_seed(5200 + c["n"])
    ab = torch.cat([torch.randn(M, F, generator=g, dtype=F64) * 3, torch.randn(M, F, generator=g, dtype=F64)], -1)
    special = torch.tensor([10.0, -10.0, 12.5, -40.0, 0.0, -0.0, 2.0 ** -130, -2.0 ** -133, 300.0, -1e4], dtype=F64)
    pick = torch.rand(M, 2 * F, generator=g) < 0.15
    vals = special[torch.randint(0, len(special), (M, 2 * F), generator=g)]
    return bf(torch.where(pick, vals, ab))


def all_finite_bf16():
    """every finite bf16 value, by bit pattern: 65 280 of them, float64"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(BF).to(F64)
    x = x[torch.isfinite(x)]
    assert x.numel() == 65280
    return x


GATE_B = (1.0, -3.0, 1.9921875)             # the last: 0x3fff, a bf16 with every mantissa bit set
