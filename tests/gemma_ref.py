"""float64 references of the Gemma-2 kernels and model (unigen_amd/csrc/text.hip, unigen_amd/gemma.py), restated from the published semantics of
transformers' Gemma2Model (modeling_gemma2.py: Gemma2RMSNorm, Gemma2RotaryEmbedding, apply_rotary_pos_emb, eager_attention_forward under the
causal / sliding-window masks and a right-padded attention_mask, Gemma2TextScaledWordEmbedding, Gemma2DecoderLayer).
tests/test_gemma_ref_cpu.py pins them against the installed transformers and against tests/golden/gemma_tiny.safetensors.

Every function takes `rnd`: None evaluates in exact float64; `bf` rounds where the bf16 product path rounds (every projection, RoPE's two
products and its sum, the norm's single output, the residual sums, the gated GELU's two, the probabilities as the P.V operand, the attention
output, the cos / sin table and the embedding multiplier) - the "rounding-point variant" / "bf16-rounded run" that the GPU tests measure the
kernels' error against.

A query row without a single live key (every row of a sample whose kv_len is 0; with a window the padded rows from kv_len + window - 1 on) is ZERO
here and in the kernel; the module's additive mask spreads such a row evenly over all keys, and in float64 (its softmax casts the mask to fp32, where
it is -inf) turns it into NaN. tests/golden/gemma_tiny.safetensors has no such row; tests/golden/gemma_tiny_window.safetensors (TINY_WINDOW) has 24,
which are compared apart (window_dead_rows)."""
import zlib

import torch

from tests.text_ref import BF, F32, F64, _r, bf, bf16_ulp, gated_gelu, linear  # noqa: F401

NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")
_TINY = dict(vocab_size=128, hidden_size=128, num_hidden_layers=4, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=256,
             rms_norm_eps=1e-6, query_pre_attn_scalar=256, hidden_activation="gelu_pytorch_tanh", rope_theta=10000.0, max_position_embeddings=64,
             layer_types=["sliding_attention", "full_attention", "sliding_attention", "full_attention"])
TINY_A = dict(_TINY, attn_logit_softcapping=50.0, sliding_window=4096)
TINY_B = dict(_TINY, attn_logit_softcapping=4.0, sliding_window=8)
# standard deviations of the fixture's weights: config A uniform; config B makes the cap and the window visible in the output
STD_A = dict(qk=0.08, linear=0.08, norm=0.1, embed=0.08)
STD_B = dict(qk=0.2, linear=0.08, norm=0.3, embed=0.08)
TINY_B_, TINY_L, TINY_LIVE = 2, 24, 17          # batch, tokens, live tokens of the second sample


# ---- kernels ---------------------------------------------------------------------------------------------------------------------
def live_keys(L: int, window: int = 0, kv_len=None, B: int = 1, qrows=None) -> torch.Tensor:
    """bool [B, n, L] (query, key): k <= q, and k > q - window with a window, and k < kv_len[b] with key lengths; the queries are all L rows, or `qrows`"""
    qpos, kpos = (torch.arange(L) if qrows is None else torch.as_tensor(qrows))[:, None], torch.arange(L)[None, :]
    live = kpos <= qpos
    if window:
        live = live & (kpos > qpos - window)
    live = live[None].expand(B, qpos.shape[0], L)
    if kv_len is not None:
        live = live & (kpos[None] < torch.as_tensor(kv_len).view(B, 1, 1))
    return live


MUTANTS = ("window+1", "window-1", "kvlen+1", "group_mod", "no_rescale", "tile_skip_early", "cap_as_clamp")
MUTANT_TILE = 32            # the key tile of the kernel the mutants imitate (attn_plain_kernel at head width 256)


def _mutant_live(mutant, L: int, window: int, kv_len, B: int) -> torch.Tensor:
    """live_keys as a kernel with one off-by-one mistake would see them (all L query rows)"""
    qpos, kpos = torch.arange(L)[:, None], torch.arange(L)[None, :]
    live = kpos <= qpos
    if window:
        w = window + 1 if mutant == "window+1" else window - 1 if mutant == "window-1" else window
        live = live & (kpos > qpos - w)                                 # window - 1 = 0 hides every key: unlike live_keys, where 0 means no window
        if mutant == "tile_skip_early":                                 # the tile whose LAST key is the window's first is taken for one behind the window
            first = qpos - window + 1
            live = live & ~((first >= 0) & (first % MUTANT_TILE == MUTANT_TILE - 1) & (kpos // MUTANT_TILE == first // MUTANT_TILE))
    live = live[None].expand(B, L, L)
    if kv_len is not None:
        n = torch.as_tensor(kv_len).view(B, 1, 1)
        live = live & (kpos[None] < (torch.clamp(n + 1, max=L) if mutant == "kvlen+1" else n))
    return live


def _no_rescale(s, v):
    """online softmax over tiles of MUTANT_TILE keys in which the accumulator and the sum are NOT scaled when the running maximum moves.
    s [B, H, L, L] with -inf at hidden keys, v [B, L, H, dh] -> (numerator [B, L, H, dh], sum [B, L, H, 1])"""
    B, H, L, _ = s.shape
    m = torch.full((B, H, L, 1), float("-inf"), dtype=s.dtype)
    den, acc = torch.zeros(B, H, L, 1, dtype=s.dtype), torch.zeros(B, L, H, v.shape[-1], dtype=s.dtype)
    for k0 in range(0, L, MUTANT_TILE):
        st = s[..., k0:k0 + MUTANT_TILE]
        m = torch.maximum(m, st.amax(-1, keepdim=True))
        p = torch.exp(st - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        den = den + p.sum(-1, keepdim=True)
        acc = acc + torch.einsum("bhqk,bkhd->bqhd", p, v[:, k0:k0 + MUTANT_TILE])
    return acc, den.permute(0, 2, 1, 3)


def attention(q, k, v, scale: float, softcap: float = 0.0, window: int = 0, kv_len=None, rnd=None, dtype=F64, qrows=None, mutant=None):
    """q [B, L, H, dh], k / v [B, L, KV, dh] -> [B, L, H, dh]: query head h reads K/V head h // (H // KV). rnd: the probabilities exp(s - max) are
    rounded as the P.V operand (the row sum is of the unrounded ones) and the output is rounded. dtype: float64, or float32 for the host evaluation
    of the same formula that bounds the fp32 twin's tanh. qrows: q holds only these rows [B, n, H, dh] of the sequence.
    mutant (one of MUTANTS; exact float64 on all rows only): the same attention with one mistake a kernel could make, for
    tests/test_gemma_attn_cases_cpu.py to show that the case grid of tests/gemma_attn_cases.py would see it."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    B, L, H = q.shape[0], k.shape[1], q.shape[2]
    g = H // k.shape[2]
    if mutant is not None:
        assert mutant in MUTANTS and dtype == F64 and rnd is None and qrows is None, mutant
    if mutant == "group_mod":
        idx = torch.arange(H) % k.shape[2]
        k, v = k[:, :, idx], v[:, :, idx]
    else:
        k, v = k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if softcap:
        s = s.clamp(-softcap, softcap) if mutant == "cap_as_clamp" else torch.tanh(s / softcap) * softcap
    live = (live_keys(L, window, kv_len, B, qrows) if mutant is None else _mutant_live(mutant, L, window, kv_len, B))[:, None]
    s = s.masked_fill(~live, float("-inf"))
    if mutant == "no_rescale":
        num, den = _no_rescale(s, v)
        return num / torch.where(den > 0, den, torch.ones_like(den))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
    den = p.sum(-1).permute(0, 2, 1)[..., None]
    o = torch.einsum("bhqk,bkhd->bqhd", _r(rnd, p), v) / torch.where(den > 0, den, torch.ones_like(den))
    return _r(rnd, o)


def rope_table(L: int, dh: int, theta: float = 10000.0):
    """(cos, sin) fp32 [L, dh / 2]: Gemma2RotaryEmbedding.forward before its cast (fp32 inverse frequencies times fp32 positions)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float) / dh))
    freqs = torch.arange(L, dtype=torch.float)[:, None] * inv_freq[None, :]
    return freqs.cos(), freqs.sin()


def rope(x, cos, sin, rnd=None):
    """x [B, L, heads, dh], cos / sin [L, dh / 2] -> x cos + rotate_half(x) sin; rnd: each product, then the sum"""
    x, c, s = x.to(F64), cos.to(F64)[None, :, None, :], sin.to(F64)[None, :, None, :]
    half = x.shape[-1] // 2
    lo, hi = x[..., :half], x[..., half:]
    return torch.cat([_r(rnd, _r(rnd, lo * c) - _r(rnd, hi * s)), _r(rnd, _r(rnd, hi * c) + _r(rnd, lo * s))], -1)


def rmsnorm(x, w, eps: float, residual=None, rnd=None):
    """(residual +) rnd(x rsqrt(mean(x^2) + eps) (1 + w)); with a residual the sum is rounded again"""
    x = x.to(F64)
    y = _r(rnd, x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (1.0 + w.to(F64)))
    return y if residual is None else _r(rnd, residual.to(F64) + y)


def embed(weight, ids, scale: float, rnd=None):
    return _r(rnd, weight.to(F64)[ids.long()] * scale)


# ---- layer and model -------------------------------------------------------------------------------------------------------------
def layer_types(cfg):
    lt = cfg.get("layer_types")
    return lt if lt is not None else ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(cfg["num_hidden_layers"])]


def layer(sd, cfg, i: int, x, cos, sin, kv_len=None, rnd=None):
    B, L, _ = x.shape
    H, KV, dh, eps = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["rms_norm_eps"]
    p = f"layers.{i}."
    h = rmsnorm(x, sd[p + "input_layernorm.weight"], eps, None, rnd)
    q = rope(linear(h, sd[p + "self_attn.q_proj.weight"], None, rnd).view(B, L, H, dh), cos, sin, rnd)
    k = rope(linear(h, sd[p + "self_attn.k_proj.weight"], None, rnd).view(B, L, KV, dh), cos, sin, rnd)
    v = linear(h, sd[p + "self_attn.v_proj.weight"], None, rnd).view(B, L, KV, dh)
    window = cfg["sliding_window"] if layer_types(cfg)[i] == "sliding_attention" and cfg.get("sliding_window") else 0
    a = attention(q, k, v, cfg["query_pre_attn_scalar"] ** -0.5, cfg.get("attn_logit_softcapping") or 0.0, window, kv_len, rnd).reshape(B, L, H * dh)
    x = rmsnorm(linear(a, sd[p + "self_attn.o_proj.weight"], None, rnd), sd[p + "post_attention_layernorm.weight"], eps, x, rnd)
    h = rmsnorm(x, sd[p + "pre_feedforward_layernorm.weight"], eps, None, rnd)
    ab = torch.cat([linear(h, sd[p + "mlp.gate_proj.weight"], None, rnd), linear(h, sd[p + "mlp.up_proj.weight"], None, rnd)], -1)
    f = linear(gated_gelu(ab, rnd), sd[p + "mlp.down_proj.weight"], None, rnd)
    return rmsnorm(f, sd[p + "post_feedforward_layernorm.weight"], eps, x, rnd)


def layer_rows(sd, cfg, i: int, x, cos, sin, rows, kv_len=None, rnd=None, kv_dtype=F64):
    """the rows `rows` (one index for every sample) of layer(): keys and values of all rows (their projections in kv_dtype), everything else on the chosen
    rows alone, so that a layer at the real width stays a few seconds of float64"""
    B, L, _ = x.shape
    H, KV, dh, eps = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["rms_norm_eps"]
    p = f"layers.{i}."
    h = rmsnorm(x, sd[p + "input_layernorm.weight"], eps, None, rnd)
    kvp = lambda n: _r(rnd, (h.to(kv_dtype) @ sd[p + f"self_attn.{n}_proj.weight"].to(kv_dtype).t()).to(F64)).view(B, L, KV, dh)
    k, v = rope(kvp("k"), cos, sin, rnd), kvp("v")
    x, h = x[:, rows], h[:, rows]
    q = rope(linear(h, sd[p + "self_attn.q_proj.weight"], None, rnd).view(B, len(rows), H, dh), cos[rows], sin[rows], rnd)
    window = cfg["sliding_window"] if layer_types(cfg)[i] == "sliding_attention" and cfg.get("sliding_window") else 0
    a = attention(q, k, v, cfg["query_pre_attn_scalar"] ** -0.5, cfg.get("attn_logit_softcapping") or 0.0, window, kv_len, rnd, qrows=rows)
    x = rmsnorm(linear(a.reshape(B, len(rows), H * dh), sd[p + "self_attn.o_proj.weight"], None, rnd), sd[p + "post_attention_layernorm.weight"], eps, x, rnd)
    h = rmsnorm(x, sd[p + "pre_feedforward_layernorm.weight"], eps, None, rnd)
    ab = torch.cat([linear(h, sd[p + "mlp.gate_proj.weight"], None, rnd), linear(h, sd[p + "mlp.up_proj.weight"], None, rnd)], -1)
    f = linear(gated_gelu(ab, rnd), sd[p + "mlp.down_proj.weight"], None, rnd)
    return rmsnorm(f, sd[p + "post_feedforward_layernorm.weight"], eps, x, rnd)


def model(sd, cfg, ids, attention_mask=None, rnd=None):
    """-> last_hidden_state [B, L, hidden] float64. attention_mask: None or a prefix mask [B, L]. The embedding multiplier is sqrt(hidden) rounded to
    fp32 (the module's buffer) and the cos / sin table is the fp32 one; rnd rounds both once more, as a bf16 model's casts do."""
    B, L = ids.shape
    kv_len = None if attention_mask is None else attention_mask.sum(1)
    scale = _r(rnd, torch.tensor(cfg["hidden_size"] ** 0.5, dtype=F32).to(F64))
    x = embed(sd["embed_tokens.weight"], ids, scale, rnd)
    cos, sin = (_r(rnd, t.to(F64)) for t in rope_table(L, cfg["head_dim"], cfg.get("rope_theta", 10000.0)))
    for i in range(cfg["num_hidden_layers"]):
        x = layer(sd, cfg, i, x, cos, sin, kv_len, rnd)
    return rmsnorm(x, sd["norm.weight"], cfg["rms_norm_eps"], None, rnd)


# ---- the tiny models of the fixture ----------------------------------------------------------------------------------------------
def keys(cfg):
    D, F, dh = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    H, KV = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    out = {"embed_tokens.weight": (cfg["vocab_size"], D), "norm.weight": (D,)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"layers.{i}."
        out.update({p + "self_attn.q_proj.weight": (H * dh, D), p + "self_attn.k_proj.weight": (KV * dh, D), p + "self_attn.v_proj.weight": (KV * dh, D),
                    p + "self_attn.o_proj.weight": (D, H * dh), p + "mlp.gate_proj.weight": (F, D), p + "mlp.up_proj.weight": (F, D),
                    p + "mlp.down_proj.weight": (D, F)})
        out.update({p + n + ".weight": (D,) for n in NORMS})
    return out


def _hash_normal(n: int, seed: int) -> torch.Tensor:
    """n integers in [-126, 126], bell-shaped with standard deviation 36.9 (four 6-bit fields of a 32-bit integer hash of the index, summed): exact
    integer arithmetic, so the same on every platform and library version. The two tiny models (2.4 M weights) do not fit a committed fixture; the
    fixture pins them through the outputs it records."""
    M = 0xFFFFFFFF
    x = (torch.arange(n, dtype=torch.int64) + seed * 0x9E3779B1) & M
    x = (x * 2654435761) & M
    x = x ^ (x >> 15)
    x = (x * 2246822519) & M
    x = x ^ (x >> 13)
    x = (x * 3266489917) & M
    x = x ^ (x >> 16)
    return (x & 63) + ((x >> 6) & 63) + ((x >> 12) & 63) + ((x >> 18) & 63) - 126


def tiny_state(cfg, std, seed: int):
    """{name: fp32 tensor of bf16-representable values}: q / k projections at std['qk'], the other matrices at std['linear'], the embedding at
    std['embed'], norm weights (the norm multiplies by 1 + w) at std['norm']"""
    out = {}
    for name, shape in keys(cfg).items():
        n = 1
        for d in shape:
            n *= d
        sd_ = std["norm"] if len(shape) == 1 else std["embed"] if "embed" in name else std["qk"] if ("q_proj" in name or "k_proj" in name) else std["linear"]
        ints = _hash_normal(n, seed * 1000003 + zlib.crc32(name.encode())).to(F64)
        out[name] = (ints * (sd_ / 36.9)).view(shape).to(F32).to(BF).to(F32)
    return out


def tiny_inputs():
    """ids int64 [2, 24] and the prefix mask [2, 24] whose second row has 17 ones"""
    ids = (_hash_normal(TINY_B_ * TINY_L, 12345) + 126).view(TINY_B_, TINY_L) % 128
    mask = torch.ones(TINY_B_, TINY_L, dtype=torch.int64)
    mask[1, TINY_LIVE:] = 0
    return ids, mask


TINY = {"a": (TINY_A, STD_A, 1), "b": (TINY_B, STD_B, 2)}

# A sliding layer whose window is more than a 32-key tile and shorter than the prompt (tests/golden/gemma_tiny_window.safetensors): 100 tokens, the
# second sample with 37 live ones, the weights at config B's standard deviations so that the window shows in the output.
TINY_C = dict(_TINY, attn_logit_softcapping=50.0, sliding_window=40, max_position_embeddings=128)
TINY_WINDOW = (TINY_C, STD_B, 4)
WINDOW_B, WINDOW_L, WINDOW_LIVE = 2, 100, 37


def window_inputs():
    """ids int64 [2, 100] and the prefix mask [2, 100] whose second row has 37 ones"""
    ids = (_hash_normal(WINDOW_B * WINDOW_L, 54321) + 126).view(WINDOW_B, WINDOW_L) % 128
    mask = torch.ones(WINDOW_B, WINDOW_L, dtype=torch.int64)
    mask[1, WINDOW_LIVE:] = 0
    return ids, mask


def window_dead_rows(cfg, mask):
    """bool [B, L]: the rows that have no live key in a sliding layer (padded rows `sliding_window` or more behind the last live key). gemma_ref and
    the kernel define their attention output as zero, the module's additive mask spreads them evenly over all keys: the stated departure of the
    header, so these rows are compared apart."""
    L = mask.shape[1]
    return ~live_keys(L, cfg["sliding_window"], mask.sum(1), mask.shape[0]).any(-1)


def rel_l2(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm())


def hf_model(cfg, sd):
    """the installed transformers' Gemma2Model in float64 with eager attention on these weights (CPU tests and the fixture's generator only)"""
    import transformers
    c = {k: v for k, v in cfg.items() if k != "rope_theta"}
    conf = transformers.Gemma2Config(**c, rope_parameters={"rope_type": "default", "rope_theta": cfg.get("rope_theta", 10000.0)}, attention_dropout=0.0,
                                     pad_token_id=0, bos_token_id=2, eos_token_id=1, use_cache=False, attn_implementation="eager")
    m = transformers.Gemma2Model(conf).eval()
    m.load_state_dict(sd, strict=True)
    return m.double()
