"""Gemma-2 text encoder on the HIP library: transformers' Gemma2Model (Sana's prompt encoder is gemma-2-2b-it: 26 layers, hidden 2304, 8 query
heads over 4 key/value heads of width 256, feed-forward 9216) on token ids, and `encode_prompt_sana`, diffusers' SanaPipeline.encode_prompt.

Per layer the launches are: norm, q | k | v GEMM (one packed weight), rotate-half RoPE in place on the q and k heads, causal attention with
grouped K/V heads, the logit soft cap, the sliding window of that layer and the key length of each sample (ug_flash_attn_fwd_softcap), o_proj
GEMM, norm + residual, norm, gate | up GEMM (stacked), gated GELU (ug_gated_gelu: gelu_pytorch_tanh is gelu_new), down GEMM, norm + residual
(csrc/text.hip, csrc/gemm.hip). Parameters in fp32 run the same orchestration through the `_f32` verification twins.

The attention mask must be a prefix mask (right padding): it becomes one key length per sample, computed on the device. There is no tokenizer
here: callers pass token ids or attach a tokenizer callable of their own. There is no backward: Sana freezes its text encoder.
diffusers is not installed where this package is tested, so `encode_prompt_sana` is a restatement without a pinned parity test, like the other
diffusers rows (the encoder itself is pinned against transformers: tests/test_gemma_ref_cpu.py, tests/golden/gemma_tiny.safetensors)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops
from .text import BF, F32, TextEncoderOutput, _PackedModel, _read_config_and_weights

_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")


def default_layer_types(num_hidden_layers: int) -> List[str]:
    """Gemma2Config's default: sliding attention on layers 0, 2, ..., full attention on the odd ones."""
    return ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(num_hidden_layers)]


def rope_table(L_: int, dh: int, theta: float, dtype, device=None):
    """(cos, sin) [L, dh / 2] as Gemma2RotaryEmbedding.forward builds them: fp32 inverse frequencies, their fp32 product with the positions, cos /
    sin, then the cast. The module's table is [L, dh] with both halves equal; the kernel reads one half."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float) / dh))
    pos = torch.arange(L_)[None, :].float()
    freqs = (inv_freq[None, :, None].float() @ pos[:, None, :]).transpose(1, 2)[0]
    return freqs.cos().to(dtype=dtype, device=device).contiguous(), freqs.sin().to(dtype=dtype, device=device).contiguous()


def prefix_lengths(attention_mask: torch.Tensor, B: int, L_: int) -> torch.Tensor:
    """attention_mask [B, L] of ones-then-zeros rows -> int32 [B] live keys per sample, on the mask's device (one host read for the check)."""
    if attention_mask.dim() != 2 or tuple(attention_mask.shape) != (B, L_):
        raise ValueError(f"attention_mask: expected [batch, length] = [{B}, {L_}], got {tuple(attention_mask.shape)}")
    m = attention_mask != 0
    n = m.sum(1)
    prefix = torch.arange(L_, device=m.device)[None, :] < n[:, None]
    binary, ok, live = torch.stack([((attention_mask == 0) | (attention_mask == 1)).all(), (m == prefix).all(), (n > 0).all()]).tolist()
    if not binary:
        raise NotImplementedError("attention_mask with values other than 0 and 1 is not implemented")
    if not ok:
        raise NotImplementedError("attention_mask: every row must be ones then zeros (right padding); left padding and masks with holes are not implemented")
    if not live:
        raise ValueError("attention_mask: a row without a single live token has no softmax")
    return n.to(torch.int32)


class Gemma2Model(_PackedModel):
    """transformers' Gemma2Model on token ids: `model(input_ids, attention_mask=None)[0]` is last_hidden_state [B, L, hidden_size]."""

    KEYS = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim", "intermediate_size", "rms_norm_eps",
            "query_pre_attn_scalar", "attn_logit_softcapping", "sliding_window", "layer_types", "hidden_activation", "attention_bias",
            "use_bidirectional_attention", "rope_parameters", "rope_theta", "rope_scaling")

    def __init__(self, config: dict, device=None, dtype=BF):
        super().__init__(device, dtype)
        c = dict(vocab_size=256000, hidden_size=2304, num_hidden_layers=26, num_attention_heads=8, num_key_value_heads=4, head_dim=256, intermediate_size=9216,
                 rms_norm_eps=1e-6, query_pre_attn_scalar=256, attn_logit_softcapping=50.0, sliding_window=4096, hidden_activation="gelu_pytorch_tanh",
                 attention_bias=False, use_bidirectional_attention=False)       # Gemma2Config's defaults
        c.update({k: config[k] for k in self.KEYS if k in config})
        who = type(self).__name__
        if c["head_dim"] != 256:
            raise NotImplementedError(f"{who}: head_dim = {c['head_dim']}; the soft-cap attention kernel has head width 256")
        if c["hidden_activation"] != "gelu_pytorch_tanh":
            raise NotImplementedError(f"{who}: hidden_activation = {c['hidden_activation']!r}; only 'gelu_pytorch_tanh' is implemented")
        rope = dict(c.get("rope_parameters") or c.get("rope_scaling") or {})
        if rope.get("rope_type", rope.get("type", "default")) != "default":
            raise NotImplementedError(f"{who}: rope_type = {rope.get('rope_type', rope.get('type'))!r}; only the default rotary embedding is implemented")
        if c["attention_bias"]:
            raise NotImplementedError(f"{who}: attention_bias = True is not implemented (the projections carry no bias)")
        if c["use_bidirectional_attention"]:
            raise NotImplementedError(f"{who}: use_bidirectional_attention = True is not implemented (the attention kernel is causal)")
        if c["num_attention_heads"] % c["num_key_value_heads"]:
            raise ValueError(f"{who}: num_attention_heads = {c['num_attention_heads']} is not a multiple of num_key_value_heads = {c['num_key_value_heads']}")
        c["rope_theta"] = float(rope.get("rope_theta", c.get("rope_theta", 10000.0)))
        if c.get("layer_types") is None:
            c["layer_types"] = default_layer_types(c["num_hidden_layers"])
        if len(c["layer_types"]) != c["num_hidden_layers"] or set(c["layer_types"]) - {"sliding_attention", "full_attention"}:
            raise ValueError(f"{who}: layer_types must name 'sliding_attention' or 'full_attention' for each of the {c['num_hidden_layers']} layers")
        self.config = c
        D, F, dh = c["hidden_size"], c["intermediate_size"], c["head_dim"]
        H, KV = c["num_attention_heads"], c["num_key_value_heads"]
        self.embed = self._pack([("embed_tokens.weight", c["vocab_size"])], D)
        self.layers = []
        for i in range(c["num_hidden_layers"]):
            p = f"layers.{i}."
            layer = dict(
                qkv=self._pack([(p + "self_attn.q_proj.weight", H * dh), (p + "self_attn.k_proj.weight", KV * dh), (p + "self_attn.v_proj.weight", KV * dh)], D),
                o=self._pack([(p + "self_attn.o_proj.weight", D)], H * dh),
                gate_up=self._pack([(p + "mlp.gate_proj.weight", F), (p + "mlp.up_proj.weight", F)], D),
                down=self._pack([(p + "mlp.down_proj.weight", D)], F))
            for n in _NORMS:
                layer[n] = self._pack([(p + n + ".weight", D)], None)
            self.layers.append(layer)
        self.final_norm = self._pack([("norm.weight", D)], None)
        self._rope: Dict[int, tuple] = {}

    def _canon(self, key):
        if key.startswith("model."):                    # the causal-LM checkpoint's prefix
            key = key[len("model."):]
        return key if key in self._views else None

    def load_state_dict(self, sd, strict: bool = True):
        return super().load_state_dict({k: v for k, v in sd.items() if k != "lm_head.weight"}, strict)      # tied to embed_tokens.weight

    def init_synthetic_(self, seed: int = 0, std: float = 0.05):
        """Random weights for tests and benchmarks; the norm weights stay around 0 (the norm multiplies by 1 + w)."""
        g = torch.Generator().manual_seed(seed)
        for v in self._views.values():
            v.copy_((torch.randn(v.shape, generator=g, dtype=F32) * std).to(device=self._device, dtype=self._dtype))
        return self

    @classmethod
    def from_config(cls, config: dict, device=None, dtype=BF) -> "Gemma2Model":
        return cls(config, device=device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path, subfolder: Optional[str] = None, device=None, dtype=BF) -> "Gemma2Model":
        cfg, sd = _read_config_and_weights(path, subfolder)
        m = cls(cfg, device=device, dtype=dtype)
        m.load_state_dict(sd)
        return m

    def rope(self, L_: int):
        """The (cos, sin) tables of this length in the model's dtype, built once per length."""
        t = self._rope.get(L_)
        if t is None:
            t = self._rope[L_] = rope_table(L_, self.config["head_dim"], self.config["rope_theta"], self._dtype, self._device)
        return t

    def layer(self, x: torch.Tensor, i: int, B: int, L_: int, rope, kv_len: Optional[torch.Tensor]) -> torch.Tensor:
        """One decoder layer on x [B * L, hidden_size]."""
        c, p = self.config, self.layers[i]
        H, KV, dh, M, eps = c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], B * L_, c["rms_norm_eps"]
        new = lambda n: torch.empty(M, n, dtype=x.dtype, device=x.device)
        W = (H + 2 * KV) * dh
        h = ops.gemma_rmsnorm_rows(x, p["input_layernorm"], eps)
        qkv = ops.gemm(h, p["qkv"], None, new(W), M=M)
        ops.rope_half(qkv, rope[0], rope[1], rows_per_batch=L_, col0=0, nheads=H + KV, dh=dh)
        att = new(H * dh)
        s3 = (W, L_ * W)
        window = c["sliding_window"] if c["layer_types"][i] == "sliding_attention" and c["sliding_window"] else 0
        ops.flash_attn_softcap(qkv, qkv[:, H * dh:], qkv[:, (H + KV) * dh:], att, batches=B, heads=H, kv_heads=KV, dh=dh, L_=L_, q_strides=s3, k_strides=s3,
                               v_strides=s3, o_strides=(H * dh, L_ * H * dh), scale=float(c["query_pre_attn_scalar"]) ** -0.5,
                               softcap=float(c["attn_logit_softcapping"] or 0.0), window=int(window), kv_len=kv_len)
        a = ops.gemm(att, p["o"], None, new(c["hidden_size"]), M=M)
        x = ops.gemma_rmsnorm_rows(a, p["post_attention_layernorm"], eps, residual=x, out=a)
        h = ops.gemma_rmsnorm_rows(x, p["pre_feedforward_layernorm"], eps, out=h)
        ab = ops.gemm(h, p["gate_up"], None, new(2 * c["intermediate_size"]), M=M)
        f = ops.gemm(ops.gated_gelu(ab), p["down"], None, new(c["hidden_size"]), M=M)
        return ops.gemma_rmsnorm_rows(f, p["post_feedforward_layernorm"], eps, residual=x, out=f)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None, position_ids=None, past_key_values=None,
                 inputs_embeds=None, use_cache=None, cache_position=None, **_ignored) -> TextEncoderOutput:
        for name, val in (("position_ids", position_ids), ("past_key_values", past_key_values), ("inputs_embeds", inputs_embeds),
                          ("cache_position", cache_position)):
            if val is not None:
                raise NotImplementedError(f"Gemma2Model: {name} is not implemented (token ids at positions 0 .. L - 1, no cache)")
        if use_cache:
            raise NotImplementedError("Gemma2Model: use_cache is not implemented (an encoder pass keeps no cache)")
        if input_ids is None:
            raise ValueError("Gemma2Model: input_ids is required")
        kv_len = None
        if attention_mask is not None and input_ids.dim() == 2:         # refused before anything runs; the lengths are computed where the model lives
            kv_len = prefix_lengths(attention_mask.to(self._device), *input_ids.shape)
        ids = self._ids(input_ids)
        B, L_ = ids.shape
        c = self.config
        D = c["hidden_size"]
        scale = float(torch.tensor(D ** 0.5).to(self._dtype))          # the module's embed_scale.to(weight.dtype)
        x = ops.gather_rows_scaled(self.embed, ids.view(-1), scale, torch.empty(B * L_, D, dtype=self._dtype, device=self._device))
        rope = self.rope(L_)
        for i in range(len(self.layers)):
            x = self.layer(x, i, B, L_, rope, kv_len)
        x = ops.gemma_rmsnorm_rows(x, self.final_norm, c["rms_norm_eps"])
        return TextEncoderOutput(x.view(B, L_, D))

    forward = __call__


def _select_index(max_sequence_length: int) -> List[int]:
    return [0] + list(range(-max_sequence_length + 1, 0))


def encode_prompt_sana(text_encoder, tokenizer, prompt, max_sequence_length: int = 300, complex_human_instruction: Optional[List[str]] = None,
                       text_input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None, num_images_per_prompt: int = 1,
                       device=None):
    """diffusers' SanaPipeline._get_gemma_prompt_embeds / encode_prompt (the positive prompt) -> (prompt_embeds [B n, max_sequence_length, hidden],
    prompt_attention_mask [B n, max_sequence_length]).

    Prompts are lower-cased and stripped. With `complex_human_instruction` its lines, joined by "\\n", are put in front of every prompt and the
    tokenised length becomes len(tokenizer.encode(instruction)) + max_sequence_length - 2. Padding is "max_length", on the right. Both outputs keep the
    positions [0] + [-max_sequence_length + 1, ..., -1]: the first token and the last max_sequence_length - 1. Without a tokenizer, `text_input_ids` and
    `attention_mask` [B, length] are what the tokenizer would have returned. The results feed SanaTransformer2DModel.forward(encoder_hidden_states=...,
    encoder_attention_mask=...) as they are. Restated from the pipeline's published source; not pinned against diffusers (not installed here)."""
    if tokenizer is not None:
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        prompts = [p.lower().strip() for p in prompts]
        if not complex_human_instruction:
            max_length_all = max_sequence_length
        else:
            chi = "\n".join(complex_human_instruction)
            prompts = [chi + p for p in prompts]
            max_length_all = len(tokenizer.encode(chi)) + max_sequence_length - 2
        enc = tokenizer(prompts, padding="max_length", max_length=max_length_all, truncation=True, add_special_tokens=True, return_tensors="pt")
        text_input_ids, attention_mask = enc.input_ids, enc.attention_mask
    elif text_input_ids is None or attention_mask is None:
        raise ValueError("text_input_ids and attention_mask must be provided when the tokenizer is not specified")
    if text_input_ids.shape[1] < max_sequence_length:
        raise ValueError(f"{text_input_ids.shape[1]} tokens, fewer than max_sequence_length = {max_sequence_length}")
    dev = device if device is not None else text_encoder.device
    mask = attention_mask.to(dev)
    embeds = text_encoder(text_input_ids.to(dev), attention_mask=mask)[0].to(dtype=text_encoder.dtype, device=dev)
    sel = _select_index(max_sequence_length)
    embeds, mask = embeds[:, sel], mask[:, sel]
    B, T, _ = embeds.shape
    n = num_images_per_prompt
    embeds = embeds.repeat(1, n, 1).view(B * n, T, -1)
    mask = mask.repeat(1, n).view(B * n, -1)          # diffusers: view(bs, -1).repeat(n, 1) - the same rows when B = 1; here each prompt's copies stay adjacent
    return embeds, mask
