"""Text encoders on the HIP library: the T5 encoder and the CLIP text model that the reference calls through src/text_encoder.py
(train.py:381-395, :523-569; the top of every pipeline call), and `encode_prompt` itself; for the SD3 pipeline the projected CLIP
(`CLIPTextModelWithProjection`: CLIP-L and OpenCLIP bigG, src/utils.py:16-19) and `encode_prompt_sd3` / `encode_condition_prompt_sd3`
(src/UniGenPipeline.py:34-105, :246-290).

Both classes take token ids and run entirely on libunigen_hip.so: the embedding is ug_gather_rows, every projection ug_gemm_bf16 (q | k | v and
wi_0 | wi_1 packed into one weight each, the residual sums in the GEMM epilogue), attention ug_flash_attn_fwd_bias (T5: relative-position
bias table, no 1/sqrt(dh) scale; CLIP: causal mask), the norms ug_rmsnorm_rows / ug_layernorm_rows, the activations ug_gated_gelu /
ug_quick_gelu / ug_gelu_erf (csrc/text.hip). Parameters in fp32 run the same orchestration through the `_f32` verification twins. No attention mask is applied
(the reference passes none: padding tokens are attended to). There is no tokenizer here: callers pass token ids (the reference's
`text_input_ids` path) or attach a tokenizer callable of their own. There is no backward: the reference freezes both encoders.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import torch

from . import lib as L
from . import ops

BF, F32 = torch.bfloat16, torch.float32


class TextEncoderOutput:
    """`out[0]` / `out.last_hidden_state`, `out.pooler_output`, `out.hidden_states` (transformers' BaseModelOutputWithPooling surface)."""

    def __init__(self, last_hidden_state, pooler_output=None, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states

    def __getitem__(self, i):
        return tuple(t for t in (self.last_hidden_state, self.pooler_output, self.hidden_states) if t is not None)[i]


class CLIPTextModelOutput:
    """`out[0]` / `out.text_embeds`, `out.last_hidden_state`, `out.hidden_states` (transformers' CLIPTextModelOutput surface)."""

    def __init__(self, text_embeds, last_hidden_state, hidden_states=None):
        self.text_embeds, self.last_hidden_state, self.hidden_states = text_embeds, last_hidden_state, hidden_states

    def __getitem__(self, i):
        return tuple(t for t in (self.text_embeds, self.last_hidden_state, self.hidden_states) if t is not None)[i]


def _read_config_and_weights(path: str, subfolder: Optional[str]):
    from .checkpoint import read_control_state_dict
    root = os.path.join(os.fspath(path), subfolder) if subfolder else os.fspath(path)
    if os.path.isdir(root):
        with open(os.path.join(root, "config.json")) as f:
            cfg = json.load(f)
        return cfg, read_control_state_dict(root)
    with open(os.path.join(os.path.dirname(root), "config.json")) as f:      # a single weight file beside its config.json
        cfg = json.load(f)
    return cfg, read_control_state_dict(root)


class _PackedModel:
    """Parameters live in a few packed tensors; every on-disk name is a view of one of them (as the engines do for their fused QKV)."""

    def __init__(self, device, dtype):
        self._views: Dict[str, torch.Tensor] = {}
        self._device, self._dtype = torch.device(device) if device is not None else torch.device("cpu"), dtype
        self._loaded = set()

    dtype = property(lambda self: self._dtype)
    device = property(lambda self: self._device)

    def _new(self, *shape):
        return torch.zeros(*shape, dtype=self._dtype, device=self._device)

    def _pack(self, names_and_rows, cols: Optional[int]):
        """One tensor [sum(rows), cols] (or [sum(rows)] for cols None) whose row blocks are the named parameters."""
        total = sum(r for _, r in names_and_rows)
        pack = self._new(total, cols) if cols is not None else self._new(total)
        r0 = 0
        for name, r in names_and_rows:
            self._views[name] = pack[r0:r0 + r]
            r0 += r
        return pack

    def _canon(self, key: str) -> Optional[str]:
        raise NotImplementedError

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._views)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        seen, unexpected = set(), []
        for key, t in sd.items():
            name = self._canon(key)
            if name is None:
                unexpected.append(key)
                continue
            dst = self._views[name]
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError(f"{key}: shape {tuple(t.shape)} does not match {tuple(dst.shape)}")
            dst.copy_(t.to(device=self._device, dtype=self._dtype))
            seen.add(name)
        missing = sorted(set(self._views) - seen)
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {unexpected[:4]}")
        self._invalidate()
        return missing, unexpected

    def _invalidate(self):
        pass

    def init_synthetic_(self, seed: int = 0, std: float = 0.05):
        """Random weights for tests and benchmarks (norm weights around 1)."""
        g = torch.Generator().manual_seed(seed)
        for name, v in self._views.items():
            t = torch.randn(v.shape, generator=g, dtype=F32) * std
            if "norm" in name and name.endswith("weight"):
                t = 1.0 + t
            v.copy_(t.to(device=self._device, dtype=self._dtype))
        self._invalidate()
        return self

    def _ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int32, torch.int64):
            raise TypeError("input_ids: expected an integer tensor [batch, length]")
        if self._device.type != "cuda":
            raise L.UniGenHipError("text encoders run on the HIP device only (unigen_amd has no CPU path): create the model with device='cuda'")
        return input_ids.to(device=self._device, dtype=torch.int32).contiguous()


class T5EncoderModel(_PackedModel):
    """transformers' T5EncoderModel (gated-GELU feed-forward, T5 v1.1 / XXL) on token ids."""

    KEYS = ("d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets", "relative_attention_max_distance",
            "layer_norm_epsilon", "feed_forward_proj", "vocab_size")

    def __init__(self, config: dict, device=None, dtype=BF):
        super().__init__(device, dtype)
        c = dict(relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
        c.update({k: config[k] for k in self.KEYS if k in config})
        if c["feed_forward_proj"] != "gated-gelu":
            raise NotImplementedError(f"T5EncoderModel: feed_forward_proj = {c['feed_forward_proj']!r}; only 'gated-gelu' (gelu_new gate) is implemented")
        if c["d_kv"] != 64:
            raise NotImplementedError(f"T5EncoderModel: d_kv = {c['d_kv']}; the bias attention kernel has head width 64")
        self.config = c
        D, inner, F = c["d_model"], c["num_heads"] * c["d_kv"], c["d_ff"]
        self.shared = self._pack([("shared.weight", c["vocab_size"])], D)
        self.rel_bias = self._pack([("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", c["relative_attention_num_buckets"])], c["num_heads"])
        self.layers = []
        for i in range(c["num_layers"]):
            p = f"encoder.block.{i}.layer."
            self.layers.append(dict(
                ln0=self._pack([(p + "0.layer_norm.weight", D)], None),
                qkv=self._pack([(p + f"0.SelfAttention.{n}.weight", inner) for n in "qkv"], D),
                o=self._pack([(p + "0.SelfAttention.o.weight", D)], inner),
                ln1=self._pack([(p + "1.layer_norm.weight", D)], None),
                wi=self._pack([(p + "1.DenseReluDense.wi_0.weight", F), (p + "1.DenseReluDense.wi_1.weight", F)], D),
                wo=self._pack([(p + "1.DenseReluDense.wo.weight", D)], F)))
        self.final_ln = self._pack([("encoder.final_layer_norm.weight", D)], None)
        self._tables: Dict[int, torch.Tensor] = {}

    def _canon(self, key):
        if key == "encoder.embed_tokens.weight":       # tied to shared.weight on disk
            return "shared.weight"
        return key if key in self._views else None

    def load_state_dict(self, sd, strict: bool = True):
        if "shared.weight" in sd and "encoder.embed_tokens.weight" in sd:
            sd = {k: v for k, v in sd.items() if k != "encoder.embed_tokens.weight"}
        return super().load_state_dict(sd, strict)

    def _invalidate(self):
        self._tables = {}

    @classmethod
    def from_config(cls, config: dict, device=None, dtype=BF) -> "T5EncoderModel":
        return cls(config, device=device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path, subfolder: Optional[str] = None, device=None, dtype=BF) -> "T5EncoderModel":
        cfg, sd = _read_config_and_weights(path, subfolder)
        m = cls(cfg, device=device, dtype=dtype)
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("decoder.", "lm_head."))})
        return m

    def rel_table(self, Lq: int) -> torch.Tensor:
        """The [heads, 2L - 1] bias table of this length, built once per length (and again after a weight load)."""
        t = self._tables.get(Lq)
        if t is None:
            c = self.config
            t = ops.t5_rel_table(self.rel_bias, Lq, num_buckets=c["relative_attention_num_buckets"], max_distance=c["relative_attention_max_distance"])
            self._tables[Lq] = t
        return t

    def layer(self, x: torch.Tensor, i: int, B: int, Lq: int, table: torch.Tensor) -> torch.Tensor:
        """One encoder block on x [B * Lq, d_model]."""
        c, p = self.config, self.layers[i]
        H, dh, M = c["num_heads"], c["d_kv"], B * Lq
        inner, eps = H * dh, c["layer_norm_epsilon"]
        h = ops.rmsnorm_rows(x, p["ln0"], eps)
        qkv = ops.gemm(h, p["qkv"], None, torch.empty(M, 3 * inner, dtype=x.dtype, device=x.device), M=M)
        att = torch.empty(M, inner, dtype=x.dtype, device=x.device)
        s3 = (3 * inner, Lq * 3 * inner)
        ops.flash_attn_bias(qkv, qkv[:, inner:], qkv[:, 2 * inner:], att, batches=B, heads=H, dh=dh, Lq=Lq, Lkv=Lq, q_strides=s3, k_strides=s3, v_strides=s3,
                            o_strides=(inner, Lq * inner), scale=1.0, rel_table=table)
        x = ops.gemm(att, p["o"], None, torch.empty_like(x), M=M, epilogue=L.EPI_RES_SCALE, residual=x, alpha=1.0)
        h = ops.rmsnorm_rows(x, p["ln1"], eps)
        ab = ops.gemm(h, p["wi"], None, torch.empty(M, 2 * c["d_ff"], dtype=x.dtype, device=x.device), M=M)
        g = ops.gated_gelu(ab)
        return ops.gemm(g, p["wo"], None, torch.empty_like(x), M=M, epilogue=L.EPI_RES_SCALE, residual=x, alpha=1.0)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, **_ignored) -> TextEncoderOutput:
        ids = self._ids(input_ids)
        B, Lq = ids.shape
        D = self.config["d_model"]
        x = ops.gather_rows(self.shared, ids.view(-1), torch.empty(B * Lq, D, dtype=self._dtype, device=self._device))
        table = self.rel_table(Lq)
        for i in range(len(self.layers)):
            x = self.layer(x, i, B, Lq, table)
        x = ops.rmsnorm_rows(x, self.final_ln, self.config["layer_norm_epsilon"])
        return TextEncoderOutput(x.view(B, Lq, D))

    forward = __call__


_CLIP_ACTS = ("quick_gelu", "gelu_pytorch_tanh", "gelu_new")


class CLIPTextModel(_PackedModel):
    """transformers' CLIPTextModel (CLIP-L: quick_gelu) on token ids."""

    KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "hidden_act", "layer_norm_eps",
            "eos_token_id", "vocab_size")
    ACTS = _CLIP_ACTS                                   # the hidden_act values this class takes
    DROPPED = ("vision_model.", "visual_projection.", "text_projection.", "logit_scale")    # checkpoint entries from_pretrained leaves out

    def __init__(self, config: dict, device=None, dtype=BF):
        super().__init__(device, dtype)
        c = dict(hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, max_position_embeddings=77)
        c.update({k: config[k] for k in self.KEYS if k in config})
        if c["hidden_act"] not in self.ACTS:
            raise NotImplementedError(f"{type(self).__name__}: hidden_act = {c['hidden_act']!r} is not implemented (one of {self.ACTS}; erf-GELU, "
                                      "'gelu', is CLIPTextModelWithProjection's)")
        if c["hidden_size"] // c["num_attention_heads"] != 64:
            raise NotImplementedError("CLIPTextModel: the causal attention kernel has head width 64")
        self.config = c
        D, F = c["hidden_size"], c["intermediate_size"]
        self.tok = self._pack([("embeddings.token_embedding.weight", c["vocab_size"])], D)
        self.pos = self._pack([("embeddings.position_embedding.weight", c["max_position_embeddings"])], D)
        self.layers = []
        for i in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            self.layers.append(dict(
                ln1w=self._pack([(p + "layer_norm1.weight", D)], None), ln1b=self._pack([(p + "layer_norm1.bias", D)], None),
                qkv=self._pack([(p + f"self_attn.{n}_proj.weight", D) for n in "qkv"], D),
                qkv_b=self._pack([(p + f"self_attn.{n}_proj.bias", D) for n in "qkv"], None),
                o=self._pack([(p + "self_attn.out_proj.weight", D)], D), o_b=self._pack([(p + "self_attn.out_proj.bias", D)], None),
                ln2w=self._pack([(p + "layer_norm2.weight", D)], None), ln2b=self._pack([(p + "layer_norm2.bias", D)], None),
                fc1=self._pack([(p + "mlp.fc1.weight", F)], D), fc1_b=self._pack([(p + "mlp.fc1.bias", F)], None),
                fc2=self._pack([(p + "mlp.fc2.weight", D)], F), fc2_b=self._pack([(p + "mlp.fc2.bias", D)], None)))
        self.fln_w = self._pack([("final_layer_norm.weight", D)], None)
        self.fln_b = self._pack([("final_layer_norm.bias", D)], None)

    def _canon(self, key):
        if key.startswith("text_model."):
            key = key[len("text_model."):]
        if key == "embeddings.position_ids":            # a buffer of older checkpoints
            return None
        return key if key in self._views else None

    def load_state_dict(self, sd, strict: bool = True):
        return super().load_state_dict({k: v for k, v in sd.items() if not k.endswith("embeddings.position_ids")}, strict)

    def state_dict(self, prefix: str = "text_model.") -> Dict[str, torch.Tensor]:
        return {prefix + k: v for k, v in self._views.items()}

    @classmethod
    def from_config(cls, config: dict, device=None, dtype=BF) -> "CLIPTextModel":
        return cls(config, device=device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path, subfolder: Optional[str] = None, device=None, dtype=BF) -> "CLIPTextModel":
        cfg, sd = _read_config_and_weights(path, subfolder)
        cfg = cfg.get("text_config", cfg) if "hidden_size" not in cfg else cfg
        m = cls(cfg, device=device, dtype=dtype)
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith(cls.DROPPED)})
        return m

    def layer(self, x: torch.Tensor, i: int, B: int, Lq: int) -> torch.Tensor:
        c, p = self.config, self.layers[i]
        D, H, M = c["hidden_size"], c["num_attention_heads"], B * Lq
        new = lambda n: torch.empty(M, n, dtype=x.dtype, device=x.device)
        h = ops.layernorm_rows(x, p["ln1w"], p["ln1b"], c["layer_norm_eps"])
        qkv = ops.gemm(h, p["qkv"], p["qkv_b"], new(3 * D), M=M)
        att = new(D)
        s3 = (3 * D, Lq * 3 * D)
        ops.flash_attn_bias(qkv, qkv[:, D:], qkv[:, 2 * D:], att, batches=B, heads=H, dh=64, Lq=Lq, Lkv=Lq, q_strides=s3, k_strides=s3, v_strides=s3,
                            o_strides=(D, Lq * D), scale=64 ** -0.5, causal=True)
        x = ops.gemm(att, p["o"], p["o_b"], new(D), M=M, epilogue=L.EPI_RES_SCALE, residual=x, alpha=1.0)
        h = ops.layernorm_rows(x, p["ln2w"], p["ln2b"], c["layer_norm_eps"])
        if c["hidden_act"] == "quick_gelu":
            f = ops.gemm(h, p["fc1"], p["fc1_b"], new(c["intermediate_size"]), M=M)
            ops.quick_gelu(f, f)
        elif c["hidden_act"] == "gelu":                 # the erf form (CLIPTextModelWithProjection only): a pass of its own, like quick_gelu
            f = ops.gemm(h, p["fc1"], p["fc1_b"], new(c["intermediate_size"]), M=M)
            ops.gelu_erf(f, f)
        else:                                           # the tanh form: the GEMM's own GELU epilogue
            f = ops.gemm(h, p["fc1"], p["fc1_b"], new(c["intermediate_size"]), M=M, epilogue=L.EPI_BIAS_GELU)
        return ops.gemm(f, p["fc2"], p["fc2_b"], new(D), M=M, epilogue=L.EPI_RES_SCALE, residual=x, alpha=1.0)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, output_hidden_states: bool = False, **_ignored) -> TextEncoderOutput:
        ids = self._ids(input_ids)
        B, Lq = ids.shape
        c = self.config
        D = c["hidden_size"]
        if Lq > c["max_position_embeddings"]:
            raise ValueError(f"input_ids: {Lq} tokens, max_position_embeddings = {c['max_position_embeddings']}")
        new = lambda: torch.empty(B * Lq, D, dtype=self._dtype, device=self._device)
        tok = ops.gather_rows(self.tok, ids.view(-1), new())
        pos = ops.gather_rows(self.pos, torch.arange(Lq, dtype=torch.int32, device=self._device).repeat(B), new())
        x = ops.add(tok, pos, new())
        hidden = [x]
        for i in range(len(self.layers)):
            x = self.layer(x, i, B, Lq)
            hidden.append(x)
        last = ops.layernorm_rows(x, self.fln_w, self.fln_b, c["layer_norm_eps"])
        # the pooled row: the highest token id of each row for legacy configs (eos_token_id == 2), else the first eos_token_id position
        where = ids.argmax(dim=-1) if c["eos_token_id"] == 2 else (ids == c["eos_token_id"]).to(torch.int32).argmax(dim=-1)
        rows = (torch.arange(B, device=self._device) * Lq + where).to(torch.int32)
        pooled = ops.gather_rows(last, rows, torch.empty(B, D, dtype=self._dtype, device=self._device))
        return TextEncoderOutput(last.view(B, Lq, D), pooled, tuple(t.view(B, Lq, D) for t in hidden) if output_hidden_states else None)

    forward = __call__


class CLIPTextModelWithProjection(CLIPTextModel):
    """transformers' CLIPTextModelWithProjection on token ids: CLIPTextModel plus `text_projection` (no bias) on the pooled row. SD3's two CLIPs:
    CLIP-L (quick_gelu) and OpenCLIP bigG (hidden_act "gelu", the erf form; width 1280 = 20 heads of 64)."""

    KEYS = CLIPTextModel.KEYS + ("projection_dim",)
    ACTS = _CLIP_ACTS + ("gelu",)
    DROPPED = ("vision_model.", "visual_projection.", "logit_scale")

    def __init__(self, config: dict, device=None, dtype=BF):
        super().__init__(config, device=device, dtype=dtype)
        self.config.setdefault("projection_dim", 512)   # transformers' default
        self.proj = self._pack([("text_projection.weight", self.config["projection_dim"])], self.config["hidden_size"])

    def _canon(self, key):
        if key.endswith("text_projection.weight"):      # beside text_model.* on disk, not under it
            return key if key == "text_projection.weight" else None
        return super()._canon(key)

    def state_dict(self, prefix: str = "text_model.") -> Dict[str, torch.Tensor]:
        return {(k if k == "text_projection.weight" else prefix + k): v for k, v in self._views.items()}

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, output_hidden_states: bool = False, **_ignored) -> CLIPTextModelOutput:
        out = super().__call__(input_ids, output_hidden_states=output_hidden_states)
        pooled = out.pooler_output
        embeds = ops.small_linear(pooled, self.proj, None, torch.empty(pooled.shape[0], self.proj.shape[0], dtype=self._dtype, device=self._device))
        return CLIPTextModelOutput(embeds, out.last_hidden_state, out.hidden_states)

    forward = __call__


def _tokenize(tokenizer, prompt: List[str], max_length: int) -> torch.Tensor:
    return tokenizer(prompt, padding="max_length", max_length=max_length, truncation=True, return_length=False, return_overflowing_tokens=False,
                     return_tensors="pt").input_ids


def _batch_of(prompt, ids) -> int:
    if prompt is not None:
        return 1 if isinstance(prompt, str) else len(prompt)
    return ids.shape[0]


def _input_ids(tokenizer, prompt, ids, max_length: int) -> torch.Tensor:
    if tokenizer is not None:
        return _tokenize(tokenizer, [prompt] if isinstance(prompt, str) else list(prompt), max_length)
    if ids is None:
        raise ValueError("text_input_ids must be provided when the tokenizer is not specified")
    return ids


def encode_prompt(text_encoders, tokenizers, prompt, max_sequence_length, device=None, num_images_per_prompt: int = 1, text_input_ids_list=None):
    """The reference's src/text_encoder.py entry: text_encoders = [CLIP] or [CLIP, T5], tokenizers likewise (entries may be None: then
    text_input_ids_list carries the token ids). Returns (prompt_embeds [B n, L, d_model], pooled_prompt_embeds [B n, hidden], text_ids zeros [L, 3])
    for two encoders, the pooled vector alone for one. num_images_per_prompt = n repeats as the reference does: the n copies of a prompt's T5 rows sit
    next to each other (b0, b0, b1, b1), the pooled vectors repeat as a block (b0, b1, b0, b1: its `repeat(1, n, 1)` on a 2-D tensor)."""
    n = num_images_per_prompt
    tokenizers = list(tokenizers) if tokenizers is not None else [None] * len(text_encoders)
    ids = list(text_input_ids_list) if text_input_ids_list else [None] * len(text_encoders)
    clip = text_encoders[0]
    dtype = clip.dtype
    dev = device if device is not None else clip.device
    clip_ids = _input_ids(tokenizers[0], prompt, ids[0], 77)
    B = _batch_of(prompt, clip_ids)
    pooled = clip(clip_ids.to(dev), output_hidden_states=False).pooler_output.to(dtype=clip.dtype, device=dev)
    pooled = pooled.repeat(1, n, 1).view(B * n, -1)
    if len(text_encoders) == 1:
        return pooled
    t5 = text_encoders[1]
    dev5 = device if device is not None else t5.device
    t5_ids = _input_ids(tokenizers[1], prompt, ids[1], max_sequence_length)
    embeds = t5(t5_ids.to(dev5))[0].to(dtype=t5.dtype, device=dev5)
    Lq = embeds.shape[1]
    embeds = embeds.repeat(1, n, 1).view(B * n, Lq, -1)
    text_ids = torch.zeros(Lq, 3, device=dev5, dtype=dtype)
    return embeds, pooled, text_ids


# ---- SD3: three encoders (diffusers' StableDiffusion3Pipeline.encode_prompt; the reference's encode_condition_prompt) ------------------------------
def _sd3_clip(clip, tokenizer, prompt, ids, n: int, clip_skip: Optional[int], device):
    """One projected CLIP -> (hidden_states[-2] or [-(clip_skip + 2)] as [B n, 77, hidden], text_embeds [B n, projection_dim]). The sequence repeats
    with the copies of a prompt adjacent, the pooled vector as a block: diffusers' `repeat(1, n, 1)` on a 3-D and on a 2-D tensor."""
    ids = _input_ids(tokenizer, prompt, ids, 77)
    B = ids.shape[0]
    dev = device if device is not None else clip.device
    out = clip(ids.to(dev), output_hidden_states=True)
    pooled = out[0].to(dtype=clip.dtype, device=dev)
    seq = out.hidden_states[-2 if clip_skip is None else -(clip_skip + 2)].to(dtype=clip.dtype, device=dev)
    return seq.repeat(1, n, 1).view(B * n, seq.shape[1], -1), pooled.repeat(1, n, 1).view(B * n, -1)


def _sd3_embeds(text_encoders, tokenizers, prompts, ids, n: int, clip_skip, max_sequence_length: int, device, joint_attention_dim):
    """-> (prompt_embeds [B n, 77 + L3, joint_attention_dim], pooled [B n, projection_dim_l + projection_dim_g]) of one prompt triple."""
    seq_l, pooled_l = _sd3_clip(text_encoders[0], tokenizers[0], prompts[0], ids[0], n, clip_skip, device)
    seq_g, pooled_g = _sd3_clip(text_encoders[1], tokenizers[1], prompts[1], ids[1], n, clip_skip, device)
    clip_seq = torch.cat([seq_l, seq_g], dim=-1)
    t5 = text_encoders[2] if len(text_encoders) > 2 else None
    if t5 is None:
        if joint_attention_dim is None:
            raise ValueError("joint_attention_dim must be given when there is no third text encoder (its rows are zeros of that width)")
        t5_seq = torch.zeros(clip_seq.shape[0], max_sequence_length, joint_attention_dim, device=clip_seq.device, dtype=clip_seq.dtype)
    else:
        dev = device if device is not None else t5.device
        t5_ids = _input_ids(tokenizers[2], prompts[2], ids[2], max_sequence_length)
        t5_seq = t5(t5_ids.to(dev))[0].to(dtype=t5.dtype, device=dev)
        t5_seq = t5_seq.repeat(1, n, 1).view(t5_seq.shape[0] * n, t5_seq.shape[1], -1)
    if clip_seq.shape[-1] > t5_seq.shape[-1]:
        raise ValueError(f"the two CLIP widths ({clip_seq.shape[-1]} together) exceed the T5 width {t5_seq.shape[-1]}")
    clip_seq = torch.nn.functional.pad(clip_seq, (0, t5_seq.shape[-1] - clip_seq.shape[-1]))
    return torch.cat([clip_seq, t5_seq], dim=-2), torch.cat([pooled_l, pooled_g], dim=-1)


def _triple(x, what: str):
    x = [None, None, None] if x is None else list(x)
    if len(x) != 3:
        raise ValueError(f"{what}: expected three entries (CLIP-L, CLIP-G, T5), got {len(x)}")
    return x


def encode_prompt_sd3(text_encoders, tokenizers, prompt, prompt_2=None, prompt_3=None, negative_prompt=None, negative_prompt_2=None,
                      negative_prompt_3=None, do_classifier_free_guidance: bool = True, num_images_per_prompt: int = 1, clip_skip: Optional[int] = None,
                      max_sequence_length: int = 256, device=None, text_input_ids_list=None, negative_text_input_ids_list=None,
                      joint_attention_dim: Optional[int] = None):
    """diffusers' StableDiffusion3Pipeline.encode_prompt on text_encoders = [clip_l, clip_g, t5 or None] (the CLIPs are CLIPTextModelWithProjection),
    tokenizers likewise (entries may be None: then text_input_ids_list = [ids_l [B, 77], ids_g [B, 77], ids_t5 [B, L]] carries the token ids, and
    negative_text_input_ids_list the negatives'). Returns (prompt_embeds [B n, 77 + L3, joint_attention_dim], negative_prompt_embeds, pooled_prompt_embeds
    [B n, projection_dim_l + projection_dim_g], negative_pooled_prompt_embeds); the negatives are None without classifier-free guidance.

    Each CLIP gives hidden_states[-2] (or [-(clip_skip + 2)]) and its projected pooled vector; the two sequences, side by side and zero-padded to the T5
    width, come in front of the T5 rows of prompt_3 (zeros [B n, max_sequence_length, joint_attention_dim] without a T5)."""
    n = num_images_per_prompt
    text_encoders, tokenizers = _triple(text_encoders, "text_encoders"), _triple(tokenizers, "tokenizers")
    ids, neg_ids = _triple(text_input_ids_list, "text_input_ids_list"), _triple(negative_text_input_ids_list, "negative_text_input_ids_list")
    prompts = [prompt, prompt_2 if prompt_2 is not None else prompt, prompt_3 if prompt_3 is not None else prompt]
    if do_classifier_free_guidance and any(text_encoders[i] is not None and tokenizers[i] is None and neg_ids[i] is None for i in range(3)):
        raise ValueError("negative_text_input_ids_list must be provided for classifier-free guidance when the tokenizers are not specified")
    embeds, pooled = _sd3_embeds(text_encoders, tokenizers, prompts, ids, n, clip_skip, max_sequence_length, device, joint_attention_dim)
    if not do_classifier_free_guidance:
        return embeds, None, pooled, None
    B = embeds.shape[0] // n
    neg = negative_prompt if negative_prompt is not None else ""
    negs = [neg, negative_prompt_2 if negative_prompt_2 is not None else neg, negative_prompt_3 if negative_prompt_3 is not None else neg]
    negs = [B * [p] if isinstance(p, str) else list(p) for p in negs]
    if any(len(p) != B for p in negs):
        raise ValueError(f"negative prompts: batch sizes {[len(p) for p in negs]} do not match the prompt's {B}")
    # the negatives never take clip_skip (diffusers passes clip_skip=None for them)
    neg_embeds, neg_pooled = _sd3_embeds(text_encoders, tokenizers, negs, neg_ids, n, None, max_sequence_length, device, joint_attention_dim)
    return embeds, neg_embeds, pooled, neg_pooled


def encode_condition_prompt_sd3(text_encoders, tokenizers, prompt, num_images_per_prompt: int = 1, clip_skip: Optional[int] = None,
                                max_sequence_length: int = 256, device=None, text_input_ids_list=None, joint_attention_dim: Optional[int] = None):
    """The reference's UniGenSD3Pipeline.encode_condition_prompt (src/UniGenPipeline.py:34-105): the same assembly for the condition prompt (one text
    for all three encoders), no negatives. Returns (prompt_embeds, pooled_prompt_embeds)."""
    text_encoders, tokenizers = _triple(text_encoders, "text_encoders"), _triple(tokenizers, "tokenizers")
    return _sd3_embeds(text_encoders, tokenizers, [prompt] * 3, _triple(text_input_ids_list, "text_input_ids_list"), num_images_per_prompt, clip_skip,
                       max_sequence_length, device, joint_attention_dim)
