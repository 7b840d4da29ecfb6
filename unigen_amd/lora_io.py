"""The adapter wire format: FLUX / SD3 LoRA files -> `{module name: (A [r, K_in], B [N_out, r], alpha)}` under the engines' own module names.

The reference writes adapters with `FluxPipeline.save_lora_weights` and reads them back with `FluxPipeline.lora_state_dict` +
`set_peft_model_state_dict` (src/hook.py:29-70); that reader also accepts the kohya (sd-scripts) and BFL-named (ComfyUI) files the FLUX ecosystem
ships. Three key forms are recognised here:

  1. diffusers / PEFT   `[transformer.|base_model.model.]<module>.lora_A[.<adapter>].weight`, `lora_B`; aliases `lora_down` / `lora_up` and the
                        legacy `lora.down` / `lora.up`; optional `<module>.alpha`. Any engine: these are the module names the engines use.
  2. kohya              `lora_unet_<BFL path with underscores>.lora_down.weight`, `.lora_up.weight`, `.alpha` (FLUX only).
  3. BFL-dotted         `[diffusion_model.]double_blocks.N.img_attn.qkv.lora_A.weight` ... (FLUX only).

BFL names fuse projections that diffusers keeps apart (`qkv`, the single block's `linear1`): their `lora_up` is split by rows and every part shares
the one `lora_down` (`BFL_MAP`). Scaling is alpha / r, r read from the shapes; a missing alpha means alpha = r. Text-encoder entries are reported
as ignored; every other key that is not understood is a KeyError naming it - nothing is dropped silently. Host only: no kernel is involved until
`HipModule.load_lora_weights` attaches the result and `fuse_lora` merges it.

Parity note: diffusers is not installed and no file of any of these formats exists beside this code, so the three namings are pinned only by
writers that restate their published SAVE side (tests/lora_io_ref.py) - format parity unpinned.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

LORA_FILE = "pytorch_lora_weights.safetensors"       # what FluxPipeline.save_lora_weights writes under <dir>/<adapter>/ (src/hook.py:42-45)

Entry = Tuple[torch.Tensor, torch.Tensor, Optional[float]]


class LoraReport(NamedTuple):
    live: List[str]          # modules whose GEMM launch takes the adapter K-segment (HipModule.LORA_CAPABLE): attached, switched by enable_lora
    merge_only: List[str]    # modules the engine runs another way (AdaLN linears, embedders, experts, proj_out ...): reach the output through fuse_lora only
    ignored: List[str]       # keys left out on purpose: text-encoder entries, and (strict=False) modules the model does not have


# ----------------------------------------------------------------------------------------------------------------------
# reading
# ----------------------------------------------------------------------------------------------------------------------
def read_lora_file(path) -> Dict[str, torch.Tensor]:
    """A `.safetensors` file, a directory holding `pytorch_lora_weights.safetensors`, or a `.bin` / `.pt` state dict -> {key: CPU tensor}."""
    path = os.fspath(path)
    if os.path.isdir(path):
        f = os.path.join(path, LORA_FILE)
        if not os.path.exists(f):
            raise OSError(f"{path}: no {LORA_FILE} in this directory")
        path = f
    if not os.path.exists(path):
        raise OSError(f"{path}: no such LoRA file")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    if path.endswith((".bin", ".pt")):
        from .checkpoint import _torch_load
        return _torch_load(path)
    raise ValueError(f"{path}: expected a .safetensors, .bin or .pt file, or a directory holding {LORA_FILE}")


# ----------------------------------------------------------------------------------------------------------------------
# key forms
# ----------------------------------------------------------------------------------------------------------------------
_SIDE = {"lora_A": "A", "lora_down": "A", "lora.down": "A", "lora_B": "B", "lora_up": "B", "lora.up": "B"}
_WEIGHT_RE = re.compile(r"^(?P<mod>.+?)\.(?P<side>lora_A|lora_B|lora_down|lora_up|lora\.down|lora\.up)(?:\.(?P<adapter>[^.]+))?\.weight$")
_ALPHA_RE = re.compile(r"^(?P<mod>.+)\.alpha$")
_PREFIXES = ("base_model.model.", "transformer.", "diffusion_model.")
_TEXT_ENCODER_RE = re.compile(r"^(lora_te\d*_|text_encoder(_\d+)?\.)")

# kohya: one regular expression per template (the BFL path with "." written as "_"; never split on "_": `attn_qkv`, `in_layer` carry their own)
_KOHYA_DOUBLE_RE = re.compile(r"^lora_unet_double_blocks_(\d+)_(img|txt)_(attn_qkv|attn_proj|mlp_0|mlp_2|mod_lin)$")
_KOHYA_SINGLE_RE = re.compile(r"^lora_unet_single_blocks_(\d+)_(linear1|linear2|modulation_lin)$")
_KOHYA_DOUBLE_LEAF = {"attn_qkv": "attn.qkv", "attn_proj": "attn.proj", "mlp_0": "mlp.0", "mlp_2": "mlp.2", "mod_lin": "mod.lin"}
_KOHYA_SINGLE_LEAF = {"linear1": "linear1", "linear2": "linear2", "modulation_lin": "modulation.lin"}
_KOHYA_TOP = {"lora_unet_" + k.replace(".", "_"): k for k in (
    "img_in", "txt_in", "time_in.in_layer", "time_in.out_layer", "vector_in.in_layer", "vector_in.out_layer", "guidance_in.in_layer",
    "guidance_in.out_layer", "final_layer.linear", "final_layer.adaLN_modulation.1")}

# BFL -> diffusers, FLUX engines only (restated from diffusers' published kohya / BFL conversion, loaders/lora_conversion_utils.py).
# value: (diffusers module names, how the rows of lora_up are handled)
_BFL_DOUBLE = {
    "img_attn.qkv": (("attn.to_q", "attn.to_k", "attn.to_v"), "thirds"),
    "txt_attn.qkv": (("attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"), "thirds"),
    "img_attn.proj": (("attn.to_out.0",), None), "txt_attn.proj": (("attn.to_add_out",), None),
    "img_mlp.0": (("ff.net.0.proj",), None), "img_mlp.2": (("ff.net.2",), None),
    "txt_mlp.0": (("ff_context.net.0.proj",), None), "txt_mlp.2": (("ff_context.net.2",), None),
    "img_mod.lin": (("norm1.linear",), None), "txt_mod.lin": (("norm1_context.linear",), None),
}
_BFL_SINGLE = {
    "linear1": (("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp"), "qkv_mlp"),      # rows [D, D, D, rest]: the order of engine._pack(... ".qkv_mlp.w")
    "linear2": (("proj_out",), None),
    "modulation.lin": (("norm.linear",), None),
}
_BFL_TOP = {
    "img_in": ("x_embedder", None), "txt_in": ("context_embedder", None),
    "time_in.in_layer": ("time_text_embed.timestep_embedder.linear_1", None), "time_in.out_layer": ("time_text_embed.timestep_embedder.linear_2", None),
    "vector_in.in_layer": ("time_text_embed.text_embedder.linear_1", None), "vector_in.out_layer": ("time_text_embed.text_embedder.linear_2", None),
    "guidance_in.in_layer": ("time_text_embed.guidance_embedder.linear_1", None), "guidance_in.out_layer": ("time_text_embed.guidance_embedder.linear_2", None),
    "final_layer.linear": ("proj_out", None),
    "final_layer.adaLN_modulation.1": ("norm_out.linear", "swap_halves"),              # BFL stores (shift, scale), diffusers (scale, shift)
}
_BFL_DOUBLE_RE = re.compile(r"^double_blocks\.(\d+)\.(" + "|".join(re.escape(k) for k in _BFL_DOUBLE) + r")$")
_BFL_SINGLE_RE = re.compile(r"^single_blocks\.(\d+)\.(" + "|".join(re.escape(k) for k in _BFL_SINGLE) + r")$")
_BFL_HEAD_RE = re.compile(r"^(double_blocks|single_blocks|img_in|txt_in|time_in|vector_in|guidance_in|final_layer)(\.|$)")


def _bfl_targets(name: str, key: str):
    """BFL module name -> ([diffusers module names], lora_up row handling). Unknown BFL names are refused by key."""
    m = _BFL_DOUBLE_RE.match(name)
    if m:
        mods, how = _BFL_DOUBLE[m.group(2)]
        return [f"transformer_blocks.{m.group(1)}.{x}" for x in mods], how
    m = _BFL_SINGLE_RE.match(name)
    if m:
        mods, how = _BFL_SINGLE[m.group(2)]
        return [f"single_transformer_blocks.{m.group(1)}.{x}" for x in mods], how
    if name in _BFL_TOP:
        mod, how = _BFL_TOP[name]
        return [mod], how
    raise KeyError(f"LoRA key {key!r}: {name!r} is not a BFL FLUX module this reader maps to a diffusers name")


def _alpha_value(v, key: str) -> float:
    t = torch.as_tensor(v)
    if t.numel() != 1:
        raise ValueError(f"LoRA key {key!r}: alpha must hold one number, got shape {tuple(t.shape)}")
    return float(t.float().reshape(()))


def _parse_key(key: str):
    """-> ("te", None) | (form, module, field) with form in {"diffusers", "bfl"}, field in {"A", "B", "alpha"}; KeyError for anything else."""
    if _TEXT_ENCODER_RE.match(key):
        return "te", None, None
    if key.startswith("lora_unet_"):
        stem, _, rest = key.partition(".")
        field = {"lora_down.weight": "A", "lora_up.weight": "B", "alpha": "alpha"}.get(rest)
        m = _KOHYA_DOUBLE_RE.match(stem)
        if m:
            name = f"double_blocks.{m.group(1)}.{m.group(2)}_{_KOHYA_DOUBLE_LEAF[m.group(3)]}"
        else:
            m = _KOHYA_SINGLE_RE.match(stem)
            name = f"single_blocks.{m.group(1)}.{_KOHYA_SINGLE_LEAF[m.group(2)]}" if m else _KOHYA_TOP.get(stem)
        if field is None or name is None:
            raise KeyError(f"LoRA key {key!r} is not a kohya FLUX entry this reader understands (lora_down / lora_up / alpha of a known module)")
        return "bfl", name, field
    k = key
    stripped = True
    while stripped:
        stripped = False
        for p in _PREFIXES:
            if k.startswith(p):
                k, stripped = k[len(p):], True
    m = _WEIGHT_RE.match(k)
    if m:
        mod, field = m.group("mod"), _SIDE[m.group("side")]
    else:
        m = _ALPHA_RE.match(k)
        if not m:
            raise KeyError(f"LoRA key {key!r} is not a lora_A / lora_B weight or an alpha (DoRA scales, LoHa / LoKr factors, full-weight `diff`s, "
                           "norm and bias deltas are not supported)")
        mod, field = m.group("mod"), "alpha"
    return ("bfl" if _BFL_HEAD_RE.match(mod) else "diffusers"), mod, field


def _entries(sd: Dict[str, torch.Tensor]):
    """Any of the three key forms -> ({diffusers module: (A, B, alpha or None)}, ignored keys, saw_bfl_names)."""
    raw: Dict[Tuple[str, str], Dict[str, Tuple[str, torch.Tensor]]] = {}
    ignored: List[str] = []
    for key, val in sd.items():
        form, mod, field = _parse_key(key)
        if form == "te":
            ignored.append(key)
            continue
        slot = raw.setdefault((form, mod), {})
        if field in slot:
            raise KeyError(f"LoRA key {key!r} repeats {slot[field][0]!r}")
        slot[field] = (key, val)
    out: Dict[str, Entry] = {}
    saw_bfl = False
    for (form, mod), slot in raw.items():
        anykey = next(iter(slot.values()))[0]
        if "A" not in slot or "B" not in slot:
            raise KeyError(f"LoRA key {anykey!r}: module {mod!r} has no {'lora_A / lora_down' if 'A' not in slot else 'lora_B / lora_up'} weight beside it")
        (ka, A), (kb, B) = slot["A"], slot["B"]
        if A.dim() != 2 or B.dim() != 2:
            raise KeyError(f"LoRA key {ka if A.dim() != 2 else kb!r}: only 2-D (linear) adapter weights are supported")
        if A.shape[0] != B.shape[1]:
            raise ValueError(f"LoRA key {kb!r}: lora_B is {tuple(B.shape)} but lora_A {ka!r} has rank {A.shape[0]}")
        alpha = _alpha_value(slot["alpha"][1], slot["alpha"][0]) if "alpha" in slot else None
        if form == "diffusers":
            parts = [(mod, B)]
        else:
            saw_bfl = True
            mods, how = _bfl_targets(mod, ka)
            if how == "thirds":
                if B.shape[0] % 3:
                    raise ValueError(f"LoRA key {kb!r}: {B.shape[0]} rows do not split into q | k | v thirds")
                rows = [B.shape[0] // 3] * 3
            elif how == "qkv_mlp":
                D = A.shape[1]                                                    # linear1 reads the block's hidden state: K_in = D
                if B.shape[0] <= 3 * D:
                    raise ValueError(f"LoRA key {kb!r}: {B.shape[0]} rows do not split into [D, D, D, mlp] with D = {D}")
                rows = [D, D, D, B.shape[0] - 3 * D]
            elif how == "swap_halves":
                if B.shape[0] % 2:
                    raise ValueError(f"LoRA key {kb!r}: {B.shape[0]} rows do not split into (shift, scale) halves")
                h = B.shape[0] // 2
                B, rows = torch.cat([B[h:], B[:h]], 0), [B.shape[0]]
            else:
                rows = [B.shape[0]]
            parts = list(zip(mods, torch.split(B, rows, 0)))
        for name, b in parts:
            if name in out:
                raise KeyError(f"LoRA key {kb!r}: module {name!r} is defined twice in this file")
            out[name] = (A, b.contiguous(), alpha)
    return out, ignored, saw_bfl


def lora_state_dict(path_or_dict) -> Dict[str, torch.Tensor]:
    """`FluxPipeline.lora_state_dict(path)` as the reference's load hook consumes it (src/hook.py:60-67): `transformer.<module>.lora_A.weight`,
    `transformer.<module>.lora_B.weight`, and `transformer.<module>.alpha` (a 0-dim fp32 tensor) where the file had one - whatever naming the file
    used. Text-encoder entries keep their keys (the hook filters on the `transformer.` prefix)."""
    sd = path_or_dict if isinstance(path_or_dict, dict) else read_lora_file(path_or_dict)
    entries, ignored, _ = _entries(sd)
    out: Dict[str, torch.Tensor] = {}
    for name, (A, B, alpha) in entries.items():
        out[f"transformer.{name}.lora_A.weight"] = A
        out[f"transformer.{name}.lora_B.weight"] = B
        if alpha is not None:
            out[f"transformer.{name}.alpha"] = torch.tensor(alpha, dtype=torch.float32)
    for k in ignored:
        out[k] = sd[k]
    return out


def convert(sd: Dict[str, torch.Tensor], model, strict: bool = True) -> Tuple[Dict[str, Entry], LoraReport]:
    """-> ({module name of `model`: (A [r, K_in], B [N_out, r], alpha or None)}, LoraReport). BFL / kohya names are mapped only for engines that declare `BFL_NAMES = True` (the FLUX ones);
    a module the model does not have raises under `strict` (otherwise its name goes to report.ignored); shapes are checked against the weights."""
    entries, ignored, saw_bfl = _entries(sd)
    if saw_bfl and not getattr(model, "BFL_NAMES", False):
        bad = next(k for k in sd if not _TEXT_ENCODER_RE.match(k) and _parse_key(k)[0] == "bfl")
        raise KeyError(f"LoRA key {bad!r} uses kohya / BFL FLUX names, which have no mapping onto {type(model).__name__}")
    params = dict(model.named_parameters())
    out: Dict[str, Entry] = {}
    live, merge_only = [], []
    for name, (A, B, alpha) in entries.items():
        w = params.get(name + ".weight")
        if w is None:
            if strict:
                raise KeyError(f"LoRA module {name!r} does not exist in {type(model).__name__}")
            ignored.append(name)
            continue
        if w.dim() != 2:
            raise KeyError(f"LoRA module {name!r}: its weight is {tuple(w.shape)}, not a linear projection")
        if A.shape[1] != w.shape[1] or B.shape[0] != w.shape[0]:
            raise ValueError(f"LoRA module {name!r}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not fit the weight {tuple(w.shape)}")
        out[name] = (A, B, alpha)
        (live if model.lora_capable(name) else merge_only).append(name)
    return out, LoraReport(live, merge_only, ignored)


def save_lora_weights(save_directory, model, adapter: str) -> str:
    """The reference's save hook for one adapter (src/hook.py:41-45, `FluxPipeline.save_lora_weights(dir, transformer_lora_layers=...)`):
    `<dir>/pytorch_lora_weights.safetensors` with `transformer.`-prefixed `model.lora_state_dict(adapter)` keys plus one `alpha` per module; the
    adapter's merge-only entries (load_lora_weights) are written too, so that a loaded file round-trips. Returns the file's path."""
    from safetensors.torch import save_file
    out: Dict[str, torch.Tensor] = {}
    for name, A, B, alpha in model.lora_entries(adapter):
        out[f"transformer.{name}.lora_A.weight"] = A.detach().cpu().contiguous()
        out[f"transformer.{name}.lora_B.weight"] = B.detach().cpu().contiguous()
        out[f"transformer.{name}.alpha"] = torch.tensor(float(alpha), dtype=torch.float32)
    if not out:
        raise KeyError(f"save_lora_weights: no projection carries an adapter named {adapter!r}")
    os.makedirs(os.fspath(save_directory), exist_ok=True)
    path = os.path.join(os.fspath(save_directory), LORA_FILE)
    save_file(out, path)
    return path
