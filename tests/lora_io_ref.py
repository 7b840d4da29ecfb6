"""Reference side of the LoRA file tests: writers that restate the SAVE side of the three namings unigen_amd/lora_io.py reads, from a canonical
`{diffusers module: (A [r, K_in], B [N_out, r], alpha or None)}`, and the float64 merge `merge_ref`.

The BFL table below is restated independently of lora_io's (from the published FLUX layouts: BFL's `flux/model.py` module names, diffusers'
`FluxTransformer2DModel`): a BFL module that fuses several diffusers projections is generated as ONE `lora_down` and a full-height `lora_up`, and the
canonical per-projection entries are derived by slicing its rows. No file written by diffusers, sd-scripts or ComfyUI is available - format parity
unpinned."""
from typing import Dict, List, Optional, Tuple

import torch

BF = torch.bfloat16

# BFL module (N = block index) -> the diffusers projections its rows hold, in order
BFL_DOUBLE = {
    "img_attn.qkv": ["attn.to_q", "attn.to_k", "attn.to_v"], "txt_attn.qkv": ["attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"],
    "img_attn.proj": ["attn.to_out.0"], "txt_attn.proj": ["attn.to_add_out"],
    "img_mlp.0": ["ff.net.0.proj"], "img_mlp.2": ["ff.net.2"], "txt_mlp.0": ["ff_context.net.0.proj"], "txt_mlp.2": ["ff_context.net.2"],
    "img_mod.lin": ["norm1.linear"], "txt_mod.lin": ["norm1_context.linear"],
}
BFL_SINGLE = {"linear1": ["attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp"], "linear2": ["proj_out"], "modulation.lin": ["norm.linear"]}
BFL_TOP = {
    "img_in": "x_embedder", "txt_in": "context_embedder",
    "time_in.in_layer": "time_text_embed.timestep_embedder.linear_1", "time_in.out_layer": "time_text_embed.timestep_embedder.linear_2",
    "vector_in.in_layer": "time_text_embed.text_embedder.linear_1", "vector_in.out_layer": "time_text_embed.text_embedder.linear_2",
    "guidance_in.in_layer": "time_text_embed.guidance_embedder.linear_1", "guidance_in.out_layer": "time_text_embed.guidance_embedder.linear_2",
    "final_layer.linear": "proj_out", "final_layer.adaLN_modulation.1": "norm_out.linear",
}
SWAPPED = "final_layer.adaLN_modulation.1"      # BFL rows (shift, scale); diffusers rows (scale, shift)


def bfl_modules(num_layers: int, num_single_layers: int, guidance: bool = False) -> Dict[str, List[str]]:
    """Every BFL module of a FLUX transformer of this depth -> its diffusers projections."""
    out = {}
    for i in range(num_layers):
        for k, v in BFL_DOUBLE.items():
            out[f"double_blocks.{i}.{k}"] = [f"transformer_blocks.{i}.{x}" for x in v]
    for i in range(num_single_layers):
        for k, v in BFL_SINGLE.items():
            out[f"single_blocks.{i}.{k}"] = [f"single_transformer_blocks.{i}.{x}" for x in v]
    for k, v in BFL_TOP.items():
        if guidance or not k.startswith("guidance_in"):
            out[k] = [v]
    return out


def make_bfl_adapter(shapes: Dict[str, Tuple[int, int]], modules: Dict[str, List[str]], seed: int, ranks=(4, 8), b_std: float = 0.02,
                     alpha_of=lambda i, r: float(2 * r) if i % 3 else None):
    """-> (bfl {BFL module: (lora_down [r, K], lora_up [sum N, r], alpha or None)}, canon {diffusers module: (A, B, alpha)}).
    `shapes`: {diffusers module: (N_out, K_in)} of the model. Values are bf16-representable fp32, so every dtype a writer picks holds them exactly."""
    g = torch.Generator().manual_seed(seed)
    bfl, canon = {}, {}
    for i, (name, mods) in enumerate(modules.items()):
        r = ranks[i % len(ranks)]
        K = shapes[mods[0]][1]
        rows = [shapes[m][0] for m in mods]
        assert all(shapes[m][1] == K for m in mods), name
        down = (torch.randn(r, K, generator=g) / K ** 0.5).to(BF).float()
        up = (torch.randn(sum(rows), r, generator=g) * b_std).to(BF).float()
        alpha = alpha_of(i, r)
        bfl[name] = (down, up, alpha)
        parts = torch.split(up, rows, 0)
        if name == SWAPPED:
            h = up.shape[0] // 2
            parts = (torch.cat([up[h:], up[:h]], 0),)        # diffusers order (scale, shift) from BFL's (shift, scale)
        for m, b in zip(mods, parts):
            canon[m] = (down, b.contiguous(), alpha)
    return bfl, canon


def write_kohya(bfl: Dict[str, tuple], alpha_dtype=torch.float16) -> Dict[str, torch.Tensor]:
    """sd-scripts: `lora_unet_<BFL path, dots as underscores>.lora_down.weight / .lora_up.weight / .alpha` (alpha a 0-dim tensor)."""
    sd = {}
    for name, (down, up, alpha) in bfl.items():
        stem = "lora_unet_" + name.replace(".", "_")
        sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"] = down.clone(), up.clone()
        if alpha is not None:
            sd[stem + ".alpha"] = torch.tensor(alpha, dtype=alpha_dtype)
    return sd


def write_bfl(bfl: Dict[str, tuple], prefix: str = "diffusion_model.") -> Dict[str, torch.Tensor]:
    """ComfyUI / BFL-dotted: `[diffusion_model.]<BFL path>.lora_A.weight / .lora_B.weight / .alpha`."""
    sd = {}
    for name, (down, up, alpha) in bfl.items():
        sd[f"{prefix}{name}.lora_A.weight"], sd[f"{prefix}{name}.lora_B.weight"] = down.clone(), up.clone()
        if alpha is not None:
            sd[f"{prefix}{name}.alpha"] = torch.tensor(alpha, dtype=torch.float32)
    return sd


def write_diffusers(canon: Dict[str, tuple], prefix: str = "transformer.", sides=("lora_A", "lora_B"), adapter: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """diffusers / PEFT: `<prefix><module>.<lora_A>[.<adapter>].weight`, `<lora_B>`, optional `<module>.alpha`. sides: ("lora_A", "lora_B"),
    ("lora_down", "lora_up") or the legacy ("lora.down", "lora.up")."""
    sd = {}
    mid = f".{adapter}" if adapter else ""
    for name, (A, B, alpha) in canon.items():
        sd[f"{prefix}{name}.{sides[0]}{mid}.weight"], sd[f"{prefix}{name}.{sides[1]}{mid}.weight"] = A.clone(), B.clone()
        if alpha is not None:
            sd[f"{prefix}{name}.alpha"] = torch.tensor(alpha, dtype=torch.float32)
    return sd


def scaling(entry) -> float:
    A, _, alpha = entry
    return (alpha if alpha is not None else A.shape[0]) / A.shape[0]


def merge_ref(W: torch.Tensor, adapters, dtype):
    """float64: W + sum_a Bs_a A_a with Bs_a = dtype(fp32(B_a) * scaling_a) as lora.fuse_adapters builds it; A, B, W are read at `dtype`.
    adapters: [(A [r, K], B [N, r], scaling)]. Returns (exact [N, K] float64, mag [N, K] float64 = |W| + sum_j |Bs_nj A_jk|, P = exact - W)."""
    Wd = W.to(dtype).double()
    P = torch.zeros_like(Wd)
    mag = Wd.abs()
    for A, B, s in adapters:
        Bs = (B.to(dtype).float() * s).to(dtype).double()
        Ad = A.to(dtype).double()
        P += Bs @ Ad
        mag += Bs.abs() @ Ad.abs()
    return Wd + P, mag, P


def merged_state(state: Dict[str, torch.Tensor], canon: Dict[str, tuple], dtype, only=None) -> Dict[str, torch.Tensor]:
    """`state` with merge_ref applied to `<module>.weight` for every canonical entry (or those in `only`), rounded to `dtype`."""
    st = dict(state)
    for m, e in canon.items():
        if only is not None and m not in only:
            continue
        st[m + ".weight"] = merge_ref(state[m + ".weight"], [(e[0], e[1], scaling(e))], dtype)[0].to(dtype)
    return st


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 (8 significant bits) at |x| (float64 in, float64 out; 0 at 0)."""
    _, e = torch.frexp(x.abs().double())             # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x, dtype=torch.float64), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8))
