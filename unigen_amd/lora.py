"""Per-condition LoRA switch on MI355X, and the engines' adapter management.

The reference ships `src/lora_switching_module.py` (`module_active_adapters`, `enable_lora`) on top of PEFT 0.15 tuner layers, but
never invokes it (imported, not called; inherited from UniCombine). This module supplies the same API over a PEFT-free
LoRA-capable linear whose forward is ONE fused GEMM in libunigen_hip.so:   y = x W^T + b + sum_a scaling_a * (x A_a^T) B_a^T
(the adapter product is a second K-segment of the base GEMM's accumulators, `ug_gemm_desc.lora_T / lora_B`).

Semantics restated from PEFT 0.15 `LoraLayer`: `scaling[a] = lora_alpha / r`; `set_scale(a, s)` sets `scaling[a] = s * lora_alpha / r`.
`enable_lora.__exit__` therefore "restores" through `set_scale(saved_scaling)`, i.e. multiplies by lora_alpha / r again
(idempotent only when alpha == r) - kept as the reference has it.

Everything the engines know about adapters lives here as well: the parameter holders that carry them (`_Holder`, `_LoRAHolder`), `adapter_operands` -
the ONE builder of a launch's A_cat / B_bd, behind inference, training and the merge - and `LoRAHost`, the mixin `engine.HipModule` inherits
(attachment, PEFT key forms, LoRA files, merge / unmerge, `_lora_gemm`: a projection's launch with its adapters). Nothing here imports the engine.
"""
from __future__ import annotations

import contextlib
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple, Type

import torch
from torch import nn

from . import lib as L
from . import ops

BF = torch.bfloat16
_RANK_PAD = 64    # the GEMM's K-tile: adapter ranks are zero-padded to a multiple of it


class _AdapterWeight(nn.Module):
    """One side of one adapter: holds `.weight` so that the state-dict keys read `<proj>.lora_A.<adapter>.weight` / `<proj>.lora_B.<adapter>.weight`
    as PEFT's `ModuleDict` of `nn.Linear` does. Never called: the arithmetic is the K-segment of ug_gemm_bf16."""

    def __init__(self, w: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(w, requires_grad=False)


class LoRALayer:
    """The duck-typed stand-in for a PEFT `BaseTunerLayer` / `LoraLayer` (peft 0.15 tuners/lora/layer.py): `lora_A`, `lora_B`, `r`, `lora_alpha`,
    `scaling`, `active_adapters`, `set_scale`. Mixed into `LoRALinear` (a stand-alone layer) and into the parameter holders of the engines'
    projections (`HipModule.add_lora`), so that `enable_lora(list(model.modules()), [...])` - the reference's call shape - finds them."""

    def _init_lora(self) -> None:
        self.lora_A, self.lora_B = nn.ModuleDict(), nn.ModuleDict()
        self.r: Dict[str, int] = {}
        self.lora_alpha: Dict[str, float] = {}
        self.scaling: Dict[str, float] = {}
        self.active_adapters: List[str] = []
        self.fused_adapters: set = set()          # merged into the base weight (HipModule.fuse_lora): no longer part of the forward

    def add_adapter(self, name: str, r: int, lora_alpha: float, A: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None,
                    generator: Optional[torch.Generator] = None) -> None:
        """peft `update_layer`: A [r, in] (default: uniform(-1/sqrt(in), 1/sqrt(in)), PEFT's kaiming_uniform(a = sqrt 5)), B [out, r] (default: zeros)."""
        w = self.weight
        N, K = w.shape
        if A is None:
            bound = 1.0 / (K ** 0.5)
            A = torch.empty(r, K, dtype=torch.float32).uniform_(-bound, bound, generator=generator)
        if B is None:
            B = torch.zeros(N, r)
        if tuple(A.shape) != (r, K) or tuple(B.shape) != (N, r):
            raise ValueError(f"adapter {name!r}: A must be [{r}, {K}] and B [{N}, {r}], got {tuple(A.shape)} / {tuple(B.shape)}")
        self.lora_A[name] = _AdapterWeight(A.detach().to(w.device, w.dtype).contiguous())
        self.lora_B[name] = _AdapterWeight(B.detach().to(w.device, w.dtype).contiguous())
        self.r[name], self.lora_alpha[name] = int(r), float(lora_alpha)
        self.scaling[name] = float(lora_alpha) / r
        if name not in self.active_adapters:
            self.active_adapters.append(name)

    def remove_adapter(self, name: str) -> None:
        """The inverse of add_adapter."""
        del self.lora_A[name], self.lora_B[name]
        for d in (self.r, self.lora_alpha, self.scaling):
            d.pop(name, None)
        if name in self.active_adapters:
            self.active_adapters.remove(name)
        self.fused_adapters.discard(name)

    def set_scale(self, adapter: str, scale: float) -> None:          # peft LoraLayer.set_scale
        if adapter in self.scaling:
            self.scaling[adapter] = scale * self.lora_alpha[adapter] / self.r[adapter]

    def scale_layer(self, scale: float) -> None:                      # peft LoraLayer.scale_layer (diffusers scale_lora_layers calls it)
        if scale == 1:
            return
        for a in self.active_adapters:
            if a in self.lora_A:
                self.scaling[a] *= scale

    def unscale_layer(self, scale=None) -> None:                      # peft LoraLayer.unscale_layer
        for a in self.active_adapters:
            if a not in self.lora_A:
                continue
            if scale is None:
                self.scaling[a] = self.lora_alpha[a] / self.r[a]
            else:
                self.scaling[a] /= scale

    def live_adapters(self) -> List[str]:
        """The adapters that contribute to this layer's output right now: active, known, scaling != 0, not merged into the base weight."""
        return [a for a in self.active_adapters if a in self.scaling and self.scaling[a] != 0.0 and a not in self.fused_adapters]


class _Holder(nn.Module):
    """Parameter container; the arithmetic lives in libunigen_hip.so, so calling it is an error."""

    def forward(self, *a, **k):  # pragma: no cover
        raise L.UniGenHipError("parameter holder: unigen_amd modules are executed by the HIP engine, not called directly")

    def _adopt(self, src: nn.Module, skip: Sequence[str] = ()) -> "_Holder":
        """Take over `src`'s parameters - the SAME Parameter objects: packed views, state-dict keys and optimiser references survive - and submodules."""
        for n, p_ in src._parameters.items():
            self.register_parameter(n, p_)
        for n, m in src._modules.items():
            if n not in skip:
                self.add_module(n, m)
        return self


class _LoRAHolder(_Holder, LoRALayer):
    """The holder of a projection that carries LoRA adapters (HipModule.add_lora): the same `weight` / `bias` parameters plus
    `lora_A.<adapter>.weight`, `lora_B.<adapter>.weight` and the PEFT layer attributes `enable_lora` reads."""

    def __init__(self, plain: _Holder):
        super().__init__()
        self._adopt(plain)
        self._init_lora()

    def plain(self) -> _Holder:
        """The inverse of the constructor: a plain holder of the same parameters and submodules, `lora_A` / `lora_B` left behind."""
        return _Holder()._adopt(self, skip=("lora_A", "lora_B"))


def _suffix_match(name: str, keys: Sequence[str]) -> bool:
    """PEFT's `target_modules` rule: a key names a module by its full name or by a dotted suffix of it."""
    return any(name == k or name.endswith("." + k) for k in keys)


def adapter_operands(blocks: Sequence[Sequence[Tuple[torch.Tensor, torch.Tensor, float]]], widths: Sequence[int], dtype, device):
    """The adapter operands of ONE GEMM launch over row-concatenated weights. blocks[i]: the (A [r, K], B [widths[i], r], scale) of projection i,
    empty for a projection without adapters; widths = the projections' output widths. Returns A_cat [Rp, K] = every A stacked along the rank, and
    B_bd [sum widths, Rp] = block-diagonal, projection i's rows holding dtype(scale * B) in the columns of ITS adapters, zero elsewhere; the rank is
    zero-padded to the GEMM's K-tile. (None, None) without any block. Built from differentiable torch ops (cat, pad, `(B.float() * s).to(dtype)`):
    with gradients on they reach every A and B - the scaling included, the zero blocks and the padded rank receiving nothing; the rounding of
    s * B to `dtype` is the identity in the backward."""
    pad = torch.nn.functional.pad
    R = sum(a.shape[0] for bl in blocks for a, _, _ in bl)
    if R == 0:
        return None, None
    Rp = (R + _RANK_PAD - 1) // _RANK_PAD * _RANK_PAD
    A_cat = pad(torch.cat([a.to(device, dtype) for bl in blocks for a, _, _ in bl], 0), (0, 0, 0, Rp - R))
    rows, c0 = [], 0
    for bl, N in zip(blocks, widths):
        if bl:
            b = torch.cat([(b.float() * s).to(device, dtype) for _, b, s in bl], 1)
            rows.append(pad(b, (c0, Rp - c0 - b.shape[1])))
            c0 += b.shape[1]
        else:
            rows.append(torch.zeros(N, Rp, device=device, dtype=dtype))
    return A_cat, torch.cat(rows, 0)


def _live_blocks(layers: Sequence[Optional[LoRALayer]]):        # adapter_operands' `blocks` of each layer's live adapters; None = a projection without any
    return [[(lay.lora_A[a].weight, lay.lora_B[a].weight, lay.scaling[a]) for a in lay.live_adapters()] if lay is not None else [] for lay in layers]


@torch.no_grad()
def fuse_adapters(layers: List[Optional["LoRALayer"]], widths: List[int], dtype, device):
    """adapter_operands over the live adapters of `layers`, for the inference launches. (None, None) when nothing is live."""
    return adapter_operands(_live_blocks(layers), widths, dtype, device)


def fuse_adapters_autograd(layers: List[Optional["LoRALayer"]], widths: List[int], dtype, device):
    """fuse_adapters for the differentiable forward (unigen_amd/training.py): the same A_cat / B_bd values with gradients on, which reach every
    adapter's own `lora_A.<name>.weight` / `lora_B.<name>.weight`. Not cached: the result belongs to one forward's tape.
    Returns (A_cat, B_bd, has) - has[i]: projection i carries a live adapter - or None when nothing is live."""
    blocks = _live_blocks(layers)
    A_cat, B_bd = adapter_operands(blocks, widths, dtype, device)
    return None if A_cat is None else (A_cat, B_bd, tuple(bool(bl) for bl in blocks))


class LoRAHost:
    """What a HIP engine knows about LoRA adapters, mixed into `engine.HipModule` in front of `nn.Module`. It needs from its host: `named_modules` /
    `named_parameters` / `get_parameter` / `get_submodule` / `requires_grad_` of nn.Module, the properties `dtype` and `device`, `_w(name, shape)`
    (the workspace), the `_pname_cache` attribute it resets when modules change, and `_weights_rewritten(params)`, which drops what the host derived
    from base weights that were overwritten in place and clears `_lora_fused`."""

    # The projections whose GEMM launches take the adapter K-segment (every attention / feed-forward projection of a joint or single block, in
    # the base, control, shared-expert and consistency blocks alike). PEFT matches `target_modules` by module-name suffix; a suffix that hits a
    # parameter the engine runs another way (AdaLN linears, embedders, experts, zero-res projections) is refused rather than silently ignored.
    LORA_CAPABLE = ("attn.to_q", "attn.to_k", "attn.to_v", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_out.0", "attn.to_add_out",
                    "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2",
                    "proj_mlp", "proj_out")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._lora_sites: Dict[str, _LoRAHolder] = {}     # projection prefix -> its adapter-carrying holder (add_lora)
        self._lora_fused: Dict[Tuple, Tuple] = {}         # fused adapter operands per launch (prefixes + adapter state), see _lora_operands
        self._lora_merge_only: Dict[str, Dict[str, Tuple]] = {}   # adapter -> {module: (A, B, alpha)} outside LORA_CAPABLE (load_lora_weights): run only merged
        self._lora_merged: Dict[str, float] = {}          # adapter -> lora_scale of the adapters fuse_lora merged into the base weights
        self._lora_backup: Optional[Dict[str, torch.Tensor]] = None   # parameter name -> its bytes before the first fuse_lora (None: nothing fused / no backup)

    # ------------------------------------------------------------------ bookkeeping ------------------------------------
    @classmethod
    def lora_capable(cls, name: str) -> bool:
        """Does the module `name` take a live adapter (the rule add_lora enforces)? Everything else can only be merged (fuse_lora)."""
        return _suffix_match(name, cls.LORA_CAPABLE) and name != "proj_out" and ".experts." not in name

    def adapter_names(self, merge_only: bool = True) -> set:
        """The adapters this model carries: on its live sites and - unless `merge_only` is False - as merge-only entries."""
        return {a for m in self._lora_sites.values() for a in m.lora_A} | (set(self._lora_merge_only) if merge_only else set())

    def lora_entries(self, adapter: str, merge_only: bool = True) -> Iterator[Tuple[str, torch.Tensor, torch.Tensor, float]]:
        """(module name, A, B, alpha) of every module that carries `adapter`: live sites first, then - unless `merge_only` is False - merge-only entries."""
        for name, m in self._lora_sites.items():
            if adapter in m.lora_A:
                yield name, m.lora_A[adapter].weight, m.lora_B[adapter].weight, m.lora_alpha[adapter]
        if merge_only:
            for name, (A, B, alpha) in self._lora_merge_only.get(adapter, {}).items():
                yield name, A, B, alpha

    def _swap_holder(self, name: str, holder: _Holder) -> None:
        parent_name, _, leaf = name.rpartition(".")
        (self.get_submodule(parent_name) if parent_name else self)._modules[leaf] = holder

    # ------------------------------------------------------------------ live adapters ----------------------------------
    def add_lora(self, target_suffixes: Sequence[str], adapter_name: str, r: int, lora_alpha: float, A=None, B=None, prefix: str = "",
                 init_lora_weights: bool = True, seed: int = 0) -> Sequence[str]:
        """Attach the LoRA adapter `adapter_name` (rank r, scaling lora_alpha / r) to every projection whose module name ends with one of
        `target_suffixes` (PEFT's `target_modules` rule: name == key or name.endswith("." + key)) and starts with `prefix` (e.g.
        "control_joint_trans_blocks." for the per-condition adapters of the control branch). The projection's holder becomes a PEFT-shaped layer
        (`lora_A`, `lora_B`, `scaling`, `active_adapters`, `set_scale`) that `enable_lora(list(model.modules()), [...])`
        (src/lora_switching_module.py:11-38) switches; the engines' GEMM launches for that weight take the live adapters as a K-segment of the base
        product (`ug_gemm_desc.lora_T / lora_B`). A / B: None (PEFT's initial values: A uniform, B zero - or B random too with
        init_lora_weights=False, PEFT's testing mode), or {module name: tensor}. Returns the module names that received the adapter.
        No adapter attached -> nothing changes anywhere (bit-identical outputs, same launches)."""
        hits = []
        for name, mod in list(self.named_modules()):
            if not name.startswith(prefix) or not _suffix_match(name, target_suffixes):
                continue
            w = mod._parameters.get("weight")
            if w is None or w.dim() != 2:
                continue
            if not self.lora_capable(name):
                raise L.UniGenHipError(f"add_lora: {name} is not a projection the HIP engine can extend with an adapter K-segment "
                                       f"(supported suffixes: {', '.join(self.LORA_CAPABLE)} inside transformer blocks)")
            hits.append(name)
        if not hits:
            raise ValueError(f"add_lora: no module under prefix {prefix!r} matches {list(target_suffixes)}")
        g = torch.Generator().manual_seed(seed)
        for name in hits:
            mod = self.get_submodule(name)
            if not isinstance(mod, _LoRAHolder):
                mod = _LoRAHolder(mod)
                self._swap_holder(name, mod)
                self._lora_sites[name] = mod
            a = A.get(name) if isinstance(A, dict) else A
            b = B.get(name) if isinstance(B, dict) else B
            if b is None and not init_lora_weights:
                b = torch.randn(mod.weight.shape[0], r, generator=g) * 0.02
            mod.add_adapter(adapter_name, r, lora_alpha, A=a, B=b, generator=g)
        self._pname_cache = None
        self._lora_fused.clear()
        return hits

    def _drop_live_adapter(self, adapter_name: str, only=None) -> None:
        """Remove the adapter's live layers (from the sites named in `only`, or everywhere); a holder left without adapters becomes a plain one again."""
        for name, site in list(self._lora_sites.items()):
            if adapter_name not in site.lora_A or (only is not None and name not in only):
                continue
            site.remove_adapter(adapter_name)
            if not site.lora_A:
                self._swap_holder(name, site.plain())
                del self._lora_sites[name]
        self._pname_cache = None
        self._lora_fused.clear()

    @contextlib.contextmanager
    def _lora_scaled(self, joint_attention_kwargs):
        """`scale_lora_layers(self, lora_scale)` ... `unscale_lora_layers(self, lora_scale)` around a forward (src/UniGenTransformer.py:1200-1208,
        1266-1269; diffusers 0.32.2 utils/peft_utils.py): `joint_attention_kwargs["scale"]` multiplies every adapter's scaling for the duration of
        the forward; 1.0 (or no adapter-carrying projection) is a no-op, 0 is undone by `set_scale(adapter, 1.0)`."""
        w = (joint_attention_kwargs or {}).get("scale", 1.0)
        sites = list(self._lora_sites.values()) if w is not None and w != 1.0 else []
        for m in sites:
            m.scale_layer(w)
        try:
            yield
        finally:
            for m in sites:
                if w != 0:
                    m.unscale_layer(w)
                else:
                    for a in m.active_adapters:
                        m.set_scale(a, 1.0)

    def set_lora_trainable(self, adapters: Optional[Sequence[str]] = None, freeze_rest: bool = True) -> Sequence[str]:
        """Make the `lora_A` / `lora_B` weights of the named adapters (None: every adapter) trainable - the reference's `transformer_lora_parameters`
        (train.py:349). With `freeze_rest` every other parameter is frozen (the base, the control modules, the adapters not named); those adapters
        still take part in the forward while live. The differentiable forward (unigen_amd/training.py) then runs the LoRA-carrying linears of
        unigen_amd/autograd.py. Returns the names of the trainable parameters."""
        known = self.adapter_names(merge_only=False)
        want = known if adapters is None else set(adapters)
        if not want or want - known:
            raise ValueError(f"set_lora_trainable: unknown adapters {sorted(want - known)} (attached: {sorted(known)})" if want else
                             "set_lora_trainable: no adapter is attached (add_lora)")
        if freeze_rest:
            self.requires_grad_(False)
        for a in want:
            for _, A, B, _ in self.lora_entries(a, merge_only=False):
                A.requires_grad_(True)
                B.requires_grad_(True)
        return [n for n, p_ in self.named_parameters() if p_.requires_grad]

    def lora_state_dict(self, adapter: str) -> Dict[str, torch.Tensor]:
        """What PEFT's `get_peft_model_state_dict(model, adapter_name=adapter)` returns and the reference's save hook writes (src/hook.py:29-46):
        `<proj>.lora_A.weight` / `<proj>.lora_B.weight` - the adapter name dropped - for every projection that carries the adapter."""
        sd = {}
        for name, A, B, _ in self.lora_entries(adapter, merge_only=False):
            sd[f"{name}.lora_A.weight"] = A.detach().clone()
            sd[f"{name}.lora_B.weight"] = B.detach().clone()
        if not sd:
            raise KeyError(f"lora_state_dict: no projection carries an adapter named {adapter!r}")
        return sd

    def load_lora_state_dict(self, state_dict: Dict[str, torch.Tensor], adapter: str) -> Sequence[str]:
        """Load the weights of `adapter` (already attached with add_lora: rank and alpha are not part of a state dict). Accepted key forms:
        `<proj>.lora_A.weight` (lora_state_dict / PEFT), the same under a `transformer.` prefix (what `FluxPipeline.lora_state_dict` hands to the
        reference's load hook, src/hook.py:49-70) and the in-model `<proj>.lora_A.<adapter>.weight` (the base weights of a PEFT-wrapped
        checkpoint sit under `<proj>.base_layer.`: INTEGRATION.md). Every projection that carries the adapter must be covered, every key must be used. Returns the loaded keys."""
        want = {f"{n}.lora_{s}": w for n, A, B, _ in self.lora_entries(adapter, merge_only=False) for s, w in (("A", A), ("B", B))}
        if not want:
            raise KeyError(f"load_lora_state_dict: no projection carries an adapter named {adapter!r}")
        used = []
        with torch.no_grad():
            for key, val in state_dict.items():
                k = key[len("transformer."):] if key.startswith("transformer.") else key
                if not k.endswith(".weight"):
                    raise KeyError(f"load_lora_state_dict: unexpected key {key!r}")
                k = k[:-len(".weight")]
                if k.endswith("." + adapter):
                    k = k[:-len(adapter) - 1]
                dst = want.get(k)
                if dst is None or k in used:
                    raise KeyError(f"load_lora_state_dict: {key!r} does not name a lora_A / lora_B weight of adapter {adapter!r}")
                if tuple(val.shape) != tuple(dst.shape):
                    raise ValueError(f"load_lora_state_dict: {key!r} is {tuple(val.shape)}, the adapter's weight is {tuple(dst.shape)}")
                dst.copy_(val.to(dst.device, dst.dtype))
                used.append(k)
        if set(used) != set(want):
            raise KeyError(f"load_lora_state_dict: missing {sorted(set(want) - set(used))[:4]} ...")
        return used

    # ------------------------------------------------------------------ LoRA files and the merge into the base weights ---------------
    def load_lora_weights(self, src, adapter_name: str = "default", strict: bool = True):
        """Read a LoRA file (`src`: a path - unigen_amd/lora_io.py `read_lora_file` - or a state dict in the diffusers / PEFT, kohya or BFL naming),
        infer rank and alpha per module, and attach it as `adapter_name`: the modules in LORA_CAPABLE through `add_lora(..., A=, B=)` - live, switched by
        `enable_lora` as before - the others (AdaLN linears, embedders, experts, proj_out ...) as merge-only entries that reach the output only through
        `fuse_lora()`; until then the forward refuses to run (a partly applied adapter is never computed). Tensors are cast to the model's dtype.
        Module names the model does not have raise under `strict`. Returns lora_io.LoraReport(live, merge_only, ignored)."""
        from . import lora_io
        sd = src if isinstance(src, dict) else lora_io.read_lora_file(src)
        entries, report = lora_io.convert(sd, self, strict=strict)
        if not entries:
            raise ValueError("load_lora_weights: the file holds no adapter weight for this model")
        taken = {n for n, *_ in self.lora_entries(adapter_name)}
        if taken & set(entries):
            raise L.UniGenHipError(f"load_lora_weights: adapter {adapter_name!r} already covers {sorted(taken & set(entries))[:4]} ...; unload_lora_weights first")
        if adapter_name in self._lora_merged:
            raise L.UniGenHipError(f"load_lora_weights: adapter {adapter_name!r} is fused into the weights; unfuse_lora first")
        groups: Dict[Tuple[int, float], list] = {}
        for name in report.live:
            A, B, alpha = entries[name]
            groups.setdefault((A.shape[0], float(alpha if alpha is not None else A.shape[0])), []).append(name)
        # add_lora matches its targets by PEFT's suffix rule: a full module name must not ALSO be the tail of a deeper module's name
        modules = dict(self.named_modules())
        for name in report.live:
            extra = [n for n in modules if n.endswith("." + name) and modules[n]._parameters.get("weight") is not None]
            if extra:
                raise L.UniGenHipError(f"load_lora_weights: {name!r} is also the suffix of {extra[:2]}; the file's entry cannot be attached to one module alone")
        try:
            for (r, alpha), names in groups.items():
                hits = self.add_lora(names, adapter_name, r, alpha, A={n: entries[n][0] for n in names}, B={n: entries[n][1] for n in names})
                if set(hits) != set(names):
                    raise L.UniGenHipError(f"load_lora_weights: add_lora attached {sorted(set(hits) ^ set(names))[:4]} beyond / short of the file's modules")
        except Exception:
            self._drop_live_adapter(adapter_name, only=set(report.live))      # nothing of a file that failed part-way stays attached
            raise
        dev, dt = self.device, self.dtype
        for name in report.merge_only:
            A, B, alpha = entries[name]
            self._lora_merge_only.setdefault(adapter_name, {})[name] = (A.detach().to(dev, dt).contiguous(), B.detach().to(dev, dt).contiguous(),
                                                                        float(alpha if alpha is not None else A.shape[0]))
        return report

    def _lora_guard(self) -> None:
        """Refuse a forward while an adapter has merge-only entries that are not merged: only part of it would be applied."""
        pending = [a for a in self._lora_merge_only if a not in self._lora_merged]
        if pending:
            raise L.UniGenHipError(f"adapter(s) {pending} carry weights for modules outside LORA_CAPABLE (e.g. {next(iter(self._lora_merge_only[pending[0]]))}) that only run "
                                   "merged into the base weights: call fuse_lora() before the forward (or unload_lora_weights)")

    @staticmethod
    @torch.no_grad()
    def _merge_into(w: torch.Tensor, blocks) -> None:
        """w [N_out, K_in] (a view inside its pack) <- dtype(w + Bs A_cat), Bs = dtype(scaling_a * B_a), in place, every adapter of this weight as one
        concatenated rank (adapter_operands over this one projection; blocks: its (A, B, scale)) - w is rounded ONCE. Two existing launches:
        P = Bs A_cat through ug_gemm with the fp32 epilogue (UG_EPI_F32: the accumulators as they are), then w = dtype(w + P) through ug_add_rowbcast_f32. (One UG_EPI_RES_SCALE launch with the residual aliased to the output also
        merges in place, but that epilogue rounds the product to bf16 before it adds the residual; the second rounding moved a fused bf16 forward
        from 0.0089 to 0.0143 off the fp32 oracle: profiles/lora_merge_rounding.log, DESIGN.md section 7a addendum.) A weight the kernels' alignment rules refuse is staged through a
        padded temporary."""
        N, K = w.shape
        A_cat, Bs = adapter_operands([blocks], [N], w.dtype, w.device)
        direct = K % 8 == 0 and w.stride(1) == 1 and w.stride(0) % 8 == 0 and w.data_ptr() % 16 == 0
        Kp = K if direct else (K + 63) // 64 * 64
        dst = w if direct else torch.zeros(N, Kp, device=w.device, dtype=w.dtype)
        if not direct:
            dst[:, :K].copy_(w)
            A_cat = torch.nn.functional.pad(A_cat, (0, Kp - K))
        At = ops.transpose(A_cat)                                            # [K_in, Rp]: the GEMM's W operand, nn.Linear layout over the rank
        P = torch.empty(N, Kp, device=w.device, dtype=torch.float32)
        ops.gemm(Bs, At, None, P, M=N, epilogue=L.EPI_F32)
        ops.add_rowbcast_f32(dst, P, N)
        if not direct:
            w.copy_(dst[:, :K])

    @torch.no_grad()
    def fuse_lora(self, adapter_names: Optional[Sequence[str]] = None, lora_scale: float = 1.0, backup: Optional[str] = "device") -> Sequence[str]:
        """Merge the named adapters (None: every adapter that is not merged yet) into the base weights, live sites and merge-only entries alike:
        W <- dtype(W + sum_a dtype(scaling_a * lora_scale * B_a) A_a), rounded once, in place: one GEMM launch + one add per weight (`_merge_into`; fp32
        models take the fp32 twins).
        Live sites use their CURRENT scaling, merge-only entries alpha / r; a factor of 0 merges nothing. A merged adapter stops contributing at run time
        whatever `enable_lora` or `joint_attention_kwargs["scale"]` say: `live_adapters()` skips it, so the forward's launches are those of the adapter-free model.
        backup: "device" / "host" keep the original bytes of every touched parameter (about 24 GB for an all-linear FLUX adapter) for `unfuse_lora`;
        None keeps none. Merging an adapter twice is an error. Returns the names of the touched parameters."""
        if backup not in ("device", "host", None):
            raise ValueError(f"fuse_lora: backup must be 'device', 'host' or None, got {backup!r}")
        known = self.adapter_names()
        names = [a for a in sorted(known) if a not in self._lora_merged] if adapter_names is None else \
            [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        for a in names:
            if a in self._lora_merged:
                raise L.UniGenHipError(f"fuse_lora: adapter {a!r} is already fused into the weights")
            if a not in known:
                raise KeyError(f"fuse_lora: no adapter named {a!r} (attached: {sorted(known)})")
        if not names:
            raise L.UniGenHipError("fuse_lora: no adapter to fuse")
        if self._lora_merged and (backup is None) != (self._lora_backup is None):
            raise L.UniGenHipError("fuse_lora: adapters are already fused with another backup mode; unfuse_lora first")
        per_weight: Dict[str, list] = {}
        for a in names:
            for mod, A, B, alpha in self.lora_entries(a):
                site = self._lora_sites.get(mod)
                sc = (site.scaling[a] if site is not None and a in site.lora_A else alpha / A.shape[0]) * lora_scale
                if sc != 0.0:
                    per_weight.setdefault(mod, []).append((A, B, sc))
        if backup is not None and self._lora_backup is None:
            self._lora_backup = {}
        touched = []
        for mod, blocks in per_weight.items():
            p = self.get_parameter(mod + ".weight")
            if backup is not None and mod + ".weight" not in self._lora_backup:
                self._lora_backup[mod + ".weight"] = p.data.detach().clone() if backup == "device" else p.data.detach().cpu()
            self._merge_into(p.data, blocks)
            touched.append(p)
        for a in names:
            self._lora_merged[a] = float(lora_scale)
            for site in self._lora_sites.values():
                if a in site.lora_A:
                    site.fused_adapters.add(a)
        self._weights_rewritten(touched)
        return [m + ".weight" for m in per_weight]

    @torch.no_grad()
    def unfuse_lora(self) -> None:
        """Undo every fuse_lora: copy the backed-up bytes back - bit for bit - and let the merged live adapters contribute again. Without a backup
        (`fuse_lora(backup=None)`) this raises: subtracting the product again in bf16 is NOT an inverse of the merge (W was rounded after the
        addition), so there is nothing exact to restore."""
        if not self._lora_merged:
            raise L.UniGenHipError("unfuse_lora: no adapter is fused")
        if self._lora_backup is None:
            raise L.UniGenHipError("unfuse_lora: fuse_lora(backup=None) kept no copy of the original weights, and subtracting the adapters in bf16 does not "
                                   "restore them; reload the base weights instead")
        touched = []
        for name, saved in self._lora_backup.items():
            p = self.get_parameter(name)
            p.data.copy_(saved)
            touched.append(p)
        self._lora_backup = None
        for site in self._lora_sites.values():
            site.fused_adapters.difference_update(self._lora_merged)
        self._lora_merged.clear()
        self._weights_rewritten(touched)

    def unload_lora_weights(self, adapter_name: str) -> None:
        """Remove the adapter: unfuse first if it is merged (every merged adapter is unfused - the backup holds the weights before all of them), then
        drop its live layers (a holder left without adapters becomes a plain one again) and its merge-only entries."""
        known = self.adapter_names()
        if adapter_name not in known:
            raise KeyError(f"unload_lora_weights: no adapter named {adapter_name!r} (attached: {sorted(known)})")
        if adapter_name in self._lora_merged:
            self.unfuse_lora()
        self._lora_merge_only.pop(adapter_name, None)
        self._drop_live_adapter(adapter_name)

    # ------------------------------------------------------------------ the adapters of one launch --------------------
    def _lora_live(self, prefixes: Sequence[str]) -> bool:
        """Does any projection of this launch carry an adapter that contributes right now?"""
        return bool(self._lora_sites) and any(p in self._lora_sites and self._lora_sites[p].live_adapters() for p in prefixes)

    def _lora_layers(self, prefixes: Sequence[str]):       # (layers, widths) of a launch over the row-concatenated weights of `prefixes`
        return [self._lora_sites.get(p) for p in prefixes], [self.get_parameter(p + ".weight").shape[0] for p in prefixes]

    def _lora_operands(self, prefixes: Sequence[str], a: torch.Tensor, M: int, tag: str, lda: Optional[int] = None, a_map: ops.RowMap = ops.IDENT):
        """(T, B) for ONE launch over the row-concatenated weights of `prefixes` (the fused q|k|v[|proj_mlp] launch, or a single projection):
        T = a A_cat^T [M, R] - ONE GEMM for all live adapters of all projections of the launch - and the block-diagonal, scaling-folded B [N, R]
        (fuse_adapters, cached until an adapter's switch state or weights change). (None, None) when no adapter is live: the caller's launch is then
        exactly the adapter-free one."""
        if not self._lora_live(prefixes):
            return None, None
        sites = [self._lora_sites.get(p) for p in prefixes]
        state = tuple((p, tuple((n, s.scaling[n], s.lora_A[n].weight._version, s.lora_B[n].weight._version, s.lora_A[n].weight.data_ptr(),
                                 s.lora_B[n].weight.data_ptr())
                                for n in s.live_adapters())) for p, s in zip(prefixes, sites) if s is not None)
        key = (tuple(prefixes), self.dtype)
        hit = self._lora_fused.get(key)
        if hit is None or hit[0] != state:
            hit = (state,) + fuse_adapters(*self._lora_layers(prefixes), self.dtype, self.device)
            self._lora_fused[key] = hit
        A_cat, B_bd = hit[1], hit[2]
        t = self._w("lora_t_" + tag, (M, A_cat.shape[0]))
        ops.gemm(a, A_cat, None, t, M=M, lda=lda, a_map=a_map)
        return t, B_bd

    def _lora_gemm(self, prefixes: Sequence[str], a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, tag: str, *,
                   M: int, lda: Optional[int] = None, a_map: ops.RowMap = ops.IDENT, **gemm_kw) -> torch.Tensor:
        """ops.gemm(a, w, bias, out, ...) over the row-concatenated weights of `prefixes`, their live adapters riding as the launch's K-segment: the
        T = a A_cat^T GEMM (_lora_operands) reads `a` through the same M / lda / a_map, directly before. No live adapter: the plain launch alone."""
        lt, lb = self._lora_operands(prefixes, a, M, tag, lda=lda, a_map=a_map)
        return ops.gemm(a, w, bias, out, M=M, lda=lda, a_map=a_map, lora_t=lt, lora_b=lb, **gemm_kw)

    def _lora_autograd(self, prefixes: Sequence[str]):
        """_lora_operands for the differentiable forward (unigen_amd/training.py): (A_cat, B_bd, has) of fuse_adapters_autograd, or None - the launch is
        then the adapter-free one: an adapter switched off by `enable_lora(...)` or a scaling of 0 is not live, takes no launch and gets no gradient."""
        if not self._lora_live(prefixes):
            return None
        return fuse_adapters_autograd(*self._lora_layers(prefixes), self.dtype, self.device)


class LoRALinear(nn.Module, LoRALayer):
    """nn.Linear-shaped layer (weight [N, K], bias [N]) with named LoRA adapters, stand-alone (outside a transformer)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=BF):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(out_features, device=device, dtype=dtype), requires_grad=False) if bias else None
        self._init_lora()

    def _fused_adapters(self):
        """Concatenate the live adapters along the rank: A_cat [R, K], B_cat [N, R] with scaling folded into B, R padded to 64."""
        return fuse_adapters([self], [self.out_features], self.weight.dtype, self.weight.device)

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        M = x2.shape[0]
        dt = self.weight.dtype                                            # bf16 (product) or fp32 (verification twins, ug_gemm_f32)
        out = torch.empty(M, self.out_features, device=x.device, dtype=dt)
        A, Bm = self._fused_adapters()
        t = None
        if A is not None:
            t = ops.gemm(x2, A, None, torch.empty(M, A.shape[0], device=x.device, dtype=dt), M=M)      # T = x A^T
        ops.gemm(x2, self.weight, self.bias, out, M=M, lora_t=t, lora_b=Bm)       # base GEMM (+ LoRA K-segment in one accumulator)
        return out.view(*shp[:-1], self.out_features)


def module_active_adapters(module) -> List[str]:
    """src/lora_switching_module.py:4-9."""
    if hasattr(module, "active_adapters"):
        return [i for i in module.active_adapters if i in module.scaling.keys()]
    return []


class enable_lora:
    """src/lora_switching_module.py:11-38: inside the context every active adapter NOT in `enable_adapters` has its scale set to 0."""

    def __init__(self, lora_modules: List[Any], enable_adapters: List) -> None:
        self.lora_modules = [each for each in lora_modules if isinstance(each, LoRALayer)]      # PEFT: isinstance(each, BaseTunerLayer)
        self.active_adapter_scales = [{a: m.scaling[a] for a in module_active_adapters(m)} for m in self.lora_modules]
        self.enable_adapters = enable_adapters

    def __enter__(self) -> None:
        for m in self.lora_modules:
            for a in module_active_adapters(m):
                if a not in self.enable_adapters:
                    m.set_scale(a, 0)

    def __exit__(self, exc_type: Optional[Type[BaseException]], exc_val: Optional[BaseException], exc_tb: Optional[Any]) -> None:
        for i, m in enumerate(self.lora_modules):
            for a in module_active_adapters(m):
                m.set_scale(a, self.active_adapter_scales[i][a])
