"""Sana on the HIP library: diffusers' SanaTransformerBlock and the plain SanaTransformer2DModel around it, diffusers not needed.

Every component of the reference's SANAUniGen (src/UniGenTransformer.py:1453-2112) is a diffusers SanaTransformerBlock; the base transformer here is
steps 1 and 3-5 of SANAUniGen.forward plus the block call of its base_forward. The condition weave of that class is not here (docs/NEXT_ROWS.md).
diffusers is not installed where this is built and its source is not in the reference tree: the arithmetic is restated from the published semantics, and
parity with diffusers is UNPINNED (the tests compare against tests/sana_ref.py, a restatement of the same semantics in plain torch).

One block is
    mod = scale_shift_table[None] + timestep.reshape(B, 6, D)                      ug_add_bf16 (bf16 + bf16 -> bf16, the table broadcast over the batch)
    n1  = LN(h) (1 + scale_msa) + shift_msa                                        ug_adaln_modulate
    q | k | v = n1 [to_q; to_k; to_v]^T                                            ug_gemm_bf16, one packed launch
    a   = relu-linear attention at head width 32                                   ug_linear_attn on the packed buffer (fp32 state, one rounding)
    h   = h + gate_msa * to_out(a)                                                 ug_gemm_bf16, UG_EPI_RES_GATE
    h   = h + to_out2(softmax(q2 k2^T / sqrt(dc)) v2)                              ug_gemm_bf16 x 3, ug_flash_attn_fwd; see "padded heads"
    n2  = LN(h) (1 + scale_mlp) + shift_mlp                                        ug_adaln_modulate
    u   = conv_inverted(n2)   (1x1 convolution = GEMM on the token rows: NHWC is the token layout)
    g   = glu(dwconv3x3(silu(u)))                                                  ug_glu_dwconv3x3, pad columns zeroed for the next GEMM's K
    h   = h + gate_mlp * conv_point(g)                                             ug_gemm_bf16, UG_EPI_RES_GATE
with the reference's bf16 rounding points. Parameters in fp32 run the same orchestration through the `_f32` verification twins.

Padded heads. The cross-attention head widths (112 at Sana-1.6B, 72 at 0.6B) are not widths the flash kernel has. load_state_dict packs attn2's
to_q / to_k / to_v rows head by head into 64- or 128-wide slots, the spare rows zero, and to_out's input columns likewise; the flash kernel runs at the
padded width with the TRUE softmax scale cross_attention_head_dim ** -0.5. Zero rows add nothing to a score and produce zero outputs, which meet zero
columns. THE NAMED PARAMETERS (state_dict()) ARE NOT VIEWS OF THE PACK: after changing one, call load_state_dict again.

Inference by default: a call with autograd recording on an input that requires grad raises. Training is an opt-in on both classes:
    set_trainable(patterns=True)        marks the named parameters that match as leaves that take gradients (True: all; an iterable of fnmatch patterns)
    trainable_parameters()              name -> leaf tensor, for unigen_amd.optim.AdamW
    enable_gradient_checkpointing()     recompute each block in the backward
After set_trainable(), forward on inputs or parameters that require grad runs unigen_amd/training.py's sana_block_forward / sana_forward: the same
kernels on the autograd Functions of unigen_amd/autograd.py (ug_linear_attn_bwd, ug_glu_dwconv3x3_bwd, ug_flash_attn_bwd, the GEMMs). Gradients arrive at
the NAMED parameters; a packed copy is rebuilt, into its own buffer, when a version counter of one of its named tensors has moved (an in-place optimizer
step), so the next forward, training or inference, sees the new values. A load_state_dict() after the opt-in selects the same parameters again.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import lib as L
from . import ops

BF, F32 = torch.bfloat16, torch.float32
FOLLOW_UP = "a follow-up to the Sana base transformer (docs/NEXT_ROWS.md)"


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _no_autograd(*tensors) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("unigen_amd.sana is inference only: there is no backward for the Sana kernels (run under torch.no_grad(), or detach the inputs)")


def sincos_pos_embed(D: int, H: int, W: int, base_size: int, interpolation_scale: float) -> torch.Tensor:
    """diffusers' get_2d_sincos_pos_embed for an [H, W] token grid, float64 [H W, D], built on the host. grid = arange(n) / (n / base_size) /
    interpolation_scale per axis; np.meshgrid takes the WIDTH grid first, so the first half of the channels (diffusers names it emb_h) encodes the x
    coordinate and the second half the y coordinate; each half is [sin | cos] of pos * 10000 ** (-arange(D / 4) / (D / 4)). Token (y, x) is row y W + x."""
    if D % 4:
        raise ValueError(f"sincos_pos_embed: the width {D} is not a multiple of 4")
    gy = torch.arange(H, dtype=torch.float64) / (H / base_size) / interpolation_scale
    gx = torch.arange(W, dtype=torch.float64) / (W / base_size) / interpolation_scale
    omega = 10000.0 ** (-torch.arange(D // 4, dtype=torch.float64) / (D / 4))

    def one(pos):
        a = pos[:, None] * omega[None, :]
        return torch.cat([a.sin(), a.cos()], 1)
    return torch.cat([one(gx[None, :].expand(H, W).reshape(-1)), one(gy[:, None].expand(H, W).reshape(-1))], 1)


def mask_runs(mask: Optional[torch.Tensor], B: int, T: int) -> List[Tuple[int, int, int]]:
    """encoder_attention_mask -> [(first sample, samples, keys)]: consecutive samples with the same number of live keys share one flash launch.
    None or all ones: one run over everything. Rows must be prefixes (ones, then zeros) with at least one live key."""
    if mask is None:
        return [(0, B, T)]
    if mask.dim() != 2 or tuple(mask.shape) != (B, T):
        raise NotImplementedError(f"encoder_attention_mask of shape {tuple(mask.shape)}: only None or a 2-D [batch, tokens] = [{B}, {T}] mask is implemented; "
                                  f"additive biases and per-query masks are {FOLLOW_UP}")
    m = mask.detach().to("cpu")
    live = m != 0
    if not bool(((m == 0) | (m == 1)).all()):
        raise NotImplementedError(f"encoder_attention_mask with values other than 0 and 1 is not implemented; additive biases are {FOLLOW_UP}")
    lengths = live.sum(1)
    prefix = torch.arange(T)[None, :] < lengths[:, None]
    if not bool((live == prefix).all()):
        raise NotImplementedError("encoder_attention_mask: every row must be a prefix mask (ones, then zeros); masks with holes are " + FOLLOW_UP)
    if int(lengths.min()) < 1:
        raise ValueError("encoder_attention_mask: a sample without a single live text token has no softmax")
    runs: List[Tuple[int, int, int]] = []
    for b, n in enumerate(lengths.tolist()):
        if runs and runs[-1][2] == n:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1, n)
        else:
            runs.append((b, 1, n))
    return runs


class _Params:
    """Named parameters in a dict, with diffusers' keys; subclasses list them in expected_keys() and build their load-time layouts in _pack()."""

    def __init__(self, device, dtype):
        if dtype not in (BF, F32):
            raise TypeError(f"{type(self).__name__} computes in torch.bfloat16 (or torch.float32 for verification)")
        self._device, self._dtype = torch.device(device) if device is not None else torch.device("cpu"), dtype
        self._sd: Dict[str, torch.Tensor] = {}
        self._buf: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self._trainable_on = False                       # set_trainable() was called: forward may take the differentiable path
        self._grad_checkpoint = False
        self._patterns = None                            # what set_trainable() was last given (re-applied by a later load_state_dict)
        self._owned = False                              # a block of a model: the model's set_trainable() hands it its leaf tensors
        self._pv: Dict[str, tuple] = {}                  # packed copy -> its sources' version counters when it was built

    dtype = property(lambda self: self._dtype)
    device = property(lambda self: self._device)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        exp = self.expected_keys()
        unexpected = [k for k in sd if k not in exp]
        missing = sorted(set(exp) - set(sd))
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {unexpected[:4]}")
        for k, shape in exp.items():
            if k in sd:
                if tuple(sd[k].shape) != shape:
                    raise ValueError(f"{k}: shape {tuple(sd[k].shape)} does not match {shape}")
                self._sd[k] = sd[k].detach().to(device=self._device, dtype=self._dtype).contiguous()
        if not missing:
            self._pack()
            if self._trainable_on and not self._owned:   # the leaves were replaced: select them again (a model re-shares them with its blocks)
                self.set_trainable(self._patterns)
        return missing, unexpected

    def init_synthetic_(self, seed: int = 0):
        """Seeded random weights for tests and benchmarks: weights N(0, 1 / fan_in), biases and modulation tables 0.1 N, norm weights 1 + 0.1 N."""
        g = torch.Generator(device=self._device).manual_seed(seed)            # drawn on the model's device
        sd = {}
        for k, shape in self.expected_keys().items():
            t = torch.randn(shape, generator=g, device=self._device)
            if k.endswith("caption_norm.weight"):
                t = 1 + 0.1 * t
            elif k.endswith(".bias") or k.endswith("scale_shift_table"):
                t = 0.1 * t
            else:
                t = t / math.sqrt(max(1, t[0].numel()))
            sd[k] = t.to(self._dtype)
        self.load_state_dict(sd)
        return self

    # ---- training opt-in ----
    def set_trainable(self, patterns=True):
        """Opt in to the differentiable forward. patterns: True - every named parameter takes gradients; False / None / () - none does (gradients
        still reach the inputs); else an iterable of fnmatch patterns over the state-dict keys ("transformer_blocks.1.*", "*.attn2.to_q.weight")."""
        import fnmatch
        if not self._p:
            raise RuntimeError(f"{type(self).__name__}: load_state_dict first")
        pats = [patterns] if isinstance(patterns, str) else (None if patterns is True else list(patterns or ()))
        for k, t in self._sd.items():
            t.requires_grad_(pats is None or any(fnmatch.fnmatchcase(k, p) for p in pats))
            if not t.requires_grad:
                t.grad = None
        self._trainable_on, self._patterns = True, patterns
        self._share_leaves()
        return self

    def trainable_parameters(self) -> Dict[str, torch.Tensor]:
        """name -> leaf tensor of every parameter set_trainable() selected (their .grad is filled by backward())"""
        return {k: t for k, t in self._sd.items() if t.requires_grad}

    def enable_gradient_checkpointing(self):
        """recompute each block in the backward instead of keeping its activations (torch.utils.checkpoint around the block)"""
        self._grad_checkpoint = True

    def disable_gradient_checkpointing(self):
        self._grad_checkpoint = False

    def _share_leaves(self) -> None:
        pass

    def _builders(self) -> Dict[str, tuple]:
        """packed copy -> (the named tensors it is built from, a function that builds it); no sources: a view of a named tensor, always current"""
        raise NotImplementedError

    def _pack(self) -> None:
        with torch.no_grad():
            b = self._builders()
            self._p = {n: build() for n, (_, build) in b.items()}
        self._pv = {n: tuple(self._sd[k]._version for k in srcs) for n, (srcs, _) in b.items()}

    def _sync(self, training: bool = False) -> None:
        """After the opt-in the named tensors may change in place (an optimizer step) and the packed copies are not views of them. A copy whose
        sources' version counters have moved is rebuilt INTO ITS BUFFER (no new storage), and the transposes autograd cached of it are dropped.
        Copies of frozen parameters never move, so their cached transposes stay. The differentiable path (training=True) reads a copy only where a
        source is frozen, so it skips the copies of trainable parameters: those are brought up to date by the next inference forward.
        Before the opt-in this is one attribute test."""
        if not self._trainable_on:
            return
        for n, (srcs, build) in self._builders().items():
            if not srcs or self._p.get(n) is None or (training and all(self._sd[k].requires_grad for k in srcs)):
                continue
            v = tuple(self._sd[k]._version for k in srcs)
            if v != self._pv.get(n):
                from . import autograd
                with torch.no_grad():
                    self._p[n].copy_(build())
                autograd.evict_weight(self._p[n])
                self._pv[n] = v

    def _wants_grad(self, *tensors) -> bool:
        return self._trainable_on and torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors) or
                                                                   any(t.requires_grad for t in self._sd.values()))

    def _buffers(self, key: tuple) -> Dict[str, torch.Tensor]:
        """the activations and workspaces of one input shape: allocated at the first call with that shape, reused afterwards"""
        b = self._buf.get(key)
        if b is None:
            if len(self._buf) >= 8:
                self._buf.clear()
            b = self._buf[key] = {}
        return b

    def _get(self, bufs: Dict[str, torch.Tensor], name: str, shape, dtype=None) -> torch.Tensor:
        t = bufs.get(name)
        if t is None:
            t = bufs[name] = torch.empty(*shape, dtype=dtype or self._dtype, device=self._device)
        return t


class SanaTransformerBlock(_Params):
    """diffusers' SanaTransformerBlock: its constructor arguments, its state-dict keys, its forward. See the module docstring for the kernels, the padded
    cross-attention heads (the named parameters are not views of the packed copies) and the limits."""

    def __init__(self, dim: int = 2240, num_attention_heads: int = 70, attention_head_dim: int = 32, dropout: float = 0.0,
                 num_cross_attention_heads: Optional[int] = 20, cross_attention_head_dim: Optional[int] = 112, cross_attention_dim: Optional[int] = 2240,
                 attention_bias: bool = True, norm_elementwise_affine: bool = False, norm_eps: float = 1e-6, attention_out_bias: bool = True,
                 mlp_ratio: float = 2.5, qk_norm: Optional[str] = None, device=None, dtype=BF):
        super().__init__(device, dtype)
        if qk_norm is not None:
            raise NotImplementedError(f"SanaTransformerBlock: qk_norm = {qk_norm!r} is not implemented (Sana 1.5's rms_norm_across_heads is {FOLLOW_UP})")
        if dropout != 0:
            raise NotImplementedError(f"SanaTransformerBlock: dropout = {dropout} is not implemented (dropout in training is {FOLLOW_UP})")
        if norm_elementwise_affine or not attention_out_bias:
            raise NotImplementedError(f"SanaTransformerBlock: norm_elementwise_affine = True / attention_out_bias = False are not implemented ({FOLLOW_UP})")
        if attention_head_dim != 32 or num_attention_heads * attention_head_dim != dim:
            raise NotImplementedError(f"SanaTransformerBlock: {num_attention_heads} heads of {attention_head_dim} at dim {dim}: the linear attention "
                                      "kernel has head width 32, and diffusers' block needs heads x width = dim")
        if cross_attention_dim is None or not num_cross_attention_heads or not cross_attention_head_dim:
            raise NotImplementedError(f"SanaTransformerBlock: a block without cross attention is not implemented ({FOLLOW_UP})")
        if cross_attention_head_dim > 128 or cross_attention_head_dim % 8:
            raise NotImplementedError(f"SanaTransformerBlock: cross_attention_head_dim = {cross_attention_head_dim}: multiples of 8 up to 128 are implemented")
        if dim % 64 or cross_attention_dim % 64:
            raise NotImplementedError("SanaTransformerBlock: dim and cross_attention_dim must be multiples of 64 (the GEMM's K granularity)")
        self.dim, self.heads, self.norm_eps, self.attention_bias = dim, num_attention_heads, float(norm_eps), bool(attention_bias)
        self.cross_heads, self.cross_dh, self.cross_dim = num_cross_attention_heads, cross_attention_head_dim, cross_attention_dim
        self.cross_dp = 64 if cross_attention_head_dim <= 64 else 128          # the slot a cross head is packed into
        self.C = int(mlp_ratio * dim)                                          # GLUMBConv's hidden_channels
        if self.C % 8:
            raise NotImplementedError(f"SanaTransformerBlock: int(mlp_ratio * dim) = {self.C} is not a multiple of 8")
        self.Cp = _pad(self.C, 64)
        self._p: Dict[str, torch.Tensor] = {}
        self._runs: List[tuple] = []                                           # (mask tensor, its version, runs): see _mask_runs

    def expected_keys(self) -> Dict[str, Tuple[int, ...]]:
        D, C, I2, Dc = self.dim, self.C, self.cross_heads * self.cross_dh, self.cross_dim
        e: Dict[str, Tuple[int, ...]] = {"scale_shift_table": (6, D)}
        for n in ("to_q", "to_k", "to_v"):
            e[f"attn1.{n}.weight"] = (D, D)
            if self.attention_bias:
                e[f"attn1.{n}.bias"] = (D,)
        e["attn1.to_out.0.weight"], e["attn1.to_out.0.bias"] = (D, D), (D,)
        e["attn2.to_q.weight"], e["attn2.to_q.bias"] = (I2, D), (I2,)
        for n in ("to_k", "to_v"):
            e[f"attn2.{n}.weight"], e[f"attn2.{n}.bias"] = (I2, Dc), (I2,)
        e["attn2.to_out.0.weight"], e["attn2.to_out.0.bias"] = (D, I2), (D,)
        e["ff.conv_inverted.weight"], e["ff.conv_inverted.bias"] = (2 * C, D, 1, 1), (2 * C,)
        e["ff.conv_depth.weight"], e["ff.conv_depth.bias"] = (2 * C, 1, 3, 3), (2 * C,)
        e["ff.conv_point.weight"] = (D, C, 1, 1)
        return e

    def _builders(self) -> Dict[str, tuple]:
        s = self._sd
        D, C, Cp, Hc, dc, dp = self.dim, self.C, self.Cp, self.cross_heads, self.cross_dh, self.cross_dp
        z = lambda *shape: torch.zeros(*shape, dtype=self._dtype, device=self._device)
        qkv = ("to_q", "to_k", "to_v")

        def slots_w(w):                                  # [Hc dc, K] -> [Hc dp, K], zero rows behind each head
            out = z(Hc, dp, w.shape[1])
            out[:, :dc] = w.reshape(Hc, dc, -1)
            return out.reshape(Hc * dp, -1)

        def slots_b(b):
            out = z(Hc, dp)
            out[:, :dc] = b.reshape(Hc, dc)
            return out.reshape(-1)

        def o2():
            out = z(D, Hc, dp)
            out[:, :, :dc] = s["attn2.to_out.0.weight"].reshape(D, Hc, dc)
            return out.reshape(D, Hc * dp)

        def pt():
            out = z(D, Cp)
            out[:, :C] = s["ff.conv_point.weight"].reshape(D, C)
            return out
        wn, bn = [f"attn1.{n}.weight" for n in qkv], [f"attn1.{n}.bias" for n in qkv]
        return {
            "table": ([], lambda: s["scale_shift_table"].reshape(1, 6 * D)),                        # a view
            "qkv_w": (wn, lambda: torch.cat([s[k] for k in wn], 0).contiguous()),
            "qkv_b": (bn if self.attention_bias else [], lambda: torch.cat([s[k] for k in bn], 0).contiguous() if self.attention_bias else None),
            "q2_w": (["attn2.to_q.weight"], lambda: slots_w(s["attn2.to_q.weight"])),
            "q2_b": (["attn2.to_q.bias"], lambda: slots_b(s["attn2.to_q.bias"])),
            "kv2_w": (["attn2.to_k.weight", "attn2.to_v.weight"], lambda: torch.cat([slots_w(s["attn2.to_k.weight"]), slots_w(s["attn2.to_v.weight"])], 0)),
            "kv2_b": (["attn2.to_k.bias", "attn2.to_v.bias"], lambda: torch.cat([slots_b(s["attn2.to_k.bias"]), slots_b(s["attn2.to_v.bias"])], 0)),
            "o2_w": (["attn2.to_out.0.weight"], o2),
            "inv_w": ([], lambda: s["ff.conv_inverted.weight"].reshape(2 * C, D)),              # a view
            "dw_w": (["ff.conv_depth.weight"], lambda: s["ff.conv_depth.weight"].reshape(2 * C, 9).t().contiguous()),     # [9][2C], tap ky 3 + kx major
            "pt_w": (["ff.conv_point.weight"], pt),
        }

    def _mask_runs(self, mask: Optional[torch.Tensor], B: int, T: int):
        """mask_runs() of a mask, read on the host once per mask tensor. An entry holds the tensor ITSELF and its version counter: an address is no
        identity (the allocator hands a freed mask's address to the next mask of that shape), and holding the tensor keeps the address taken."""
        if mask is None:
            return [(0, B, T)]
        for m, version, runs in self._runs:
            if m is mask and version == mask._version:
                return runs
        runs = mask_runs(mask, B, T)
        self._runs = [e for e in self._runs if e[0] is not mask][-3:] + [(mask, mask._version, runs)]     # the last four masks
        return runs

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, encoder_hidden_states: Optional[torch.Tensor] = None,
                encoder_attention_mask: Optional[torch.Tensor] = None, timestep: Optional[torch.Tensor] = None, height: Optional[int] = None,
                width: Optional[int] = None, out: Optional[torch.Tensor] = None, _runs=None, _bufs=None) -> torch.Tensor:
        """hidden_states [B, N, D], encoder_hidden_states [B, T, cross_attention_dim], timestep [B, 6 D], N = height x width -> [B, N, D].
        encoder_attention_mask: None, or a 2-D [B, T] mask of ones and zeros whose rows are prefixes."""
        if attention_mask is not None:
            raise NotImplementedError(f"SanaTransformerBlock: attention_mask is not implemented (the linear attention takes none; it is {FOLLOW_UP})")
        if encoder_hidden_states is None or timestep is None or height is None or width is None:
            raise ValueError("SanaTransformerBlock.forward needs encoder_hidden_states, timestep, height and width")
        if not self._p:
            raise RuntimeError("SanaTransformerBlock: load_state_dict first")
        train = self._wants_grad(hidden_states, encoder_hidden_states, timestep)
        if not train:
            _no_autograd(hidden_states, encoder_hidden_states, timestep)
        if _bufs is None:                                # (a model has brought its blocks up to date)
            self._sync(train)
        dt, D, H1 = self._dtype, self.dim, self.heads
        B, N, _ = hidden_states.shape
        T = encoder_hidden_states.shape[1]
        if hidden_states.shape[2] != D or N != height * width or tuple(timestep.shape) != (B, 6 * D) or \
                tuple(encoder_hidden_states.shape) != (B, T, self.cross_dim):
            raise ValueError(f"SanaTransformerBlock.forward: shapes {tuple(hidden_states.shape)}, {tuple(encoder_hidden_states.shape)}, "
                             f"{tuple(timestep.shape)} with height x width = {height} x {width}")
        for t, n in ((hidden_states, "hidden_states"), (encoder_hidden_states, "encoder_hidden_states"), (timestep, "timestep")):
            if t.dtype != dt or not t.is_contiguous():
                raise TypeError(f"SanaTransformerBlock.forward: {n} must be a contiguous {dt} tensor")
        runs = _runs if _runs is not None else self._mask_runs(encoder_attention_mask, B, T)
        if train:
            from . import training
            return training._sana_ckpt(self, lambda h_, e_, t_: training.sana_block_forward(self, h_, e_, t_, height, width, runs), hidden_states,
                                       encoder_hidden_states, timestep)
        p, M = self._p, B * N
        Hc, dp, C, Cp = self.cross_heads, self.cross_dp, self.C, self.Cp
        W2 = Hc * dp
        bufs = _bufs if _bufs is not None else self._buffers((B, N, T))       # the model hands all its blocks one set
        g = lambda name, *shape, **kw: self._get(bufs, name, shape, **kw)
        h0 = hidden_states.view(M, D)
        mod = g("blk_mod", B, 6 * D)
        ops._call("ug_add_bf16", dt, timestep.data_ptr(), 6 * D, p["table"].data_ptr(), 0, mod.data_ptr(), 6 * D, B, 6 * D, ops._stream())
        chunk = lambda i: mod[0, i * D:]                 # base of modulation chunk i: sample b's row is 6 D further per sample
        # --- self attention: ReLU linear attention ---
        n1 = ops.adaln_modulate(h0, chunk(0), chunk(1), g("n", M, D), rows=M, D=D, rows_per_sample=N, mod_ld=6 * D, eps=self.norm_eps)
        qkv = ops.gemm(n1, p["qkv_w"], p["qkv_b"], g("qkv", M, 3 * D), M=M)
        s3 = (3 * D, N * 3 * D)
        ws = g("la_ws", ops.linear_attn_workspace_bytes(B, H1, N), dtype=torch.uint8)
        att = ops.linear_attn(qkv, qkv[:, D:], qkv[:, 2 * D:], g("att", M, D), batches=B, heads=H1, N=N, q_strides=s3, k_strides=s3, v_strides=s3,
                              o_strides=(D, N * D), workspace=ws)
        h1 = ops.gemm(att, self._sd["attn1.to_out.0.weight"], self._sd["attn1.to_out.0.bias"], g("h1", M, D), M=M, epilogue=L.EPI_RES_GATE, residual=h0,
                      gate=chunk(2), gate_ld=6 * D, rows_per_sample=N)
        # --- cross attention at the padded head width, the true scale ---
        q2 = ops.gemm(h1, p["q2_w"], p["q2_b"], g("q2", M, W2), M=M)
        kv2 = ops.gemm(encoder_hidden_states.view(B * T, self.cross_dim), p["kv2_w"], p["kv2_b"], g("kv2", B * T, 2 * W2), M=B * T)
        a2 = g("a2", M, W2)
        for b0, nb, keys in runs:
            ops.flash_attn(q2[b0 * N:], kv2[b0 * T:], kv2[b0 * T:, W2:], a2[b0 * N:], batches=nb, heads=Hc, dh=dp, Lq=N, Lkv=keys,
                           q_strides=(W2, N * W2), k_strides=(2 * W2, T * 2 * W2), v_strides=(2 * W2, T * 2 * W2), o_strides=(W2, N * W2),
                           scale=self.cross_dh ** -0.5)
        h2 = ops.gemm(a2, p["o2_w"], self._sd["attn2.to_out.0.bias"], g("h2", M, D), M=M, epilogue=L.EPI_RES_SCALE, residual=h1, alpha=1.0)
        # --- Mix-FFN ---
        n2 = ops.adaln_modulate(h2, chunk(3), chunk(4), g("n", M, D), rows=M, D=D, rows_per_sample=N, mod_ld=6 * D, eps=self.norm_eps)
        u = ops.gemm(n2, p["inv_w"], self._sd["ff.conv_inverted.bias"], g("u", M, 2 * C), M=M)
        glu = ops.glu_dwconv3x3(u, p["dw_w"], self._sd["ff.conv_depth.bias"], g("glu", M, Cp), B=B, H=height, W=width, C=C)
        res = out.view(M, D) if out is not None else torch.empty(M, D, dtype=dt, device=self._device)
        ops.gemm(glu, p["pt_w"], None, res, M=M, epilogue=L.EPI_RES_GATE, residual=h2, gate=chunk(5), gate_ld=6 * D, rows_per_sample=N)
        return res.view(B, N, D)

    __call__ = forward


class SanaTransformer2DModel(_Params):
    """diffusers' SanaTransformer2DModel without the condition weave: config names, state-dict keys and forward of the published class.
    forward(hidden_states [B, C, H, W], encoder_hidden_states [B, T, caption_channels], timestep [B], encoder_attention_mask=None) -> [B, out_channels, H, W]."""

    CONFIG = dict(in_channels=32, out_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                  cross_attention_head_dim=112, cross_attention_dim=2240, caption_channels=2304, mlp_ratio=2.5, dropout=0.0, attention_bias=False,
                  sample_size=32, patch_size=1, norm_elementwise_affine=False, norm_eps=1e-6, interpolation_scale=None, qk_norm=None,
                  guidance_embeds=False, use_rope=False)

    def __init__(self, config: Optional[dict] = None, device=None, dtype=BF, **kw):
        super().__init__(device, dtype)
        c = dict(self.CONFIG)
        given = dict(config or {})
        given.update(kw)
        # diffusers writes its own bookkeeping keys ("_class_name", ...) into config.json; guidance_embeds_scale only acts with guidance_embeds
        unknown = sorted(k for k in given if k not in c and not k.startswith("_") and k not in ("guidance_embeds_scale", "timestep_scale"))
        if unknown:
            raise ValueError(f"SanaTransformer2DModel: config keys {unknown} are not known to this class; nothing is ignored silently")
        if float(given.get("timestep_scale", 1.0)) != 1.0:
            raise NotImplementedError(f"SanaTransformer2DModel: timestep_scale = {given['timestep_scale']} (Sana-Sprint) is not implemented; it is {FOLLOW_UP}")
        c.update({k: v for k, v in given.items() if k in c})
        if c["out_channels"] is None:
            c["out_channels"] = c["in_channels"]
        if c["guidance_embeds"]:
            raise NotImplementedError(f"SanaTransformer2DModel: guidance_embeds = True (Sana-Sprint) is not implemented; it is {FOLLOW_UP}")
        if c["use_rope"]:
            raise NotImplementedError(f"SanaTransformer2DModel: use_rope = True is not implemented (the reference defines no SanaRoPETransformerBlock); it is {FOLLOW_UP}")
        if c["patch_size"] != 1:
            raise NotImplementedError(f"SanaTransformer2DModel: patch_size = {c['patch_size']} is not implemented (every published Sana uses 1); it is {FOLLOW_UP}")
        self.config = c
        D = self.D = c["num_attention_heads"] * c["attention_head_dim"]
        if c["cross_attention_dim"] != D:
            raise ValueError(f"SanaTransformer2DModel: cross_attention_dim = {c['cross_attention_dim']} must equal the inner width {D} (caption_projection's output)")
        if c["caption_channels"] % 64:
            raise NotImplementedError("SanaTransformer2DModel: caption_channels must be a multiple of 64 (the GEMM's K granularity)")
        self.blocks = [SanaTransformerBlock(D, c["num_attention_heads"], c["attention_head_dim"], c["dropout"], c["num_cross_attention_heads"],
                                            c["cross_attention_head_dim"], c["cross_attention_dim"], c["attention_bias"], c["norm_elementwise_affine"],
                                            c["norm_eps"], True, c["mlp_ratio"], c["qk_norm"], device=device, dtype=dtype) for _ in range(c["num_layers"])]
        self.Kin = _pad(c["in_channels"], 64)
        self.Pout = _pad(c["out_channels"], 8)
        self._p: Dict[str, torch.Tensor] = {}
        self._pos: Dict[Tuple[int, int], torch.Tensor] = {}

    def expected_keys(self) -> Dict[str, Tuple[int, ...]]:
        c, D = self.config, self.D
        e: Dict[str, Tuple[int, ...]] = {"patch_embed.proj.weight": (D, c["in_channels"], 1, 1), "patch_embed.proj.bias": (D,)}

        def lin(p, o, i):
            e[p + ".weight"], e[p + ".bias"] = (o, i), (o,)
        lin("time_embed.emb.timestep_embedder.linear_1", D, 256)
        lin("time_embed.emb.timestep_embedder.linear_2", D, D)
        lin("time_embed.linear", 6 * D, D)
        lin("caption_projection.linear_1", D, c["caption_channels"])
        lin("caption_projection.linear_2", D, D)
        e["caption_norm.weight"] = (D,)
        for i, b in enumerate(self.blocks):
            for k, s in b.expected_keys().items():
                e[f"transformer_blocks.{i}.{k}"] = s
        e["scale_shift_table"] = (2, D)
        lin("proj_out", c["out_channels"], D)
        return e

    def _pack(self) -> None:
        for i, b in enumerate(self.blocks):
            pre = f"transformer_blocks.{i}."
            b.load_state_dict({k[len(pre):]: v for k, v in self._sd.items() if k.startswith(pre)})
        super()._pack()
        self._pos.clear()

    def _share_leaves(self) -> None:
        """the blocks hold aliases of the model's tensors (load_state_dict detaches): hand them the leaf objects themselves, so that a block's
        gradient arrives at the tensor trainable_parameters() returns (same storage and version counter: the blocks' packed copies stay valid)"""
        for i, b in enumerate(self.blocks):
            pre = f"transformer_blocks.{i}."
            for k, t in self._sd.items():
                if k.startswith(pre):
                    b._sd[k[len(pre):]] = t
            b._trainable_on = b._owned = True

    def _sync(self, training: bool = False) -> None:
        if self._trainable_on:
            super()._sync(training)
            for b in self.blocks:                        # each block looks at its own copies
                b._sync(training)

    def _builders(self) -> Dict[str, tuple]:
        c, D, s = self.config, self.D, self._sd
        z = lambda *shape: torch.zeros(*shape, dtype=self._dtype, device=self._device)
        oc = c["out_channels"]

        def rows(name, n):                               # proj_out's weight / bias, zero rows up to n
            out = z(n, *s[name].shape[1:])
            out[:oc] = s[name]
            return out

        def patch():
            w = z(D, self.Kin)
            w[:, :c["in_channels"]] = s["patch_embed.proj.weight"].reshape(D, -1)
            return w
        return {"patch_w": (["patch_embed.proj.weight"], patch),
                "out_w": (["proj_out.weight"], lambda: rows("proj_out.weight", self.Pout)), "out_b": (["proj_out.bias"], lambda: rows("proj_out.bias", self.Pout)),
                # the differentiable path: out_features is the contraction length of dX = dY W, a multiple of 64
                "out_w64": (["proj_out.weight"], lambda: rows("proj_out.weight", _pad(oc, 64))), "out_b64": (["proj_out.bias"], lambda: rows("proj_out.bias", _pad(oc, 64)))}

    def position_table(self, H: int, W: int) -> Optional[torch.Tensor]:
        """fp32 [H W, D] on the device, built once per (H, W) on the host in float64; None when interpolation_scale is None (no table is added)"""
        c = self.config
        if c["interpolation_scale"] is None:
            return None
        t = self._pos.get((H, W))
        if t is None:
            if len(self._pos) >= 16:
                self._pos.clear()
            t = sincos_pos_embed(self.D, H, W, c["sample_size"] // c["patch_size"], c["interpolation_scale"]).to(F32).to(self._device).contiguous()
            self._pos[(H, W)] = t
        return t

    @classmethod
    def from_pretrained(cls, path, device=None, dtype=BF) -> "SanaTransformer2DModel":
        """A local directory only (no hub access): config.json + diffusion_pytorch_model.safetensors, or the sharded form with its index file."""
        path = os.fspath(path)
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local directory (this package does not download checkpoints)")
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        from safetensors.torch import load_file
        m = cls(cfg, device=device, dtype=dtype)
        single = os.path.join(path, "diffusion_pytorch_model.safetensors")
        if os.path.exists(single):
            sd = load_file(single)
        else:
            with open(os.path.join(path, "diffusion_pytorch_model.safetensors.index.json")) as f:
                shards = sorted(set(json.load(f)["weight_map"].values()))
            sd = {}
            for sh in shards:
                sd.update(load_file(os.path.join(path, sh)))
        m.load_state_dict(sd)
        return m

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, timestep: torch.Tensor,
                encoder_attention_mask: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if attention_mask is not None:
            raise NotImplementedError(f"SanaTransformer2DModel: attention_mask is not implemented (the linear attention takes none; it is {FOLLOW_UP})")
        if not self._p:
            raise RuntimeError("SanaTransformer2DModel: load_state_dict first")
        train = self._wants_grad(hidden_states, encoder_hidden_states, timestep)
        if not train:
            _no_autograd(hidden_states, encoder_hidden_states, timestep)
        self._sync(train)
        c, D, dt, s, p = self.config, self.D, self._dtype, self._sd, self._p
        B, Cin, H, W = hidden_states.shape
        T = encoder_hidden_states.shape[1]
        if Cin != c["in_channels"] or tuple(encoder_hidden_states.shape) != (B, T, c["caption_channels"]) or timestep.numel() != B:
            raise ValueError(f"SanaTransformer2DModel.forward: shapes {tuple(hidden_states.shape)}, {tuple(encoder_hidden_states.shape)}, {tuple(timestep.shape)}")
        if hidden_states.dtype != dt or encoder_hidden_states.dtype != dt:
            raise TypeError(f"SanaTransformer2DModel.forward: hidden_states and encoder_hidden_states must be {dt}")
        if train:
            from . import training
            return training.sana_forward(self, hidden_states, encoder_hidden_states, timestep, encoder_attention_mask)
        N, M = H * W, B * H * W
        runs = self.blocks[0]._mask_runs(encoder_attention_mask, B, T) if self.blocks else None
        bufs = self._buffers((B, H, W, T))
        g = lambda name, *shape, **kw: self._get(bufs, name, shape, **kw)
        # patch embedding: patch_size 1 is a linear on the pixels, K = in_channels zero-padded to 64; then the position table (fp32 add, one rounding)
        x = ops.nchw_to_nhwc(hidden_states.contiguous(), self.Kin)
        h = ops.gemm(x.view(M, self.Kin), p["patch_w"], s["patch_embed.proj.bias"], g("h_a", M, D), M=M)
        pos = self.position_table(H, W)
        if pos is not None:
            ops.add_rowbcast_f32(h, pos, N)
        # AdaLayerNormSingle
        tp = ops.timestep_embed(timestep.reshape(B).to(device=self._device, dtype=F32), g("tproj", B, 256))
        e1 = ops.small_linear(tp, s["time_embed.emb.timestep_embedder.linear_1.weight"], s["time_embed.emb.timestep_embedder.linear_1.bias"], g("e1", B, D))
        et = ops.small_linear(e1, s["time_embed.emb.timestep_embedder.linear_2.weight"], s["time_embed.emb.timestep_embedder.linear_2.bias"], g("et", B, D),
                              silu_in=True)
        mod = ops.small_linear(et, s["time_embed.linear.weight"], s["time_embed.linear.bias"], g("mod6", B, 6 * D), silu_in=True)
        # caption projection (linear, GELU-tanh, linear) and RMSNorm
        enc = encoder_hidden_states.contiguous().view(B * T, c["caption_channels"])
        c1 = ops.gemm(enc, s["caption_projection.linear_1.weight"], s["caption_projection.linear_1.bias"], g("c1", B * T, D), M=B * T, epilogue=L.EPI_BIAS_GELU)
        c2 = ops.gemm(c1, s["caption_projection.linear_2.weight"], s["caption_projection.linear_2.bias"], g("c2", B * T, D), M=B * T)
        cn = ops.rmsnorm_rows(c2, s["caption_norm.weight"], 1e-5, out=g("cn", B * T, D)).view(B, T, D)
        hb, other = h.view(B, N, D), g("h_b", M, D).view(B, N, D)
        for blk in self.blocks:
            blk.forward(hb, None, cn, encoder_attention_mask, mod, H, W, out=other, _runs=runs, _bufs=bufs)
            hb, other = other, hb
        # SanaModulatedNorm: (scale_shift_table[None] + embedded_timestep[:, None]).chunk(2, 1) = shift, scale
        fm = g("fmod", B, 2 * D)
        for i in range(2):
            ops._call("ug_add_bf16", dt, et.data_ptr(), D, s["scale_shift_table"][i].data_ptr(), 0, fm[:, i * D:].data_ptr(), 2 * D, B, D, ops._stream())
        nf = ops.adaln_modulate(hb.view(M, D), fm[0], fm[0, D:], g("nf", M, D), rows=M, D=D, rows_per_sample=N, mod_ld=2 * D, eps=c["norm_eps"])
        y = ops.gemm(nf, p["out_w"], p["out_b"], g("y", M, self.Pout), M=M)
        return ops.nhwc_to_nchw(y, B, c["out_channels"], H, W)          # unpatchify at patch_size 1: NHWC -> NCHW

    __call__ = forward
