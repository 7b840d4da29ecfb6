"""Depth condition on the HIP library: transformers' DepthAnythingForDepthEstimation (DINOv2 backbone, DPT neck and head), DPTImageProcessor and
the depth-estimation pipeline's post-processing, none of those packages needed.

The reference builds its "depth" condition (type 0 of condition_dict) with `pipeline("depth-estimation", "LiheYoung/depth-anything-small-hf")`
(src/condition.py:52-62). Here the image is uploaded once as uint8 and everything after that runs in libunigen_hip.so:
  pre-processing   PIL's BICUBIC resampler (ug_img_resize_u8 with bicubic tables) and ug_img_u8_to_patches, which normalises and lays the pixels out
                   as the rows of the patch-embedding GEMM;
  backbone         ug_gemm_bf16 (q | k | v stacked; LayerScale + residual as UG_EPI_RES_GATE with one gate row; the position table as the residual of
                   the patch GEMM, whose C row map leaves each sample's class row free), ug_layernorm_rows, ug_flash_attn_fwd, ug_gelu_erf;
  neck and head    1x1 convolutions as GEMMs (the A row map skips the class row), ConvTranspose2d(k = s) as a GEMM + ug_deconv_scatter_nhwc, 3x3
                   convolutions as ug_conv2d_nhwc with the channels zero-padded to 64, ug_relu, ug_bilinear_nhwc, ug_depth_head_out;
  post-processing  ug_bicubic_f32 back to the image's size and ug_minmax_to_u8.
The reference's bf16 rounding points are kept: the 1x1 projection is not merged into the ConvTranspose2d and lambda is not merged into the weights.
Parameters in fp32 run the same orchestration through the `_f32` verification twins. Position embeddings for a patch grid other than the native one
are interpolated once per grid with torch (fp32, bicubic) and cached: a parameter transform, not per-image work.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import lib as L
from . import ops
from .engine import HipModule
from .ops import RowMap

BF, F32 = torch.bfloat16, torch.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _pad(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class DepthAnythingConfig:
    """transformers' DepthAnythingConfig with its nested Dinov2 `backbone_config`, as a plain object; the defaults are depth-anything-small's."""

    BACKBONE = dict(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, mlp_ratio=4, hidden_act="gelu", layer_norm_eps=1e-6, image_size=518,
                    patch_size=14, num_channels=3, qkv_bias=True, use_swiglu_ffn=False, apply_layernorm=True, reshape_hidden_states=False,
                    out_indices=None, out_features=None)
    TOP = dict(patch_size=14, reassemble_hidden_size=384, reassemble_factors=(4, 2, 1, 0.5), neck_hidden_sizes=(48, 96, 192, 384), fusion_hidden_size=64,
               head_in_index=-1, head_hidden_size=32, depth_estimation_type="relative", max_depth=None)

    def __init__(self, config: Optional[dict] = None, **kw):
        c = dict(config or {})
        c.update(kw)
        bb = dict(c.pop("backbone_config", None) or {})
        for k in list(c):                                        # a flat dict may carry the backbone's fields at the top level
            if k in self.BACKBONE and k not in self.TOP:
                bb.setdefault(k, c.pop(k))
        b = dict(self.BACKBONE)
        b.update({k: v for k, v in bb.items() if k in self.BACKBONE})
        t = dict(self.TOP)
        t.update({k: v for k, v in c.items() if k in self.TOP})
        if "reassemble_hidden_size" not in c:
            t["reassemble_hidden_size"] = b["hidden_size"]
        if bb.get("model_type", "dinov2") != "dinov2":
            raise NotImplementedError(f"DepthAnythingConfig: backbone model_type = {bb['model_type']!r} is not implemented (dinov2 only)")
        if b["use_swiglu_ffn"]:
            raise NotImplementedError("DepthAnythingConfig: use_swiglu_ffn = True is not implemented (the giant backbone's gated feed-forward)")
        if b["reshape_hidden_states"]:
            raise NotImplementedError("DepthAnythingConfig: reshape_hidden_states = True is not implemented (Depth Anything checkpoints set it to False)")
        if b["hidden_act"] != "gelu" or not b["qkv_bias"] or b["num_channels"] != 3:
            raise NotImplementedError("DepthAnythingConfig: hidden_act other than 'gelu', qkv_bias = False or num_channels other than 3 is not implemented")
        D, H = b["hidden_size"], b["num_attention_heads"]
        if D % H or D // H not in (64, 128):
            raise NotImplementedError(f"DepthAnythingConfig: num_attention_heads = {H} gives a head width of {D / H:g}; the attention kernel has 64 and 128")
        if t["depth_estimation_type"] not in ("relative", "metric"):
            raise ValueError(f"Unknown depth estimation type: {t['depth_estimation_type']}")
        nl = b["num_hidden_layers"]
        idx = b["out_indices"]
        if b["out_features"] is not None:
            idx = [int(str(f)[len("stage"):]) if str(f) != "stem" else 0 for f in b["out_features"]]
        if idx is None:
            idx = list(range(max(nl - 3, 1), nl + 1))            # the last four stages
        idx = [i % (nl + 1) for i in idx]
        if 0 in idx:
            raise NotImplementedError("DepthAnythingConfig: the stem as an output stage is not implemented")
        if len(idx) != len(t["neck_hidden_sizes"]) or len(idx) != len(t["reassemble_factors"]):
            raise ValueError(f"DepthAnythingConfig: {len(idx)} backbone stages, {len(t['neck_hidden_sizes'])} neck widths, {len(t['reassemble_factors'])} factors")
        for f in t["reassemble_factors"]:
            if not (f in (1, 2, 4, 8) or (0 < f < 1 and 1 / f == int(1 / f))):
                raise NotImplementedError(f"DepthAnythingConfig: reassemble factor {f} is not implemented")
        if t["reassemble_hidden_size"] != D or b["patch_size"] != t["patch_size"]:
            raise ValueError("DepthAnythingConfig: reassemble_hidden_size / patch_size differ from the backbone's hidden_size / patch_size")
        isz = b["image_size"]
        self.image_size = int(isz if isinstance(isz, int) else isz[0])
        self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.mlp_ratio = D, nl, H, b["mlp_ratio"]
        self.layer_norm_eps, self.patch_size, self.apply_layernorm, self.out_indices = float(b["layer_norm_eps"]), int(b["patch_size"]), bool(b["apply_layernorm"]), idx
        self.reassemble_hidden_size, self.reassemble_factors = D, tuple(t["reassemble_factors"])
        self.neck_hidden_sizes, self.fusion_hidden_size = tuple(int(v) for v in t["neck_hidden_sizes"]), int(t["fusion_hidden_size"])
        self.head_in_index, self.head_hidden_size = int(t["head_in_index"]), int(t["head_hidden_size"])
        self.depth_estimation_type, self.max_depth = t["depth_estimation_type"], float(t["max_depth"] if t["max_depth"] is not None else 1)

    def to_dict(self) -> dict:
        """transformers' config.json layout."""
        return dict(model_type="depth_anything", patch_size=self.patch_size, reassemble_hidden_size=self.reassemble_hidden_size,
                    reassemble_factors=list(self.reassemble_factors), neck_hidden_sizes=list(self.neck_hidden_sizes), fusion_hidden_size=self.fusion_hidden_size,
                    head_in_index=self.head_in_index, head_hidden_size=self.head_hidden_size, depth_estimation_type=self.depth_estimation_type,
                    max_depth=self.max_depth,
                    backbone_config=dict(model_type="dinov2", hidden_size=self.hidden_size, num_hidden_layers=self.num_hidden_layers,
                                         num_attention_heads=self.num_attention_heads, mlp_ratio=self.mlp_ratio, hidden_act="gelu", layer_norm_eps=self.layer_norm_eps,
                                         image_size=self.image_size, patch_size=self.patch_size, num_channels=3, qkv_bias=True, use_swiglu_ffn=False,
                                         apply_layernorm=self.apply_layernorm, reshape_hidden_states=False, out_indices=list(self.out_indices)))


def _conv_w(w: torch.Tensor, cout_p: int, cin_p: int) -> torch.Tensor:
    """torch's [Cout][Cin][KH][KW] -> [cout_p][KH][KW][cin_p], zero rows and zero input channels in the pads."""
    co, ci, kh, kw = w.shape
    out = torch.zeros(cout_p, kh, kw, cin_p, dtype=w.dtype, device=w.device)
    out[:co, :, :, :ci] = w.permute(0, 2, 3, 1)
    return out.contiguous()


def _vec_p(v: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=v.dtype, device=v.device)
    out[:v.numel()] = v.reshape(-1)
    return out


class DepthAnythingForDepthEstimation(HipModule):
    """transformers' DepthAnythingForDepthEstimation: same config, same state-dict keys, `forward` -> predicted_depth fp32 [B, 14 ph, 14 pw]."""

    def __init__(self, config=None, device=None, dtype=BF):
        super().__init__()
        self.config = config if isinstance(config, DepthAnythingConfig) else DepthAnythingConfig(config)
        if dtype not in (BF, F32):
            raise TypeError("DepthAnythingForDepthEstimation computes in torch.bfloat16 (or torch.float32 for verification)")
        self._device, self._dtype = torch.device(device) if device is not None else torch.device("cpu"), dtype
        self._sd: Dict[str, torch.Tensor] = {}
        self._p: Dict[str, torch.Tensor] = {}
        self._pos: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._idx: Dict[int, torch.Tensor] = {}
        self.image_mean, self.image_std = IMAGENET_MEAN, IMAGENET_STD

    dtype = property(lambda self: self._dtype)
    device = property(lambda self: self._device)

    # ---------------------------------------------------------------- parameters --------------------------------------------------------------
    def expected_keys(self) -> Dict[str, Tuple[int, ...]]:
        """Every key of transformers' state dict that this class reads, with its shape (`backbone.embeddings.mask_token` is ignored)."""
        c = self.config
        D, P, F, Hh = c.hidden_size, c.patch_size, c.fusion_hidden_size, c.head_hidden_size
        n0 = c.image_size // P
        e: Dict[str, Tuple[int, ...]] = {"backbone.embeddings.cls_token": (1, 1, D), "backbone.embeddings.position_embeddings": (1, 1 + n0 * n0, D),
                                         "backbone.embeddings.patch_embeddings.projection.weight": (D, 3, P, P),
                                         "backbone.embeddings.patch_embeddings.projection.bias": (D,)}

        def lin(p, o, i):
            e[p + ".weight"], e[p + ".bias"] = (o, i), (o,)

        def conv(p, o, i, k, bias=True):
            e[p + ".weight"] = (o, i, k, k)
            if bias:
                e[p + ".bias"] = (o,)

        for i in range(c.num_hidden_layers):
            p = f"backbone.encoder.layer.{i}."
            for n in ("norm1", "norm2"):
                e[p + n + ".weight"], e[p + n + ".bias"] = (D,), (D,)
            for n in ("query", "key", "value"):
                lin(p + "attention.attention." + n, D, D)
            lin(p + "attention.output.dense", D, D)
            lin(p + "mlp.fc1", D * c.mlp_ratio, D)
            lin(p + "mlp.fc2", D, D * c.mlp_ratio)
            e[p + "layer_scale1.lambda1"], e[p + "layer_scale2.lambda1"] = (D,), (D,)
        e["backbone.layernorm.weight"], e["backbone.layernorm.bias"] = (D,), (D,)
        for i, (ch, f) in enumerate(zip(c.neck_hidden_sizes, c.reassemble_factors)):
            p = f"neck.reassemble_stage.layers.{i}."
            conv(p + "projection", ch, D, 1)
            if f > 1:
                conv(p + "resize", ch, ch, int(f))
            elif f < 1:
                conv(p + "resize", ch, ch, 3)
            conv(f"neck.convs.{i}", F, ch, 3, bias=False)
            p = f"neck.fusion_stage.layers.{i}."
            conv(p + "projection", F, F, 1)
            for r in ("residual_layer1", "residual_layer2"):
                conv(p + r + ".convolution1", F, F, 3)
                conv(p + r + ".convolution2", F, F, 3)
        conv("head.conv1", F // 2, F, 3)
        conv("head.conv2", Hh, F // 2, 3)
        conv("head.conv3", 1, Hh, 1)
        return e

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        exp = self.expected_keys()
        unexpected = [k for k in sd if k not in exp and k != "backbone.embeddings.mask_token"]
        missing = sorted(set(exp) - set(sd))
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {unexpected[:4]}")
        for k, shape in exp.items():
            if k in sd:
                if tuple(sd[k].shape) != shape:
                    raise ValueError(f"{k}: shape {tuple(sd[k].shape)} does not match {shape}")
                self._sd[k] = sd[k].detach().to(device=self._device, dtype=self._dtype)
        if not missing:
            self._pack()
        return missing, unexpected

    @classmethod
    def from_pretrained(cls, path, device=None, dtype=BF) -> "DepthAnythingForDepthEstimation":
        """A local directory only (no hub access): config.json + model.safetensors."""
        path = os.fspath(path)
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local directory (this package does not download checkpoints)")
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        from safetensors.torch import load_file
        m = cls(cfg, device=device, dtype=dtype)
        m.load_state_dict(load_file(os.path.join(path, "model.safetensors")))
        return m

    def init_synthetic_(self, seed: int = 0) -> "DepthAnythingForDepthEstimation":
        """Seeded random weights for tests and benchmarks, drawn on the model's device, with a spread that keeps the head alive: weights
        N(0, (1.4 / sqrt(fan_in))^2), biases N(0, 0.1^2), norm weights 1 + 0.2 N, lambda U(0.5, 1.5), class token and positions 0.5 N, head.conv3.bias 0.5."""
        g = torch.Generator(device=self._device).manual_seed(seed)
        rn = lambda shape: torch.randn(shape, generator=g, device=self._device, dtype=F32)
        sd = {}
        for k, shape in self.expected_keys().items():
            if k.endswith("lambda1"):
                t = 0.5 + torch.rand(shape, generator=g, device=self._device, dtype=F32)
            elif "cls_token" in k or "position_embeddings" in k:
                t = 0.5 * rn(shape)
            elif k == "head.conv3.bias":
                t = torch.full(shape, 0.5, device=self._device)
            elif k.endswith(".bias"):
                t = 0.1 * rn(shape)
            elif "norm" in k:
                t = 1.0 + 0.2 * rn(shape)
            else:
                fan_in = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
                if ".resize." in k and self._factor_of(k) > 1:                     # ConvTranspose2d [Cin][Cout][f][f] with stride f: one tap per output
                    fan_in = shape[0]
                t = (1.4 / math.sqrt(fan_in)) * rn(shape)
            sd[k] = t.to(BF)
        self.load_state_dict(sd)
        return self

    def _factor_of(self, key: str) -> float:
        return self.config.reassemble_factors[int(key.split(".")[3])]

    def _pack(self) -> None:
        """Load-time layouts: q | k | v stacked, conv weights [Cout][KH][KW][Cin] with Cin (and the Cout a later convolution reads) zero-padded to 64,
        the patch weight padded to Kp, ConvTranspose2d weights re-laid as [(ky, kx, co)][Cin]."""
        c, s, p = self.config, self._sd, {}
        D, P, F = c.hidden_size, c.patch_size, c.fusion_hidden_size
        Fp, Kp = _pad(F, 64), _pad(3 * P * P, 64)
        pw = torch.zeros(D, Kp, dtype=self._dtype, device=self._device)
        pw[:, :3 * P * P] = s["backbone.embeddings.patch_embeddings.projection.weight"].reshape(D, -1)
        p["patch_w"], p["patch_b"] = pw, s["backbone.embeddings.patch_embeddings.projection.bias"].contiguous()
        for i in range(c.num_hidden_layers):
            k = f"backbone.encoder.layer.{i}."
            p[f"l{i}.qkv_w"] = torch.cat([s[k + f"attention.attention.{n}.weight"] for n in ("query", "key", "value")], 0).contiguous()
            p[f"l{i}.qkv_b"] = torch.cat([s[k + f"attention.attention.{n}.bias"] for n in ("query", "key", "value")], 0).contiguous()
            p[f"l{i}.ls1"], p[f"l{i}.ls2"] = s[k + "layer_scale1.lambda1"].reshape(1, D).contiguous(), s[k + "layer_scale2.lambda1"].reshape(1, D).contiguous()
        for i, (ch, f) in enumerate(zip(c.neck_hidden_sizes, c.reassemble_factors)):
            k, cp = f"neck.reassemble_stage.layers.{i}.", _pad(ch, 64)
            w = torch.zeros(cp, D, dtype=self._dtype, device=self._device)
            w[:ch] = s[k + "projection.weight"].reshape(ch, D)
            p[f"n{i}.proj_w"], p[f"n{i}.proj_b"] = w, _vec_p(s[k + "projection.bias"], cp)
            if f > 1:
                f = int(f)
                w = torch.zeros(f * f * ch, cp, dtype=self._dtype, device=self._device)
                w[:, :ch] = s[k + "resize.weight"].permute(2, 3, 1, 0).reshape(f * f * ch, ch)          # [Cin][Cout][ky][kx] -> [(ky, kx, co)][Cin]
                p[f"n{i}.up_w"], p[f"n{i}.up_b"] = w, s[k + "resize.bias"].contiguous()
            elif f < 1:
                p[f"n{i}.down_w"], p[f"n{i}.down_b"] = _conv_w(s[k + "resize.weight"], cp, cp), _vec_p(s[k + "resize.bias"], cp)
            p[f"n{i}.conv_w"] = _conv_w(s[f"neck.convs.{i}.weight"], Fp, cp)
            k = f"neck.fusion_stage.layers.{i}."
            w = torch.zeros(Fp, Fp, dtype=self._dtype, device=self._device)
            w[:F, :F] = s[k + "projection.weight"].reshape(F, F)
            p[f"f{i}.proj_w"], p[f"f{i}.proj_b"] = w, _vec_p(s[k + "projection.bias"], Fp)
            for r in (1, 2):
                for q in (1, 2):
                    kk = k + f"residual_layer{r}.convolution{q}."
                    p[f"f{i}.r{r}c{q}_w"], p[f"f{i}.r{r}c{q}_b"] = _conv_w(s[kk + "weight"], Fp, Fp), _vec_p(s[kk + "bias"], Fp)
        h1p, hh = _pad(F // 2, 64), c.head_hidden_size
        p["h.c1_w"], p["h.c1_b"] = _conv_w(s["head.conv1.weight"], h1p, Fp), _vec_p(s["head.conv1.bias"], h1p)
        p["h.c2_w"], p["h.c2_b"] = _conv_w(s["head.conv2.weight"], _pad(hh, 8), h1p), _vec_p(s["head.conv2.bias"], _pad(hh, 8))
        p["h.c3_w"], p["h.c3_b"] = _vec_p(s["head.conv3.weight"], _pad(hh, 8)), s["head.conv3.bias"].reshape(1).contiguous()
        self._p = p
        self._pos.clear()

    def position_table(self, ph: int, pw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(patch positions [ph * pw, D], class token + its position [1, D]) for a patch grid: Dinov2Embeddings.interpolate_pos_encoding (bicubic,
        align_corners=False, in fp32, cast back), computed once per grid."""
        t = self._pos.get((ph, pw))
        if t is None:
            c, D = self.config, self.config.hidden_size
            pos = self._sd["backbone.embeddings.position_embeddings"]
            n0 = int(round((pos.shape[1] - 1) ** 0.5))
            patch = pos[0, 1:]
            if (ph, pw) != (n0, n0):
                grid = patch.reshape(1, n0, n0, D).permute(0, 3, 1, 2).to(F32)
                grid = torch.nn.functional.interpolate(grid, size=(ph, pw), mode="bicubic", align_corners=False).to(self._dtype)
                patch = grid.permute(0, 2, 3, 1).reshape(ph * pw, D)
            cls = (self._sd["backbone.embeddings.cls_token"].reshape(1, D) + pos[0, :1]).contiguous()          # one rounding, as cat + add does
            t = (patch.contiguous(), cls)
            if len(self._pos) >= 16:
                self._pos.clear()
            self._pos[(ph, pw)] = t
        return t

    # ---------------------------------------------------------------- forward ------------------------------------------------------------------
    def _new(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self._dtype, device=self._device)

    def _conv(self, x, w, b, *, stride=1, residual=None):
        B, H, W, _ = x.shape
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        out = self._new(B, Ho, Wo, w.shape[0])
        return ops.conv2d_nhwc(x, w, b, out, B=B, H=H, W=W, Ho=Ho, Wo=Wo, KH=3, KW=3, stride=stride, pad_t=1, pad_l=1, residual=residual)

    def _rcu(self, x, i: int, r: int):
        """DepthAnythingPreActResidualLayer: x + conv2(relu(conv1(relu(x))))."""
        p = self._p
        t = self._conv(ops.relu(x), p[f"f{i}.r{r}c1_w"], p[f"f{i}.r{r}c1_b"])
        ops.relu(t, t)
        return self._conv(t, p[f"f{i}.r{r}c2_w"], p[f"f{i}.r{r}c2_b"], residual=x)

    def backbone(self, patches: torch.Tensor, B: int, ph: int, pw: int, stages: Optional[dict] = None) -> List[torch.Tensor]:
        """Patch rows [B * ph * pw, Kp] -> the selected hidden states [B * (1 + ph * pw), D], final layernorm applied."""
        c, p = self.config, self._p
        D, H, N = c.hidden_size, c.num_attention_heads, ph * pw
        T, dh, Fm = N + 1, c.hidden_size // c.num_attention_heads, c.hidden_size * c.mlp_ratio
        M = B * T
        pos, cls = self.position_table(ph, pw)
        x = self._new(M, D)
        # conv output (rounded) + position (rounded again), written behind each sample's class row
        ops.gemm(patches, p["patch_w"], p["patch_b"], x[1:], M=B * N, epilogue=L.EPI_RES_SCALE, residual=pos, r_map=RowMap(N, 0), c_map=RowMap(N, T), alpha=1.0)
        idx = self._idx.get(B)
        if idx is None:
            idx = self._idx[B] = torch.zeros(B, dtype=torch.int32, device=self._device)
        ops.gather_rows(cls, idx, x.view(B, T, D)[:, 0])
        if stages is not None:
            stages["embeddings"] = x.view(B, T, D)
        lnw, lnb = self._sd["backbone.layernorm.weight"], self._sd["backbone.layernorm.bias"]
        feats = []
        s3 = (3 * D, T * 3 * D)
        for i in range(c.num_hidden_layers):
            k = f"backbone.encoder.layer.{i}."
            sd = self._sd
            h = ops.layernorm_rows(x, sd[k + "norm1.weight"], sd[k + "norm1.bias"], c.layer_norm_eps)
            qkv = ops.gemm(h, p[f"l{i}.qkv_w"], p[f"l{i}.qkv_b"], self._new(M, 3 * D), M=M)
            att = self._new(M, D)
            ops.flash_attn(qkv, qkv[:, D:], qkv[:, 2 * D:], att, batches=B, heads=H, dh=dh, Lq=T, Lkv=T, q_strides=s3, k_strides=s3, v_strides=s3,
                           o_strides=(D, T * D))
            x = ops.gemm(att, sd[k + "attention.output.dense.weight"], sd[k + "attention.output.dense.bias"], self._new(M, D), M=M, epilogue=L.EPI_RES_GATE,
                         residual=x, gate=p[f"l{i}.ls1"], gate_ld=D, rows_per_sample=M)
            h = ops.layernorm_rows(x, sd[k + "norm2.weight"], sd[k + "norm2.bias"], c.layer_norm_eps)
            f = ops.gemm(h, sd[k + "mlp.fc1.weight"], sd[k + "mlp.fc1.bias"], self._new(M, Fm), M=M)
            ops.gelu_erf(f, f)
            x = ops.gemm(f, sd[k + "mlp.fc2.weight"], sd[k + "mlp.fc2.bias"], self._new(M, D), M=M, epilogue=L.EPI_RES_GATE, residual=x,
                         gate=p[f"l{i}.ls2"], gate_ld=D, rows_per_sample=M)
            if i + 1 in c.out_indices:
                feats.append(ops.layernorm_rows(x, lnw, lnb, c.layer_norm_eps) if c.apply_layernorm else x)
        if stages is not None:
            stages["feature_maps"] = [f.view(B, T, D) for f in feats]
        return feats

    def neck_and_head(self, feats: List[torch.Tensor], B: int, ph: int, pw: int, stages: Optional[dict] = None) -> torch.Tensor:
        c, p = self.config, self._p
        D, N, F, P = c.hidden_size, ph * pw, c.fusion_hidden_size, c.patch_size
        T, Fp = N + 1, _pad(c.fusion_hidden_size, 64)
        maps, reasm = [], []
        for i, (fm, ch, f) in enumerate(zip(feats, c.neck_hidden_sizes, c.reassemble_factors)):
            cp = _pad(ch, 64)
            # the 1x1 projection reads the feature map without its class row: rows b T + 1 + n
            y = ops.gemm(fm[1:], p[f"n{i}.proj_w"], p[f"n{i}.proj_b"], self._new(B * N, cp), M=B * N, a_map=RowMap(N, T))
            if f > 1:
                f = int(f)
                prod = ops.gemm(y, p[f"n{i}.up_w"], None, self._new(B * N, f * f * ch, dtype=F32), M=B * N, epilogue=L.EPI_F32)
                y = ops.deconv_scatter_nhwc(prod, p[f"n{i}.up_b"], B=B, h=ph, w=pw, f=f, Cout=ch, Cp=cp)
            elif f < 1:
                y = self._conv(y.view(B, ph, pw, cp), p[f"n{i}.down_w"], p[f"n{i}.down_b"], stride=int(1 / f))
            else:
                y = y.view(B, ph, pw, cp)
            reasm.append(y)
            maps.append(self._conv(y, p[f"n{i}.conv_w"], None))
        fused, h = [], None
        n = len(maps)
        for i in range(n):
            m = maps[n - 1 - i]
            if h is None:
                h = m
            else:
                if h.shape != m.shape:
                    m = ops.bilinear_nhwc(m, h.shape[1], h.shape[2], align_corners=False)
                h = ops.add(h, self._rcu(m, i, 1), torch.empty_like(h))
            h = self._rcu(h, i, 2)
            Ho, Wo = (maps[n - 2 - i].shape[1], maps[n - 2 - i].shape[2]) if i + 1 < n else (2 * h.shape[1], 2 * h.shape[2])
            h = ops.bilinear_nhwc(h, Ho, Wo, align_corners=True)
            h = ops.gemm(h.view(-1, Fp), p[f"f{i}.proj_w"], p[f"f{i}.proj_b"], self._new(B * Ho * Wo, Fp), M=B * Ho * Wo).view(B, Ho, Wo, Fp)
            fused.append(h)
        if stages is not None:
            stages["reassembled"] = [r[..., :ch] for r, ch in zip(reasm, c.neck_hidden_sizes)]
            stages["fused"] = [t[..., :F] for t in fused]
        h = self._conv(fused[c.head_in_index], p["h.c1_w"], p["h.c1_b"])
        h = ops.bilinear_nhwc(h, ph * P, pw * P, align_corners=True)
        h = self._conv(h, p["h.c2_w"], p["h.c2_b"])
        return ops.depth_head_out(h, p["h.c3_w"][:c.head_hidden_size], p["h.c3_b"], C_=c.head_hidden_size, max_depth=c.max_depth,
                                  metric=c.depth_estimation_type == "metric")

    @torch.no_grad()
    def forward(self, pixel_u8: Optional[torch.Tensor] = None, patches: Optional[torch.Tensor] = None, grid: Optional[Tuple[int, int]] = None,
                return_stages: bool = False):
        """`pixel_u8`: uint8 [B, H, W, C] on the GPU, already at the model's size (H, W multiples of the patch size), normalised here with the ImageNet
        constants; or `patches` from DepthImageProcessor.preprocess with `grid` = (ph, pw). -> predicted_depth fp32 [B, 14 ph, 14 pw]
        (with return_stages, also the dict of intermediate tensors, NHWC with the pad channels cut)."""
        if not self._p:
            raise L.UniGenHipError("DepthAnythingForDepthEstimation: no weights loaded")
        if self._device.type != "cuda":
            raise L.UniGenHipError("the depth model runs on the HIP device only (unigen_amd has no CPU path): create the model with device='cuda'")
        P = self.config.patch_size
        if (pixel_u8 is None) == (patches is None):
            raise ValueError("forward takes either pixel_u8 or patches")
        if pixel_u8 is not None:
            B, H, W, _ = pixel_u8.shape
            ph, pw = H // P, W // P
            patches = ops.img_u8_to_patches(pixel_u8, P, self.image_mean, self.image_std, dtype=self._dtype)
        else:
            if grid is None:
                raise ValueError("forward(patches=...) needs grid=(ph, pw)")
            ph, pw = grid
            B = patches.shape[0] // (ph * pw)
            if patches.dtype != self._dtype or patches.shape[0] != B * ph * pw:
                raise ValueError(f"patches: expected {self._dtype} [B * {ph} * {pw}, Kp], got {patches.dtype} {tuple(patches.shape)}")
        stages = {} if return_stages else None
        feats = self.backbone(patches, B, ph, pw, stages)
        depth = self.neck_and_head(feats, B, ph, pw, stages)
        if return_stages:
            stages["predicted_depth"] = depth
            return depth, stages
        return depth

    __call__ = forward


class DepthImageProcessor:
    """transformers' DPTImageProcessor with depth-anything's settings: a BICUBIC resize that keeps the aspect ratio and lands on multiples of 14,
    then rescale and normalise - here PIL's resampler on the GPU followed by ug_img_u8_to_patches."""

    def __init__(self, size=518, keep_aspect_ratio: bool = True, ensure_multiple_of: int = 14, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD,
                 rescale_factor: float = 1 / 255, device=None):
        if isinstance(size, dict):
            size = (size["height"], size["width"])
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.keep_aspect_ratio, self.ensure_multiple_of = bool(keep_aspect_ratio), int(ensure_multiple_of)
        self.image_mean, self.image_std, self.rescale_factor = tuple(image_mean), tuple(image_std), float(rescale_factor)
        self.device = None if device is None else torch.device(device)

    def output_size(self, height: int, width: int) -> Tuple[int, int]:
        """get_resize_output_image_size of the DPT processor: scale as little as possible, then the nearest multiple (Python's round: half to even)."""
        m = self.ensure_multiple_of
        sh, sw = self.size[0] / height, self.size[1] / width
        if self.keep_aspect_ratio:
            if abs(1 - sw) < abs(1 - sh):
                sh = sw
            else:
                sw = sh

        def constrain(val):
            x = round(val / m) * m
            if x < 0:                                            # min_val = 0; max_val is never given
                x = math.ceil(val / m) * m
            return x

        return constrain(sh * height), constrain(sw * width)

    def preprocess(self, images, dtype=BF, patch_size: int = 14):
        """Image-like or a list (the kinds unigen_amd.image takes) -> (patches [B * ph * pw, Kp] in `dtype`, (ph, pw), (H, W) of the input)."""
        from .image import _default_device, resize_u8, to_device_u8
        first = images[0] if isinstance(images, (list, tuple)) and images else images
        dev = self.device or (first.device if isinstance(first, torch.Tensor) and first.is_cuda else _default_device())
        x = to_device_u8(images, dev)
        H, W = x.shape[1], x.shape[2]
        h, w = self.output_size(H, W)
        if h < patch_size or w < patch_size or h % patch_size or w % patch_size:
            raise ValueError(f"a {H}x{W} image resizes to {h}x{w}, which is not a positive multiple of the patch size {patch_size}")
        x = resize_u8(x, h, w, filter="bicubic")
        patches = ops.img_u8_to_patches(x, patch_size, self.image_mean, self.image_std, self.rescale_factor, dtype=dtype)
        return patches, (h // patch_size, w // patch_size), (H, W)


def _estimate(model: DepthAnythingForDepthEstimation, images, processor: Optional[DepthImageProcessor], channels: int):
    processor = processor or DepthImageProcessor(device=model.device)
    patches, grid, (H, W) = processor.preprocess(images, dtype=model.dtype, patch_size=model.config.patch_size)
    depth = model(patches=patches, grid=grid)
    depth = ops.bicubic_f32(depth, H, W)
    return depth, ops.minmax_to_u8(depth, channels)


def estimate_depth(model: DepthAnythingForDepthEstimation, images, processor: Optional[DepthImageProcessor] = None):
    """transformers' depth-estimation pipeline: per image {"predicted_depth": fp32 [H, W], "depth": uint8 [H, W]} - one dict for one image, a list
    for a list or a batch. Everything stays on the GPU and nothing synchronises with the host, unless PIL images went in: then "depth" is a PIL image."""
    from .image import _is_pil
    many = isinstance(images, (list, tuple)) or getattr(images, "ndim", 3) == 4
    first = images[0] if isinstance(images, (list, tuple)) and images else images
    depth, u8 = _estimate(model, images, processor, 1)
    if _is_pil(first):
        from PIL import Image
        arr = u8.cpu().numpy()
        out = [{"predicted_depth": depth[b], "depth": Image.fromarray(arr[b, :, :, 0])} for b in range(depth.shape[0])]
    else:
        out = [{"predicted_depth": depth[b], "depth": u8[b, :, :, 0]} for b in range(depth.shape[0])]
    return out if many else out[0]
