"""AutoencoderDC (DC-AE) on MI355X: Sana's 32x autoencoder (`dc-ae-f32c32-sana-1.x`: 32x spatial, 32 latent channels).

The class carries diffusers' constructor arguments and config names, its state-dict keys and `from_pretrained` of a local directory (config.json +
safetensors). diffusers is not a dependency and its source is not at hand: the semantics are restated from the published code (autoencoder_dc.py;
SanaMultiscaleLinearAttention and its processor in attention_processor.py; GLUMBConv), so parity with diffusers is unpinned, as for the VAE and Sana
(DESIGN.md 7g). `encode(x).latent` is deterministic (DC-AE has no posterior), `decode(z).sample`, `forward`, `config.scaling_factor`.

Nothing here computes in torch: activations are NHWC 2-D tensors [B*H*W, C] and every op is a C-ABI call (unigen_amd/ops.py).
    ResBlock            conv1 (3x3, bias) -> SiLU -> conv2 (3x3, no bias) -> RMSNorm (weight, bias) -> + x
                        ug_conv2d_nhwc, ug_silu, ug_conv2d_nhwc, ug_rmsnorm_bias_rows with the residual
    EfficientViTBlock   SanaMultiscaleLinearAttention (+ x), then GLUMBConv (+ x):
                        [Q | K | V] = one ug_gemm_bf16 against the stacked to_q / to_k / to_v weight; every scale of to_qkv_multiscale = one
                        ug_msconv_proj of that buffer into the next 3 C columns; ug_linear_attn per scale (heads of 32, eps 1e-15); to_out GEMM;
                        ug_rmsnorm_bias_rows + x; conv_inverted GEMM (C -> 8 C, bias); ug_glu_dwconv3x3; conv_point GEMM (4 C -> C);
                        ug_rmsnorm_bias_rows + x
    DCDownBlock2d       "Conv": ug_dc_shortcut_down (no x) -> the stride-2 convolution takes it as its residual;
                        "pixel_unshuffle": the convolution to Cout / 4 channels, then ug_dc_shortcut_down with x_shuffle adds the two rearranged tensors
    DCUpBlock2d         "interpolate": ug_dc_shortcut_up (no x) -> the convolution (nearest 2x folded into its gather) takes it as its residual;
                        "pixel_shuffle": the convolution to 4 Cout channels, then ug_dc_shortcut_up with x_shuffle
    Encoder             conv_in, the stages (blocks, then the down block), conv_out(x) + group-mean shortcut(x)
    Decoder             conv_in(z) + repeat shortcut(z), the stages from the last to the first (up block first), norm_out + ReLU, conv_out

The 96-channel heads. diffusers concatenates to_q | to_k | to_v (and every scale's projection of that tensor) on the channel axis and RESHAPES the result
to [B, -1, 96, H W]: head g of a scale is channels [96 g, 96 g + 96) of that scale's tensor - q, k, v are its three 32-blocks - not head g of to_q,
to_k and to_v. ug_linear_attn wants head g of q at columns [32 g, 32 g + 32) of a q view. So the rows of the stacked weight are permuted once at load
time in 32-row blocks (block 3 g + part -> part * heads + g), and the channels of proj_in and the groups of proj_out alike: the grouped convolution's
groups are exactly those blocks, so the permutation commutes with it, the GEMM writes [Q | K | V] in the kernel's layout and no activation is ever
shuffled. The named parameters stay the tensors that were loaded, under diffusers' keys; the permuted copies are separate.

diffusers switches to a quadratic form of the attention when H W <= 32; it is the same function in exact arithmetic, and the linear kernel serves both
(tests/test_dcae_ref_cpu.py shows the two forms agree to 1e-13).

fp32 parameters select the verification twins, as for the VAE. Open: tiling and slicing, any backward, a Sana pipeline and scheduler, the
"batch_norm" / "relu6" DC-AE variants and the variant whose conv_in / conv_out are down / up blocks (layers_per_block[0] == 0).
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .sana import _Params

BF, F32 = torch.bfloat16, torch.float32
DH = 32                      # the head width of ug_linear_attn and ug_msconv_proj
NORM_EPS = 1e-5              # RMSNorm(C, eps = 1e-5, elementwise_affine = True, bias = True): every norm of DC-AE
OPEN = "open (docs/NEXT_ROWS.md, \"Sana\")"

DCAE_CONFIG = dict(in_channels=3, latent_channels=32, attention_head_dim=32, encoder_block_types="ResBlock", decoder_block_types="ResBlock",
                   encoder_block_out_channels=(128, 256, 512, 512, 1024, 1024), decoder_block_out_channels=(128, 256, 512, 512, 1024, 1024),
                   encoder_layers_per_block=(2, 2, 2, 3, 3, 3), decoder_layers_per_block=(3, 3, 3, 3, 3, 3),
                   encoder_qkv_multiscales=((), (), (), (5,), (5,), (5,)), decoder_qkv_multiscales=((), (), (), (5,), (5,), (5,)),
                   upsample_block_type="pixel_shuffle", downsample_block_type="pixel_unshuffle", decoder_norm_types="rms_norm", decoder_act_fns="silu",
                   scaling_factor=1.0)
# the published dc-ae-f32c32-sana-1.x geometry
DCAE_F32C32_SANA = dict(DCAE_CONFIG, encoder_block_types=("ResBlock",) * 3 + ("EfficientViTBlock",) * 3,
                        decoder_block_types=("ResBlock",) * 3 + ("EfficientViTBlock",) * 3, scaling_factor=0.41407)


def _pad(n: int, q: int) -> int:
    return (n + q - 1) // q * q


def _tup(v, n: int, name: str) -> tuple:
    t = (v,) * n if isinstance(v, str) else tuple(v)
    if len(t) != n:
        raise ValueError(f"AutoencoderDC: {name} has {len(t)} entries for {n} stages")
    return t


class AutoencoderDC(_Params):
    """Drop-in for diffusers' `AutoencoderDC` (encode / decode / forward). See the module docstring for the kernels and the limits."""

    def __init__(self, config: Optional[dict] = None, device=None, dtype=BF, **kw):
        super().__init__(device, dtype)
        c = dict(DCAE_CONFIG)
        given = dict(config or {})
        given.update(kw)
        # diffusers writes its own bookkeeping keys ("_class_name", ...) into config.json; later releases add the two shortcut switches (default on)
        for k in ("encoder_out_shortcut", "decoder_in_shortcut"):
            if not given.pop(k, True):
                raise NotImplementedError(f"AutoencoderDC: {k} = False is not implemented (every published DC-AE has the shortcut)")
        unknown = sorted(k for k in given if k not in c and not k.startswith("_"))
        if unknown:
            raise ValueError(f"AutoencoderDC: config keys {unknown} are not known to this class; nothing is ignored silently")
        c.update({k: v for k, v in given.items() if k in c})
        for side in ("encoder", "decoder"):
            ch = c[f"{side}_block_out_channels"] = tuple(int(v) for v in c[f"{side}_block_out_channels"])
            n = len(ch)
            c[f"{side}_block_types"] = _tup(c[f"{side}_block_types"], n, f"{side}_block_types")
            c[f"{side}_layers_per_block"] = tuple(int(v) for v in _tup(c[f"{side}_layers_per_block"], n, f"{side}_layers_per_block"))
            c[f"{side}_qkv_multiscales"] = tuple(tuple(int(k) for k in s) for s in _tup(c[f"{side}_qkv_multiscales"], n, f"{side}_qkv_multiscales"))
        n = len(c["decoder_block_out_channels"])
        c["decoder_norm_types"] = _tup(c["decoder_norm_types"], n, "decoder_norm_types")
        c["decoder_act_fns"] = _tup(c["decoder_act_fns"], n, "decoder_act_fns")
        self.config = SimpleNamespace(**c)
        self._validate()
        self._p: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ what is refused, by argument ------------------
    def _validate(self) -> None:
        c = self.config
        if c.attention_head_dim != DH:
            raise NotImplementedError(f"AutoencoderDC: attention_head_dim = {c.attention_head_dim}: the linear attention and the multiscale projection "
                                      f"kernels have head width {DH}")
        bad = sorted({t for t in c.decoder_norm_types if t != "rms_norm"})
        if bad:
            raise NotImplementedError(f"AutoencoderDC: decoder_norm_types {bad}: only \"rms_norm\" is implemented (the \"batch_norm\" variants are {OPEN})")
        bad = sorted({t for t in c.decoder_act_fns if t != "silu"})
        if bad:
            raise NotImplementedError(f"AutoencoderDC: decoder_act_fns {bad}: only \"silu\" (with the decoder's \"relu\" conv_act) is implemented "
                                      f"(the \"relu6\" variants are {OPEN})")
        if c.downsample_block_type not in ("pixel_unshuffle", "Conv", "conv"):
            raise ValueError(f"AutoencoderDC: downsample_block_type = {c.downsample_block_type!r} (\"pixel_unshuffle\" or \"Conv\")")
        if c.upsample_block_type not in ("pixel_shuffle", "interpolate"):
            raise ValueError(f"AutoencoderDC: upsample_block_type = {c.upsample_block_type!r} (\"pixel_shuffle\" or \"interpolate\")")
        if c.latent_channels % 8 or c.latent_channels < 8:
            raise NotImplementedError(f"AutoencoderDC: latent_channels = {c.latent_channels} must be a multiple of 8 (the shortcut kernels' 16-byte rows)")
        if c.in_channels < 1:
            raise ValueError(f"AutoencoderDC: in_channels = {c.in_channels}")
        if len(c.encoder_block_out_channels) != len(c.decoder_block_out_channels):
            raise NotImplementedError("AutoencoderDC: encoder_block_out_channels and decoder_block_out_channels differ in length: the two spatial factors "
                                      "would differ")
        for side in ("encoder", "decoder"):
            ch, layers, types = getattr(c, f"{side}_block_out_channels"), getattr(c, f"{side}_layers_per_block"), getattr(c, f"{side}_block_types")
            if layers[0] == 0:
                raise NotImplementedError(f"AutoencoderDC: {side}_layers_per_block[0] == 0 (the variant whose conv_in / conv_out are down / up blocks) is "
                                          f"not implemented; it is {OPEN}")
            if min(layers) < 1:
                raise NotImplementedError(f"AutoencoderDC: {side}_layers_per_block = {layers}: a stage without layers is not implemented")
            for t in types:
                if t not in ("ResBlock", "EfficientViTBlock"):
                    raise ValueError(f"AutoencoderDC: {side}_block_types has {t!r} (\"ResBlock\" or \"EfficientViTBlock\")")
            for w in ch:
                if w % 64:
                    raise NotImplementedError(f"AutoencoderDC: {side}_block_out_channels = {ch}: every width must be a multiple of 64 (the convolution's "
                                              "and the GEMM's K granularity)")
            for s in getattr(c, f"{side}_qkv_multiscales"):
                for k in s:
                    if k not in (3, 5):
                        raise NotImplementedError(f"AutoencoderDC: {side}_qkv_multiscales has kernel size {k}: ug_msconv_proj is built for 5 and 3")
            for a, b in zip(ch[:-1], ch[1:]):          # a: the finer stage
                if (a * 4) % b or (b * 4) % a:
                    raise ValueError(f"AutoencoderDC: {side}_block_out_channels = {ch}: the shortcut between widths {a} and {b} needs 4 x {a} / {b} "
                                     f"and 4 x {b} / {a} to be integers")
            if ch[-1] % c.latent_channels:
                raise ValueError(f"AutoencoderDC: {side}_block_out_channels[-1] = {ch[-1]} is not a multiple of latent_channels = {c.latent_channels}")

    @property
    def spatial_factor(self) -> int:
        return 2 ** (len(self.config.encoder_block_out_channels) - 1)

    # ------------------------------------------------------------------ diffusers' keys --------------------------------
    def _block_keys(self, e: dict, p: str, kind: str, C: int, scales: tuple) -> None:
        if kind == "ResBlock":
            e[p + ".conv1.weight"], e[p + ".conv1.bias"] = (C, C, 3, 3), (C,)
            e[p + ".conv2.weight"] = (C, C, 3, 3)
            e[p + ".norm.weight"], e[p + ".norm.bias"] = (C,), (C,)
            return
        for n in ("to_q", "to_k", "to_v"):
            e[f"{p}.attn.{n}.weight"] = (C, C)
        for s, k in enumerate(scales):
            e[f"{p}.attn.to_qkv_multiscale.{s}.proj_in.weight"] = (3 * C, 1, k, k)
            e[f"{p}.attn.to_qkv_multiscale.{s}.proj_out.weight"] = (3 * C, DH, 1, 1)
        e[f"{p}.attn.to_out.weight"] = (C, C * (1 + len(scales)))
        e[f"{p}.attn.norm_out.weight"], e[f"{p}.attn.norm_out.bias"] = (C,), (C,)
        e[f"{p}.conv_out.conv_inverted.weight"], e[f"{p}.conv_out.conv_inverted.bias"] = (8 * C, C, 1, 1), (8 * C,)
        e[f"{p}.conv_out.conv_depth.weight"], e[f"{p}.conv_out.conv_depth.bias"] = (8 * C, 1, 3, 3), (8 * C,)
        e[f"{p}.conv_out.conv_point.weight"] = (C, 4 * C, 1, 1)
        e[f"{p}.conv_out.norm.weight"], e[f"{p}.conv_out.norm.bias"] = (C,), (C,)

    def _plan(self) -> Dict[str, List[tuple]]:
        """the modules in diffusers' order and under its names: side -> [(prefix, kind, ...)], kind in conv | ResBlock | EfficientViTBlock | down | up"""
        c = self.config
        enc: List[tuple] = []
        ch, layers, types, ms = c.encoder_block_out_channels, c.encoder_layers_per_block, c.encoder_block_types, c.encoder_qkv_multiscales
        n = len(ch)
        for i in range(n):
            for j in range(layers[i]):
                enc.append((f"encoder.down_blocks.{i}.{j}", types[i], ch[i], ms[i]))
            if i < n - 1:
                enc.append((f"encoder.down_blocks.{i}.{layers[i]}", "down", ch[i], ch[i + 1]))
        ch, layers, types, ms = c.decoder_block_out_channels, c.decoder_layers_per_block, c.decoder_block_types, c.decoder_qkv_multiscales
        stages: List[List[tuple]] = []                   # up_blocks[i] is stage i, the up block first inside a stage
        for i in range(n):
            up = [(f"decoder.up_blocks.{i}.0", "up", ch[i + 1], ch[i])] if i < n - 1 else []
            stages.append(up + [(f"decoder.up_blocks.{i}.{j + len(up)}", types[i], ch[i], ms[i]) for j in range(layers[i])])
        dec = [e for st in reversed(stages) for e in st]   # the forward walks the stages from the last to the first
        return dict(encoder=enc, decoder=dec, decoder_by_stage=[e for st in stages for e in st])

    def expected_keys(self) -> Dict[str, Tuple[int, ...]]:
        c = self.config
        e: Dict[str, Tuple[int, ...]] = {}
        pu, ps = c.downsample_block_type == "pixel_unshuffle", c.upsample_block_type == "pixel_shuffle"

        def conv(p, cout, cin):
            e[p + ".weight"], e[p + ".bias"] = (cout, cin, 3, 3), (cout,)
        plan = self._plan()
        conv("encoder.conv_in", c.encoder_block_out_channels[0], c.in_channels)
        for p, kind, a, b in plan["encoder"]:
            if kind == "down":
                conv(p + ".conv", b // 4 if pu else b, a)
            else:
                self._block_keys(e, p, kind, a, b)
        conv("encoder.conv_out", c.latent_channels, c.encoder_block_out_channels[-1])
        conv("decoder.conv_in", c.decoder_block_out_channels[-1], c.latent_channels)
        for p, kind, a, b in plan["decoder_by_stage"]:   # diffusers registers up_blocks in stage order
            if kind == "up":
                conv(p + ".conv", b * 4 if ps else b, a)
            else:
                self._block_keys(e, p, kind, a, b)
        e["decoder.norm_out.weight"], e["decoder.norm_out.bias"] = (c.decoder_block_out_channels[0],), (c.decoder_block_out_channels[0],)
        conv("decoder.conv_out", c.in_channels, c.decoder_block_out_channels[0])
        return e

    def set_trainable(self, patterns=True):
        raise NotImplementedError(f"AutoencoderDC: no backward is implemented; it is {OPEN}")

    def init_synthetic_(self, seed: int = 0) -> "AutoencoderDC":
        """Seeded weights for tests and benchmarks, drawn on the model's device: weights N(0, 1 / fan_in), biases 0.1 N, norm weights 1 + 0.1 N."""
        g = torch.Generator(device=self._device).manual_seed(seed)
        sd = {}
        for k, shape in self.expected_keys().items():
            t = torch.randn(shape, generator=g, device=self._device)
            if k.endswith(".bias"):
                t = 0.1 * t
            elif ".norm" in k:
                t = 1 + 0.1 * t
            else:
                t = t / float(max(1, t[0].numel())) ** 0.5
            sd[k] = t.to(self._dtype)
        self.load_state_dict(sd)
        return self

    @classmethod
    def from_config(cls, config: dict, **kw) -> "AutoencoderDC":
        return cls(config, **kw)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: Optional[str] = None, torch_dtype=BF, device=None) -> "AutoencoderDC":
        """A local directory only (no hub access): config.json + *.safetensors (diffusers layout: <model>/vae/)."""
        path = os.fspath(pretrained_model_name_or_path)
        if subfolder:
            path = os.path.join(path, subfolder)
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local directory (this package does not download checkpoints)")
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        from safetensors.torch import load_file
        m = cls(cfg, device=device, dtype=torch_dtype)
        sd = {}
        for fn in sorted(f for f in os.listdir(path) if f.endswith(".safetensors")):
            sd.update(load_file(os.path.join(path, fn)))
        if not sd:
            raise OSError(f"no *.safetensors weights under {path}")
        m.load_state_dict(sd)
        return m

    # ------------------------------------------------------------------ load-time layouts ------------------------------
    def _builders(self) -> Dict[str, tuple]:
        s = self._sd
        z = lambda *shape: torch.zeros(*shape, dtype=self._dtype, device=self._device)
        b: Dict[str, tuple] = {}

        def conv(name):
            """[Cout, Cin, 3, 3] -> [Cout_p, 3, 3, Cin_p] (+ bias [Cout_p]): Cin zero-padded to the convolution's K granularity (64), Cout to 8"""
            def w():
                t = s[name + ".weight"]
                out = z(_pad(t.shape[0], 8), 3, 3, _pad(t.shape[1], 64))
                out[:t.shape[0], :, :, :t.shape[1]] = t.permute(0, 2, 3, 1)
                return out
            b[name + ".w"] = ([name + ".weight"], w)
            if name + ".bias" in s:
                def bias():
                    t = s[name + ".bias"]
                    out = z(_pad(t.shape[0], 8))
                    out[:t.shape[0]] = t
                    return out
                b[name + ".b"] = ([name + ".bias"], bias)

        def blocks32(t, heads):
            """a tensor whose first axis is the 3 C channels of [to_q | to_k | to_v] in diffusers' order: 32-block 3 g + part -> part * heads + g"""
            return t.reshape(heads, 3, DH, -1).permute(1, 0, 2, 3).reshape(3 * heads * DH, -1)

        def evit(p, C, scales):
            heads = C // DH
            names = [f"{p}.attn.{n}.weight" for n in ("to_q", "to_k", "to_v")]
            b[p + ".qkv_w"] = (names, lambda: blocks32(torch.cat([s[k] for k in names], 0), heads).contiguous())
            for i, k in enumerate(scales):
                pin, pout = f"{p}.attn.to_qkv_multiscale.{i}.proj_in.weight", f"{p}.attn.to_qkv_multiscale.{i}.proj_out.weight"
                b[f"{p}.ms{i}_dw"] = ([pin], lambda pin=pin: blocks32(s[pin], heads).t().contiguous())                      # [k k][3 C], tap ky k + kx major
                b[f"{p}.ms{i}_pw"] = ([pout], lambda pout=pout: blocks32(s[pout], heads).reshape(3 * heads, DH, DH).contiguous())   # [G][32 out][32 in]
            b[p + ".inv_w"] = ([], lambda: s[p + ".conv_out.conv_inverted.weight"].reshape(8 * C, C))                 # a view
            b[p + ".dw_w"] = ([p + ".conv_out.conv_depth.weight"], lambda: s[p + ".conv_out.conv_depth.weight"].reshape(8 * C, 9).t().contiguous())
            b[p + ".pt_w"] = ([], lambda: s[p + ".conv_out.conv_point.weight"].reshape(C, 4 * C))                     # a view

        plan = self._plan()
        for name in ("encoder.conv_in", "encoder.conv_out", "decoder.conv_in", "decoder.conv_out"):
            conv(name)
        for side in ("encoder", "decoder"):
            for p, kind, a, c2 in plan[side]:
                if kind in ("down", "up"):
                    conv(p + ".conv")
                elif kind == "ResBlock":
                    conv(p + ".conv1")
                    conv(p + ".conv2")
                else:
                    evit(p, a, c2)
        return b

    # ------------------------------------------------------------------ blocks -----------------------------------------
    def _g(self, bufs, name: str, rows: int, cols: int, dtype=None) -> torch.Tensor:
        return self._get(bufs, f"{name}:{rows}x{cols}", (rows, cols), dtype=dtype)

    def _main(self, bufs, rows: int, cols: int, *avoid) -> torch.Tensor:
        """a block's output buffer: one of three per shape, none of `avoid` (the tensors still to be read)"""
        taken = {a.data_ptr() for a in avoid if a is not None}
        for t in ("m0", "m1", "m2"):
            buf = self._g(bufs, t, rows, cols)
            if buf.data_ptr() not in taken:
                return buf
        raise AssertionError("three buffers, at most two taken")

    def _conv(self, bufs, name: str, x: torch.Tensor, B: int, H: int, W: int, out: Optional[torch.Tensor] = None, tag: str = "cv", *, stride: int = 1, up: int = 0,
              residual: Optional[torch.Tensor] = None):
        """3x3 convolution, padding 1, on NHWC rows -> (out [B*Ho*Wo, Cout_p], Ho, Wo); up = 1: nearest 2x folded into the gather"""
        wp, bp = self._p[name + ".w"], self._p.get(name + ".b")
        Hv, Wv = H << up, W << up
        Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
        assert x.shape[1] == wp.shape[3], (name, tuple(x.shape), tuple(wp.shape))
        if out is None:
            out = self._g(bufs, tag, B * Ho * Wo, wp.shape[0])
        ops.conv2d_nhwc(x, wp, bp, out, B=B, H=H, W=W, Ho=Ho, Wo=Wo, KH=3, KW=3, stride=stride, pad_t=1, pad_l=1, up=up, residual=residual)
        return out, Ho, Wo

    def _norm(self, p: str, x: torch.Tensor, *, residual=None, relu=False, out=None) -> torch.Tensor:
        return ops.rmsnorm_bias_rows(x, self._sd[p + ".weight"], self._sd[p + ".bias"], NORM_EPS, residual=residual, relu=relu, out=out)

    def _resblock(self, bufs, p: str, x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        h, _, _ = self._conv(bufs, p + ".conv1", x, B, H, W, tag="rb")
        ops.silu(h, h)
        out = self._main(bufs, x.shape[0], x.shape[1], x)
        self._conv(bufs, p + ".conv2", h, B, H, W, out=out)
        return self._norm(p + ".norm", out, residual=x, out=out)

    def _evit(self, bufs, p: str, x: torch.Tensor, B: int, H: int, W: int, scales: tuple) -> torch.Tensor:
        s, P = self._sd, self._p
        M, C = x.shape
        heads, N, S1 = C // DH, H * W, 1 + len(scales)
        ld = 3 * C * S1
        # SanaMultiscaleLinearAttention: [Q | K | V] of every scale side by side, heads of 32 in the kernel's layout (module docstring)
        qkv = self._g(bufs, "qkv", M, ld)
        ops.gemm(x, P[p + ".qkv_w"], None, qkv, M=M)
        for i, k in enumerate(scales):
            ops.msconv_proj(qkv, P[f"{p}.ms{i}_dw"], P[f"{p}.ms{i}_pw"], qkv[:, (i + 1) * 3 * C:], B=B, H=H, W=W, G=3 * heads, k=k)
        att = self._g(bufs, "att", M, C * S1)
        ws = self._get(bufs, f"la_ws:{B}x{heads}x{N}", (ops.linear_attn_workspace_bytes(B, heads, N),), dtype=torch.uint8)
        st = (ld, N * ld)
        for i in range(S1):
            t = qkv[:, i * 3 * C:]
            ops.linear_attn(t, t[:, C:], t[:, 2 * C:], att[:, i * C:], batches=B, heads=heads, N=N, q_strides=st, k_strides=st, v_strides=st,
                            o_strides=(C * S1, N * C * S1), workspace=ws)
        y = self._main(bufs, M, C, x)
        ops.gemm(att, s[p + ".attn.to_out.weight"], None, y, M=M)
        self._norm(p + ".attn.norm_out", y, residual=x, out=y)
        # GLUMBConv, expand ratio 4
        u = ops.gemm(y, P[p + ".inv_w"], s[p + ".conv_out.conv_inverted.bias"], self._g(bufs, "u", M, 8 * C), M=M)
        glu = ops.glu_dwconv3x3(u, P[p + ".dw_w"], s[p + ".conv_out.conv_depth.bias"], self._g(bufs, "glu", M, 4 * C), B=B, H=H, W=W, C=4 * C)
        out = self._main(bufs, M, C, y)
        ops.gemm(glu, P[p + ".pt_w"], None, out, M=M)
        return self._norm(p + ".conv_out.norm", out, residual=y, out=out)

    def _down(self, bufs, p: str, x: torch.Tensor, B: int, H: int, W: int, cin: int, cout: int):
        Mo = B * (H // 2) * (W // 2)
        out = self._main(bufs, Mo, cout)
        if self.config.downsample_block_type == "pixel_unshuffle":
            cv, _, _ = self._conv(bufs, p + ".conv", x, B, H, W, tag="dn")
            ops.dc_shortcut(x, out, up=False, B=B, H=H, W=W, Cin=cin, Cout=cout, factor=2, x=cv, x_shuffle=True)
        else:
            y = ops.dc_shortcut(x, self._g(bufs, "sc", Mo, cout), up=False, B=B, H=H, W=W, Cin=cin, Cout=cout, factor=2)
            self._conv(bufs, p + ".conv", x, B, H, W, out=out, stride=2, residual=y)
        return out, H // 2, W // 2

    def _up(self, bufs, p: str, x: torch.Tensor, B: int, H: int, W: int, cin: int, cout: int):
        Mo = B * H * W * 4
        out = self._main(bufs, Mo, cout)
        if self.config.upsample_block_type == "pixel_shuffle":
            cv, _, _ = self._conv(bufs, p + ".conv", x, B, H, W, tag="up")
            ops.dc_shortcut(x, out, up=True, B=B, H=H, W=W, Cin=cin, Cout=cout, factor=2, x=cv, x_shuffle=True)
        else:
            y = ops.dc_shortcut(x, self._g(bufs, "sc", Mo, cout), up=True, B=B, H=H, W=W, Cin=cin, Cout=cout, factor=2)
            self._conv(bufs, p + ".conv", x, B, H, W, out=out, up=1, residual=y)
        return out, 2 * H, 2 * W

    def _stages(self, bufs, side: str, x: torch.Tensor, B: int, H: int, W: int):
        for p, kind, a, b in self._plan_cache[side]:
            if kind == "down":
                x, H, W = self._down(bufs, p, x, B, H, W, a, b)
            elif kind == "up":
                x, H, W = self._up(bufs, p, x, B, H, W, a, b)
            elif kind == "ResBlock":
                x = self._resblock(bufs, p, x, B, H, W)
            else:
                x = self._evit(bufs, p, x, B, H, W, b)
        return x, H, W

    def _pack(self) -> None:
        super()._pack()
        self._plan_cache = self._plan()

    def _ready(self, t: torch.Tensor, channels: int, what: str) -> torch.Tensor:
        if not self._p:
            raise RuntimeError("AutoencoderDC: load_state_dict first")
        if t.dim() != 4 or t.shape[1] != channels:
            raise ValueError(f"AutoencoderDC: {what} must be [B, {channels}, H, W], got {tuple(t.shape)}")
        return t.detach().to(self._device, self._dtype).contiguous()

    # ------------------------------------------------------------------ encode / decode --------------------------------
    @torch.no_grad()
    def _encode(self, image: torch.Tensor) -> torch.Tensor:
        c = self.config
        image = self._ready(image, c.in_channels, "the image")
        B, _, H, W = image.shape
        f = self.spatial_factor
        if H % f or W % f or H < f or W < f:
            raise ValueError(f"AutoencoderDC.encode: image sides {H} x {W} must be multiples of the spatial factor {f}")
        bufs = self._buffers(("enc", B, H, W))
        x = ops.nchw_to_nhwc(image, _pad(c.in_channels, 64))
        x, _, _ = self._conv(bufs, "encoder.conv_in", x, B, H, W, out=self._main(bufs, B * H * W, c.encoder_block_out_channels[0]))
        x, H, W = self._stages(bufs, "encoder", x, B, H, W)
        # conv_out(x) + the mean over groups of C / latent channels
        y = ops.dc_shortcut(x, self._g(bufs, "lat_sc", B * H * W, c.latent_channels), up=False, B=B, H=H, W=W, Cin=x.shape[1], Cout=c.latent_channels, factor=1)
        z, _, _ = self._conv(bufs, "encoder.conv_out", x, B, H, W, tag="lat", residual=y)
        return ops.nhwc_to_nchw(z, B, c.latent_channels, H, W)

    @torch.no_grad()
    def _decode(self, z: torch.Tensor) -> torch.Tensor:
        c = self.config
        z = self._ready(z, c.latent_channels, "the latents")
        B, Lc, H, W = z.shape
        bufs = self._buffers(("dec", B, H, W))
        C = c.decoder_block_out_channels[-1]
        zr = ops.nchw_to_nhwc(z, _pad(Lc, 64))
        # conv_in(z) + every latent channel C / latent times over
        y = ops.dc_shortcut(zr, self._g(bufs, "in_sc", B * H * W, C), up=True, B=B, H=H, W=W, Cin=Lc, Cout=C, factor=1)
        x, _, _ = self._conv(bufs, "decoder.conv_in", zr, B, H, W, out=self._main(bufs, B * H * W, C), residual=y)
        x, H, W = self._stages(bufs, "decoder", x, B, H, W)
        self._norm("decoder.norm_out", x, relu=True, out=x)
        img, _, _ = self._conv(bufs, "decoder.conv_out", x, B, H, W, tag="img")
        return ops.nhwc_to_nchw(img, B, c.in_channels, H, W)

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        latent = self._encode(x)
        return SimpleNamespace(latent=latent) if return_dict else (latent,)

    def decode(self, z: torch.Tensor, return_dict: bool = True):
        sample = self._decode(z)
        return SimpleNamespace(sample=sample) if return_dict else (sample,)

    def forward(self, sample: torch.Tensor, return_dict: bool = True):
        return self.decode(self.encode(sample).latent, return_dict=return_dict)

    __call__ = forward
