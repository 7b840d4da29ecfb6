"""Sana text-to-image: DPMSolverMultistepScheduler as Sana configures it, the denoise loop and SanaPipeline.

The parts are the package's own: SanaTransformer2DModel (sana.py), Gemma2Model + encode_prompt_sana (gemma.py), AutoencoderDC (dcae.py) and
VaeImageProcessor (image.py). What this module adds is the host side of the scheduler and the loop; the per-step arithmetic - classifier-free guidance,
the flow-to-x0 conversion, the first- or second-order DPM-Solver++ update, the two-step history and the next forward's input - is ONE launch of
ug_dpm_step (csrc/sched.hip) on fp32 latents. With fp32 components the same code runs ug_dpm_step_f32.

Restated from the published source of diffusers 0.32.2 (schedulers/scheduling_dpmsolver_multistep.py, pipelines/sana/pipeline_sana.py); diffusers is
not a dependency, so parity with it is not pinned by a test (docs/PARITY_TOLERANCES.md, "Sana pipeline"): the formulas in the docstrings below are
the specification, and tests/sana_pipeline_ref.py restates them in float64.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

BF, F32 = torch.bfloat16, torch.float32
FOLLOW_UP = "a follow-up (docs/NEXT_ROWS.md)"

# what Sana's published scheduler_config.json sets on top of diffusers' defaults
SANA_SCHEDULER_CONFIG = dict(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", prediction_type="flow_prediction", use_flow_sigmas=True,
                             flow_shift=3.0, final_sigmas_type="zero", lower_order_final=True)


class DPMSolverMultistepScheduler:
    """diffusers' DPMSolverMultistepScheduler for the one combination Sana uses: dpmsolver++, midpoint, solver_order 1 or 2, flow prediction on flow
    sigmas, a final sigma of zero. Config names and defaults are diffusers'; every other combination raises NotImplementedError naming itself.

    set_timesteps(n), in numpy float64: alphas = linspace(1, 1 / T, n + 1); s = 1 - alphas; s = flip(shift s / (1 + (shift - 1) s))[:-1];
    timesteps = int64(s T) (truncating); sigmas = float32(concat(s, [0])).
    Step i (s0 = sigmas[i], t = sigmas[i + 1], s1 = sigmas[i - 1]; alpha = 1 - sigma, lambda = log(alpha) - log(sigma), all on 0-dim fp32 tensors as
    diffusers forms them): h = lambda_t - lambda_s0, a = sigma_t / sigma_s0, b = alpha_t (exp(-h) - 1), rinv = 1 / ((lambda_s0 - lambda_s1) / h);
        x0 = sample - s0 model_output;   first order: a sample - b x0;   second (midpoint): ... - (0.5 b) (rinv (x0 - x0 of the step before)).
    The first step and the last are first order; the last has sigma_t = 0, so h = inf, b = -1 and the result is x0."""

    DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None, solver_order=2,
                    prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                    solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False, use_exponential_sigmas=False,
                    use_beta_sigmas=False, use_lu_lambdas=False, use_flow_sigmas=False, flow_shift=1.0, final_sigmas_type="zero",
                    lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False)
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **config):
        c = dict(self.DEFAULTS)
        unknown = sorted(k for k in config if k not in c and not k.startswith("_"))       # diffusers writes "_class_name", "_diffusers_version"
        if unknown:
            raise ValueError(f"DPMSolverMultistepScheduler: config keys {unknown} are not known to this class; nothing is ignored silently")
        c.update({k: v for k, v in config.items() if k in c})
        who = "DPMSolverMultistepScheduler"

        def refuse(what):
            raise NotImplementedError(f"{who}: {what} is not implemented: this class serves Sana's configuration (dpmsolver++, midpoint, solver_order 1 or 2, "
                                      f"flow_prediction, use_flow_sigmas, final_sigmas_type 'zero'); the rest is {FOLLOW_UP}")
        for k in ("use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas", "use_lu_lambdas", "thresholding", "euler_at_final"):
            if c[k]:
                refuse(f"{k} = True")
        if c["algorithm_type"] != "dpmsolver++":
            refuse(f"algorithm_type = {c['algorithm_type']!r} (the SDE variants and dpmsolver)")
        if c["solver_order"] not in (1, 2):
            refuse(f"solver_order = {c['solver_order']}")
        if c["solver_type"] != "midpoint":
            refuse(f"solver_type = {c['solver_type']!r}")
        if c["prediction_type"] != "flow_prediction":
            refuse(f"prediction_type = {c['prediction_type']!r}")
        if not c["use_flow_sigmas"]:
            refuse("use_flow_sigmas = False (the beta schedule's sigmas)")
        if c["final_sigmas_type"] != "zero":
            refuse(f"final_sigmas_type = {c['final_sigmas_type']!r}")
        if not c["lower_order_final"]:
            refuse("lower_order_final = False")
        if c["variance_type"] is not None:
            refuse(f"variance_type = {c['variance_type']!r}")
        if int(c["num_train_timesteps"]) < 2 or float(c["flow_shift"]) <= 0:
            raise ValueError(f"{who}: num_train_timesteps = {c['num_train_timesteps']}, flow_shift = {c['flow_shift']}")
        self.config = SimpleNamespace(**c)
        self.timesteps: Optional[torch.Tensor] = None
        self.sigmas: Optional[torch.Tensor] = None
        self.num_inference_steps: Optional[int] = None
        self._coef: List[Tuple[int, float, float, float, float]] = []
        self._reset()

    @classmethod
    def from_config(cls, config, **kwargs) -> "DPMSolverMultistepScheduler":
        c = dict(vars(config)) if isinstance(config, SimpleNamespace) else dict(config)
        c.update(kwargs)
        return cls(**c)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: Optional[str] = None, **kwargs) -> "DPMSolverMultistepScheduler":
        """A local directory holding scheduler_config.json (diffusers layout: <model>/scheduler/), or that file itself."""
        path = os.fspath(pretrained_model_name_or_path)
        if subfolder:
            path = os.path.join(path, subfolder)
        if os.path.isdir(path):
            path = os.path.join(path, "scheduler_config.json")
        if not os.path.isfile(path):
            raise OSError(f"{path} is not a local scheduler_config.json (this package does not download checkpoints)")
        with open(path) as f:
            return cls.from_config(json.load(f), **kwargs)

    def _reset(self) -> None:
        self._step_index: Optional[int] = None
        self._x0_prev: Optional[torch.Tensor] = None
        self.lower_order_nums = 0

    step_index = property(lambda self: self._step_index)

    def set_timesteps(self, num_inference_steps: int, device=None, timesteps=None, sigmas=None) -> None:
        if timesteps is not None or sigmas is not None:
            raise NotImplementedError(f"DPMSolverMultistepScheduler.set_timesteps: custom timesteps / sigmas are not implemented; they are {FOLLOW_UP}")
        n = int(num_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps = {num_inference_steps}")
        c = self.config
        T, shift = int(c.num_train_timesteps), float(c.flow_shift)
        s = 1.0 - np.linspace(1, 1 / T, n + 1)
        s = np.flip(shift * s / (1 + (shift - 1) * s))[:-1].copy()
        self.timesteps = torch.from_numpy((s * T).astype(np.int64)).to(device)
        self.sigmas = torch.from_numpy(np.concatenate([s, [0.0]]).astype(np.float32))            # on the host, as diffusers keeps them
        self.num_inference_steps = n
        self._coef = [self._coefficients(i) for i in range(n)]
        self._reset()

    def _coefficients(self, i: int) -> Tuple[int, float, float, float, float]:
        """(order, sigma_s0, a, b, rinv) of step i: elements of the fp32 sigma tensor and 0-dim fp32 tensor ops, each rounded as diffusers rounds it
        (the trick of pipeline._step32); what reaches the kernel are those fp32 values."""
        sg, n = self.sigmas, self.num_inference_steps
        lam = lambda s: torch.log(1 - s) - torch.log(s)
        s0, st = sg[i], sg[i + 1]
        h = lam(st) - lam(s0)
        a, b = st / s0, (1 - st) * (torch.exp(-h) - 1.0)
        order = 1 if (i == 0 or i == n - 1 or self.config.solver_order == 1) else 2
        rinv = 1.0 / ((lam(s0) - lam(sg[i - 1])) / h) if order == 2 else torch.tensor(0.0)
        return order, float(s0), float(a), float(b), float(rinv)

    def scale_model_input(self, sample: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        return sample

    def index_for_timestep(self, timestep) -> int:
        """diffusers' rule: the second of several equal timesteps (so that a schedule entered in the middle does not skip a sigma), the last when none matches"""
        hits = (self.timesteps == int(timestep)).nonzero().flatten().tolist()
        return len(self.timesteps) - 1 if not hits else hits[1 if len(hits) > 1 else 0]

    def fused_step(self, pred_uncond: torch.Tensor, pred_text: Optional[torch.Tensor], guidance_scale: float, sample: torch.Tensor,
                   model_in: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Step `step_index` (0 after set_timesteps) through ug_dpm_step: guidance when `pred_text` is given, `sample` (fp32) updated in place, `model_in`
        ([copies, *sample.shape] in the predictions' dtype) filled with the new sample. No host synchronisation; the history buffer is allocated at
        the first step."""
        if not self._coef:
            raise RuntimeError("DPMSolverMultistepScheduler: call set_timesteps first")
        if sample.dtype != F32:
            raise TypeError(f"DPMSolverMultistepScheduler.step: the sample must be torch.float32 (the scheduler's arithmetic is fp32 on fp32 latents), got {sample.dtype}")
        i = self._step_index or 0
        if i >= len(self._coef):
            raise IndexError(f"DPMSolverMultistepScheduler: step {i + 1} of {len(self._coef)}; call set_timesteps to start again")
        order, sigma, a, b, rinv = self._coef[i]
        if self._x0_prev is None:                        # no history yet (also a schedule entered in the middle): first order, diffusers' lower_order_nums < 1
            self._x0_prev, order = torch.empty_like(sample, memory_format=torch.contiguous_format), 1
        elif self._x0_prev.shape != sample.shape or self._x0_prev.device != sample.device:
            raise RuntimeError("DPMSolverMultistepScheduler: the sample's shape or device changed between steps; call set_timesteps to start again")
        ops.dpm_step(pred_uncond, pred_text, float(guidance_scale), sample, self._x0_prev, model_in, order=order, sigma=sigma, a=a, b=b, rinv=rinv)
        self._step_index = i + 1
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        return sample

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, variance_noise=None, return_dict: bool = True):
        """diffusers' signature. `sample` must be a contiguous fp32 GPU tensor: it is updated in place and returned as `prev_sample`; `model_output` is
        bf16 or fp32. The first call after set_timesteps starts at `timestep`'s index."""
        if self._step_index is None and self.timesteps is not None:
            self._step_index = self.index_for_timestep(timestep)
        if not sample.is_contiguous():
            raise ValueError("DPMSolverMultistepScheduler.step: the sample must be contiguous (it is updated in place)")
        prev = self.fused_step(model_output.contiguous(), None, 1.0, sample)
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)


@dataclass
class SanaPipelineOutput:
    images: Any


def _fill_model_input(model_in: torch.Tensor, latents: torch.Tensor) -> None:
    """`torch.cat([latents] * copies).to(dtype)` into the standing buffer"""
    B = latents.shape[0]
    for k in range(model_in.shape[0] // B):
        model_in[k * B:(k + 1) * B].copy_(latents)


@torch.no_grad()
def sana_denoise_loop(transformer, scheduler: DPMSolverMultistepScheduler, *, latents: torch.Tensor, prompt_embeds: torch.Tensor,
                      prompt_attention_mask: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      negative_prompt_attention_mask: Optional[torch.Tensor] = None, num_inference_steps: int = 20, guidance_scale: float = 4.5,
                      callback_on_step_end=None, callback_on_step_end_tensor_inputs: Sequence[str] = ("latents",), pipeline=None) -> torch.Tensor:
    """SanaPipeline.__call__'s loop (pipeline_sana.py, "Denoising loop") on fp32 latents [B, C, h, w], updated in place and returned.

    With guidance_scale > 1 the prompt rows are cat([negative, positive]) (the masks likewise) and the model input is ONE standing buffer [2 B, C, h, w] in
    the transformer's dtype, [B, ...] without guidance (one forward per step, pred_text = NULL). It is filled once before the loop; afterwards only
    ug_dpm_step writes it - the kernel's model_in store is the reference's `torch.cat([latents] * 2).to(dtype)` of the next step. The timestep is
    `t.expand(rows)` as fp32. A transformer with out_channels // 2 == latent channels predicts a variance beside the flow (learned sigma): its first
    half of the channels is kept, through one contiguous copy into a standing buffer. After the first step the loop makes no host synchronisation and
    allocates nothing of its own. `callback_on_step_end(pipeline, i, t, {name: tensor})` may return replacements for `latents` (the model input is
    then filled again from them), `prompt_embeds` and `negative_prompt_embeds`."""
    dev, dt = latents.device, transformer.dtype
    if latents.dtype != F32 or latents.dim() != 4:
        raise TypeError(f"sana_denoise_loop: latents must be torch.float32 [B, C, h, w], got {latents.dtype} {tuple(latents.shape)}")
    cfg_on = guidance_scale > 1.0
    if cfg_on and negative_prompt_embeds is None:
        raise ValueError("sana_denoise_loop: guidance_scale > 1 needs negative_prompt_embeds")
    latents = latents.contiguous()
    B, C = latents.shape[:2]
    tc = transformer.config
    out_channels = tc["out_channels"] if isinstance(tc, dict) else tc.out_channels
    learned_sigma = out_channels // 2 == C
    if not learned_sigma and out_channels != C:
        raise ValueError(f"sana_denoise_loop: the transformer predicts {out_channels} channels for latents of {C}")

    def rows(neg, pos):
        if pos is None or not cfg_on:
            return pos
        if neg is None:
            raise ValueError("sana_denoise_loop: a prompt_attention_mask under guidance needs a negative_prompt_attention_mask")
        return torch.cat([neg.to(dev), pos.to(dev)], 0)
    embeds = rows(negative_prompt_embeds, prompt_embeds.to(dev)).to(dt).contiguous()
    mask = rows(negative_prompt_attention_mask, None if prompt_attention_mask is None else prompt_attention_mask.to(dev))
    copies = 2 if cfg_on else 1
    if embeds.shape[0] != copies * B:
        raise ValueError(f"sana_denoise_loop: {embeds.shape[0]} prompt rows for {copies} x {B} model inputs")
    scheduler.set_timesteps(num_inference_steps, device=dev)
    # one row of `t.expand(rows)` per step, made before the loop: the forward wants a contiguous fp32 vector
    t_rows = scheduler.timesteps.to(device=dev, dtype=F32)[:, None].expand(num_inference_steps, copies * B).contiguous()
    model_in = torch.empty((copies * B,) + tuple(latents.shape[1:]), dtype=dt, device=dev)
    _fill_model_input(model_in, latents)
    kept = torch.empty_like(model_in) if learned_sigma else None
    for i in range(num_inference_steps):
        pred = transformer(model_in, encoder_hidden_states=embeds, timestep=t_rows[i], encoder_attention_mask=mask)
        if isinstance(pred, (tuple, list)):
            pred = pred[0]
        if learned_sigma:
            kept.copy_(pred[:, :C])                     # noise_pred.chunk(2, dim=1)[0]
            pred = kept
        elif not pred.is_contiguous():
            pred = pred.contiguous()
        scheduler.fused_step(pred[:B], pred[B:] if cfg_on else None, guidance_scale, latents, model_in)
        if callback_on_step_end is not None:
            have = dict(latents=latents, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, noise_pred=pred, timestep=t_rows[i])
            outs = callback_on_step_end(pipeline, i, scheduler.timesteps[i], {k: have[k] for k in callback_on_step_end_tensor_inputs}) or {}
            if "latents" in outs:
                new = outs["latents"]
                if new is not latents:
                    latents = new.to(device=dev, dtype=F32).contiguous()
                _fill_model_input(model_in, latents)      # the kernel's store held the step's own result
            if "prompt_embeds" in outs or "negative_prompt_embeds" in outs:
                prompt_embeds = outs.get("prompt_embeds", prompt_embeds)
                negative_prompt_embeds = outs.get("negative_prompt_embeds", negative_prompt_embeds)
                embeds = rows(negative_prompt_embeds, prompt_embeds.to(dev)).to(dt).contiguous()
    return latents


class SanaPipeline:
    """diffusers' SanaPipeline on the package's components: SanaPipeline(tokenizer, text_encoder, vae, transformer, scheduler), `from_pretrained` of a
    local directory, `to`, and `__call__` with diffusers' keywords. Without a tokenizer a prompt is the pair (token ids, attention mask), each
    [B, length], or the caller passes `prompt_embeds`."""

    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler: Optional[DPMSolverMultistepScheduler] = None):
        self.tokenizer, self.text_encoder, self.vae, self.transformer = tokenizer, text_encoder, vae, transformer
        self.scheduler = scheduler if scheduler is not None else DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
        self.vae_scale_factor = vae.spatial_factor if vae is not None and hasattr(vae, "spatial_factor") else 32
        from .image import VaeImageProcessor
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=BF, device=None, **kwargs) -> "SanaPipeline":
        """A local diffusers directory: transformer/, text_encoder/, vae/, scheduler/scheduler_config.json, each read by its component's own
        from_pretrained; tokenizer/ through transformers.AutoTokenizer when that package imports and the directory exists, else tokenizer = None.
        A component passed as a keyword is taken as it is."""
        root = os.fspath(pretrained_model_name_or_path)
        if not os.path.isdir(root):
            raise OSError(f"{root} is not a local directory (this package does not download checkpoints)")
        unknown = sorted(set(kwargs) - {"tokenizer", "text_encoder", "vae", "transformer", "scheduler"})
        if unknown:
            raise TypeError(f"SanaPipeline.from_pretrained: unknown arguments {unknown}")
        from .dcae import AutoencoderDC
        from .gemma import Gemma2Model
        from .sana import SanaTransformer2DModel
        sub = lambda name: os.path.join(root, name)
        tokenizer = kwargs.get("tokenizer")
        if tokenizer is None and os.path.isdir(sub("tokenizer")):
            try:
                from transformers import AutoTokenizer
            except ImportError:
                AutoTokenizer = None
            if AutoTokenizer is not None:
                tokenizer = AutoTokenizer.from_pretrained(sub("tokenizer"), local_files_only=True)
                tokenizer.padding_side = "right"
        return cls(tokenizer=tokenizer,
                   text_encoder=kwargs.get("text_encoder") or Gemma2Model.from_pretrained(sub("text_encoder"), device=device, dtype=torch_dtype),
                   vae=kwargs.get("vae") or AutoencoderDC.from_pretrained(sub("vae"), torch_dtype=torch_dtype, device=device),
                   transformer=kwargs.get("transformer") or SanaTransformer2DModel.from_pretrained(sub("transformer"), device=device, dtype=torch_dtype),
                   scheduler=kwargs.get("scheduler") or DPMSolverMultistepScheduler.from_pretrained(sub("scheduler")))

    def to(self, device=None, dtype=None) -> "SanaPipeline":
        """The components load onto their device in their dtype (from_pretrained(device=, torch_dtype=)); one that has a `to` of its own is moved, any other
        must already be there."""
        for name in ("text_encoder", "vae", "transformer"):
            m = getattr(self, name)
            if m is None:
                continue
            if hasattr(m, "to"):
                m.to(device=device, dtype=dtype)
            elif (device is not None and torch.device(device).type != m.device.type) or (dtype is not None and dtype != m.dtype):
                raise NotImplementedError(f"SanaPipeline.to: the {name} ({type(m).__name__}) lives on {m.device} in {m.dtype} and has no to(); load it there: "
                                          f"from_pretrained(dir, torch_dtype=, device=)")
        return self

    device = property(lambda self: self.transformer.device)

    def _encode(self, what: str, prompt, embeds, mask, n_img: int, max_sequence_length: int, instruction):
        """prompt text (with a tokenizer), a (token ids, attention mask) pair, or ready embeds -> (embeds, mask), each prompt's images adjacent"""
        if embeds is not None:
            if n_img > 1:
                embeds = embeds.repeat_interleave(n_img, 0)
                mask = None if mask is None else mask.repeat_interleave(n_img, 0)
            return embeds, mask
        if self.text_encoder is None:
            raise ValueError(f"SanaPipeline: `{what}` needs a text encoder; pass `{what}_embeds`")
        from .gemma import encode_prompt_sana
        if isinstance(prompt, (tuple, list)) and len(prompt) == 2 and all(isinstance(t, torch.Tensor) for t in prompt):
            return encode_prompt_sana(self.text_encoder, None, None, max_sequence_length, text_input_ids=prompt[0], attention_mask=prompt[1],
                                      num_images_per_prompt=n_img, device=self.device)
        if self.tokenizer is None:
            raise TypeError(f"SanaPipeline: no tokenizer is attached, so `{what}` must be the pair (token ids [B, length], attention mask [B, length]), "
                            f"or pass `{what}_embeds`")
        return encode_prompt_sana(self.text_encoder, self.tokenizer, prompt, max_sequence_length, complex_human_instruction=instruction,
                                  num_images_per_prompt=n_img, device=self.device)

    @torch.no_grad()
    def __call__(self, prompt=None, negative_prompt="", num_inference_steps: int = 20, timesteps=None, sigmas=None, guidance_scale: float = 4.5,
                 num_images_per_prompt: int = 1, height: int = 1024, width: int = 1024, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None, prompt_attention_mask: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
                 output_type: str = "pil", return_dict: bool = True, clean_caption: bool = False, use_resolution_binning: bool = False,
                 attention_kwargs=None, callback_on_step_end=None, callback_on_step_end_tensor_inputs: Sequence[str] = ("latents",),
                 max_sequence_length: int = 300, complex_human_instruction: Optional[List[str]] = None) -> Union[SanaPipelineOutput, Tuple]:
        """diffusers' keywords and defaults, with two deviations: `complex_human_instruction` defaults to None (the published default text is not
        restated in this package: pass its lines), and `use_resolution_binning` defaults to False - True needs the aspect-ratio bin tables and the
        resize-and-crop of the decoded image, which are a follow-up. `eta` acts only on DDIM schedulers and is ignored, as in diffusers."""
        if use_resolution_binning:
            raise NotImplementedError(f"SanaPipeline: use_resolution_binning = True (the aspect-ratio bin tables and the bilinear resize-and-crop of the decoded "
                                      f"image) is not implemented; it is {FOLLOW_UP}")
        if clean_caption:
            raise NotImplementedError(f"SanaPipeline: clean_caption = True (bs4 / ftfy caption cleaning) is not implemented; it is {FOLLOW_UP}")
        if timesteps is not None or sigmas is not None:
            raise NotImplementedError(f"SanaPipeline: custom timesteps / sigmas are not implemented; they are {FOLLOW_UP}")
        if attention_kwargs:
            raise NotImplementedError("SanaPipeline: attention_kwargs (the LoRA scale of diffusers' attention processors) are not implemented")
        if (prompt is None) == (prompt_embeds is None):
            raise ValueError("SanaPipeline: pass exactly one of `prompt` and `prompt_embeds`")
        f = self.vae_scale_factor
        if height % f or width % f:
            raise ValueError(f"SanaPipeline: height and width must be multiples of {f}, got {height} x {width}")
        if output_type != "latent" and self.vae is None:
            raise ValueError("SanaPipeline: output_type other than 'latent' needs a VAE")
        tr, dev = self.transformer, self.device
        cfg_on = guidance_scale > 1.0
        embeds, mask = self._encode("prompt", prompt, prompt_embeds, prompt_attention_mask, num_images_per_prompt, max_sequence_length, complex_human_instruction)
        neg, neg_mask = None, None
        if cfg_on:
            if negative_prompt_embeds is None and isinstance(negative_prompt, str):
                rows = embeds.shape[0] // num_images_per_prompt
                negative_prompt = [negative_prompt] * rows                                    # diffusers: one negative per prompt
            # the negative prompt never carries the instruction (diffusers: complex_human_instruction=False)
            neg, neg_mask = self._encode("negative_prompt", negative_prompt, negative_prompt_embeds, negative_prompt_attention_mask, num_images_per_prompt,
                                         max_sequence_length, None)
            if neg.shape != embeds.shape:
                raise ValueError(f"SanaPipeline: negative prompt embeds {tuple(neg.shape)} do not match the prompt's {tuple(embeds.shape)}")
        B = embeds.shape[0]
        C = tr.config["in_channels"] if isinstance(tr.config, dict) else tr.config.in_channels
        shape = (B, C, height // f, width // f)
        if latents is None:
            on = dev if generator is None or generator.device.type != "cpu" else "cpu"
            latents = torch.randn(shape, generator=generator, device=on, dtype=F32)
        elif tuple(latents.shape) != shape:
            raise ValueError(f"SanaPipeline: latents {tuple(latents.shape)}, expected {shape}")
        latents = latents.to(device=dev, dtype=F32).clone()                                   # init_noise_sigma = 1
        latents = sana_denoise_loop(tr, self.scheduler, latents=latents, prompt_embeds=embeds, prompt_attention_mask=mask, negative_prompt_embeds=neg,
                                    negative_prompt_attention_mask=neg_mask, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                    callback_on_step_end=callback_on_step_end, callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs,
                                    pipeline=self)
        if output_type == "latent":
            image = latents
        else:
            vc = self.vae.config
            scaling = vc["scaling_factor"] if isinstance(vc, dict) else vc.scaling_factor
            image = self.vae.decode(latents.to(self.vae.dtype) / scaling).sample
            image = self.image_processor.postprocess(image, output_type=output_type)
        return SanaPipelineOutput(images=image) if return_dict else (image,)
