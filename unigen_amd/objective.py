"""Flow-matching training objective of the reference's train.py on the device, and the training step built from it:

    training_sigmas(T, shift)             FlowMatchEulerDiscreteScheduler.__init__'s training sigmas (noise_scheduler_copy.sigmas)
    sample_density(scheme, B, ...)        diffusers compute_density_for_timestep_sampling (train.py:594-597), drawn on the device
    FlowMatchObjective.prepare(latents)   train.py:590-613: noise, timesteps, sigmas, (1 - sigma) x + sigma noise, _pack_latents - one HIP launch
    FlowMatchObjective.loss(pred, ...)    train.py:644-652: weighting, target = noise - x, weighted per-sample MSE, + the model's auxiliary losses
    train_step(model, optimizer, ...)     train.py:589-662 with accelerator.accumulate / backward / clip_grad_norm_ written out

The kernels are csrc/objective.hip (ug_flow_noise, ug_flow_loss, ug_flow_loss_bwd and their fp32 twins, dispatched on the latents' dtype like
every op of this package). Nothing here copies to the host: timesteps are looked up on the device (the reference's get_sigmas synchronises
once per sample), the loss backward reads autograd's upstream gradient from device memory, and train_step returns device tensors.
The per-sample loss is invariant under the pack permutation, so the loss runs on the packed prediction against a packed target and
_unpack_latents (train.py:636-641) is never needed.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from .pipeline import flow_match_sigmas

SAMPLING_SCHEMES = ("logit_normal", "mode")                   # draw u non-uniformly, weight 1
WEIGHTING_SCHEMES = ("none", "sigma_sqrt", "cosmap") + SAMPLING_SCHEMES


def training_sigmas(num_train_timesteps: int = 1000, shift: float = 1.0) -> torch.Tensor:
    """fp32 [T]: sigma_i = shift s / (1 + (shift - 1) s), s = (T - i) / T - the scheduler's training sigmas, from 1 down to
    shift / T / (1 + (shift - 1) / T). Entry i belongs to timestep sigma_i * T."""
    T = int(num_train_timesteps)
    if T <= 0:
        raise ValueError(f"training_sigmas: num_train_timesteps must be positive, got {num_train_timesteps}")
    return torch.tensor(flow_match_sigmas(T, sigmas=[(T - i) / T for i in range(T)], shift=float(shift))[:-1], dtype=torch.float32)


def sample_density(scheme: str, batch_size: int, *, logit_mean: float = 0.0, logit_std: float = 1.0, mode_scale: float = 1.29,
                   device=None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """fp32 [batch_size] draws in [0, 1): diffusers' compute_density_for_timestep_sampling with the defaults its training scripts pass.
    logit_normal: sigmoid(N(logit_mean, logit_std)); mode: 1 - u - mode_scale (cos^2(pi u / 2) - 1 + u); any other scheme: uniform."""
    if scheme not in WEIGHTING_SCHEMES:
        raise ValueError(f"sample_density: unknown weighting scheme {scheme!r} (one of {WEIGHTING_SCHEMES})")
    if scheme == "logit_normal":
        u = torch.randn(batch_size, device=device, dtype=torch.float32, generator=generator) * logit_std + logit_mean
        return torch.sigmoid(u)
    u = torch.rand(batch_size, device=device, dtype=torch.float32, generator=generator)
    if scheme == "mode":
        u = 1 - u - mode_scale * (torch.cos(math.pi * u / 2) ** 2 - 1 + u)
    return u


class _FlowLoss(torch.autograd.Function):
    """(pred, target, weight) -> (mean over the batch of the per-sample loss, the per-sample loss): ug_flow_loss forward, ug_flow_loss_bwd backward.
    Only pred gets a gradient, and only through the first output (the per-sample losses are a record, as in the reference's logs)."""

    @staticmethod
    def forward(ctx, pred, target, weight, workspace):
        per_sample, loss = ops.flow_loss(pred, target, weight, workspace)
        ctx.save_for_backward(pred, target, weight)
        ctx.mark_non_differentiable(per_sample)
        return loss, per_sample

    @staticmethod
    def backward(ctx, gout, _gper):
        pred, target, weight = ctx.saved_tensors
        return ops.flow_loss_bwd(pred, target, weight, gout.to(torch.float32).contiguous()), None, None, None


class FlowMatchObjective:
    """The flow-matching objective of one training run: weighting scheme, training sigmas, layout of the model input.

    pack=True writes the noisy input and the target in FluxPipeline._pack_latents layout (UniGenFlux); pack=False keeps [B, C, H, W]
    (UniGenSD3, which patch-embeds itself). logit_mean / logit_std / mode_scale parametrise the two sampling schemes. timestep_scale: what
    train_step multiplies prepare()'s timestep (timesteps / 1000, the FLUX transformer's convention) by before the model sees it - 1000 for a
    model that takes the scheduler's timesteps themselves (UniGenSD3)."""

    def __init__(self, weighting_scheme: str = "none", num_train_timesteps: int = 1000, shift: float = 1.0, pack: bool = True, *,
                 logit_mean: float = 0.0, logit_std: float = 1.0, mode_scale: float = 1.29, timestep_scale: float = 1.0):
        if weighting_scheme not in WEIGHTING_SCHEMES:
            raise ValueError(f"FlowMatchObjective: unknown weighting scheme {weighting_scheme!r} (one of {WEIGHTING_SCHEMES})")
        self.weighting_scheme = weighting_scheme
        self.num_train_timesteps = int(num_train_timesteps)
        self.shift = float(shift)
        self.pack = bool(pack)
        self.timestep_scale = float(timestep_scale)
        self.density = dict(logit_mean=logit_mean, logit_std=logit_std, mode_scale=mode_scale)
        self.sigmas = training_sigmas(num_train_timesteps, shift)
        self._tables: dict = {}          # device -> sigma table
        self._workspaces: dict = {}      # (device, bytes) -> partials of the loss reduction

    def sigma_table(self, device) -> torch.Tensor:
        device = torch.device(device)
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = self.sigmas.to(device)
        return t

    def prepare(self, latents: torch.Tensor, noise: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None):
        """latents [B, C, H, W] -> noisy, target, timestep, sigma, weight. `timestep` is what the model takes (timesteps / 1000, train.py:630),
        `weight` what loss() takes. noise / u default to fresh draws on the latents' device (torch.randn_like, sample_density)."""
        if noise is None:
            noise = torch.randn(latents.shape, device=latents.device, dtype=latents.dtype, generator=generator)
        if u is None:
            u = sample_density(self.weighting_scheme, latents.shape[0], device=latents.device, generator=generator, **self.density)
        noisy, target, sigma, timestep, weight = ops.flow_noise(latents, noise, u, self.sigma_table(latents.device), scheme=self.weighting_scheme,
                                                                pack=self.pack)
        return noisy, target, timestep, sigma, weight

    def loss(self, model_pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, add_losses: Optional[Dict[str, torch.Tensor]] = None):
        """-> (loss, flow_loss_per_sample): loss = mean of the weighted per-sample MSE + sum(add_losses.values()) (train.py:652), differentiable in
        model_pred and the add-losses; flow_loss_per_sample [B] fp32, detached."""
        B = model_pred.shape[0]
        nbytes = int(ops.L.load().ug_flow_loss_workspace_bytes(B, model_pred.numel() // max(B, 1)))
        key = (model_pred.device, nbytes)
        ws = self._workspaces.get(key)
        if ws is None:
            ws = self._workspaces[key] = torch.empty(nbytes, device=model_pred.device, dtype=torch.uint8)
        flow, per_sample = _FlowLoss.apply(model_pred, target, weight, ws)
        loss = flow + sum(list(add_losses.values())) if add_losses else flow
        return loss, per_sample


_OBJECTIVE_KEYS = ("latents", "noise", "u")


def train_step(model, optimizer, objective: FlowMatchObjective, batch: dict, *, accumulation_steps: int = 1, max_grad_norm: Optional[float] = 1.0,
               lr_scheduler=None, guidance_scale: Optional[float] = None, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """One pass of the reference's inner loop (train.py:589-662) for one micro-batch.

    batch: "latents" [B, C, H, W] (the encoded images), optionally "noise" and "u" (pre-drawn, e.g. for a reproducible run), and the model's other
    keyword arguments as the reference passes them (:624-635): condition_hidden_states, encoder_hidden_states, pooled_projections,
    condition_pooled_projections, txt_ids, img_ids, condition_ids (any further key is handed to the model unchanged). hidden_states, timestep and
    guidance are supplied here.

    accelerator.accumulate is written out: every call runs prepare -> forward -> loss -> (loss / accumulation_steps).backward(); every
    accumulation_steps-th call then clips (optim.clip_grad_norm_, when max_grad_norm is not None), steps the optimizer and the lr scheduler and
    zeroes the gradients. The count of calls is kept on the optimizer. Returns detached device tensors - step_loss, flow_loss (per sample), every
    add-loss, and grad_norm on the calls that clip; nothing is copied to the host."""
    if accumulation_steps < 1:
        raise ValueError(f"train_step: accumulation_steps must be >= 1, got {accumulation_steps}")
    from . import optim
    latents = batch["latents"]
    noisy, target, timestep, _sigma, weight = objective.prepare(latents, noise=batch.get("noise"), u=batch.get("u"), generator=generator)
    kwargs = {k: v for k, v in batch.items() if k not in _OBJECTIVE_KEYS}
    if getattr(model.config, "guidance_embeds", False):                                   # train.py:616-620
        if guidance_scale is None:
            raise ValueError("train_step: guidance_scale is required when model.config.guidance_embeds is True")
        kwargs["guidance"] = torch.full((1,), float(guidance_scale), device=latents.device, dtype=torch.float32).expand(latents.shape[0])
    if getattr(objective, "timestep_scale", 1.0) != 1.0:
        timestep = timestep * objective.timestep_scale
    model_pred, add_losses, _ = model(hidden_states=noisy, timestep=timestep, **kwargs)
    loss, flow_loss = objective.loss(model_pred, target, weight, add_losses)
    (loss / accumulation_steps).backward()                                                # accelerator.backward under accumulate()
    out = dict(step_loss=loss.detach(), flow_loss=flow_loss, **{k: v.detach() for k, v in (add_losses or {}).items()})
    calls = getattr(optimizer, "_unigen_micro_steps", 0) + 1
    optimizer._unigen_micro_steps = calls
    if calls % accumulation_steps == 0:                                                   # accelerator.sync_gradients
        if max_grad_norm is not None:
            params = [p for group in optimizer.param_groups for p in group["params"]]
            out["grad_norm"] = optim.clip_grad_norm_(params, max_grad_norm).detach()
        optimizer.step()
        if lr_scheduler is not None:
            lr_scheduler.step()
        optimizer.zero_grad()
    return out
