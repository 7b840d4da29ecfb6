"""References of the Sana pipeline's scheduler (unigen_amd/sana_pipeline.py, csrc/sched.hip), on the CPU:

  - schedule() and coefficients(): DPMSolverMultistepScheduler.set_timesteps and the per-step coefficients for Sana's configuration (dpmsolver++,
    midpoint, order <= 2, flow prediction on flow sigmas, final sigma zero) in float64, restated from diffusers 0.32.2's published source;
    coefficients_f32(): the same on 0-dim fp32 tensors, rounded where diffusers rounds;
  - dpm_step_f32_ops(): one step as the op-by-op fp32 torch sequence that ug_dpm_step is defined by - every line one tensor op, one rounding;
  - dpm_step_f64(): the same update in float64, and dpm_loop_f64(): a whole denoise loop in float64 around any model function.
"""
import math

import numpy as np
import torch

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def schedule(n, flow_shift=3.0, num_train_timesteps=1000):
    """-> (timesteps int64 [n], sigmas float64 [n + 1]): the shifted flow sigmas from 1 - 1/T down, a 0 appended; timesteps truncate sigma T"""
    s = 1.0 - np.linspace(1, 1 / num_train_timesteps, n + 1)
    s = np.flip(flow_shift * s / (1 + (flow_shift - 1) * s))[:-1].copy()
    return (s * num_train_timesteps).astype(np.int64), np.concatenate([s, [0.0]])


def step_order(i, n, solver_order=2):
    return 1 if (i == 0 or i == n - 1 or solver_order == 1) else 2


def _lam(s):
    return math.log(1 - s) - (math.log(s) if s > 0 else -math.inf)


def coefficients(sigmas, i, solver_order=2):
    """(order, sigma_s0, a, b, rinv, h) of step i in float64 from any sigma sequence ending in 0"""
    n = len(sigmas) - 1
    s0, st = float(sigmas[i]), float(sigmas[i + 1])
    h = _lam(st) - _lam(s0)
    a, b = st / s0, (1 - st) * (math.exp(-h) - 1.0)
    order = step_order(i, n, solver_order)
    rinv = 1.0 / ((_lam(s0) - _lam(float(sigmas[i - 1]))) / h) if order == 2 else 0.0
    return order, s0, a, b, rinv, h


def coefficients_f32(sigmas32, i, solver_order=2):
    """(order, sigma_s0, a, b, rinv) as Python floats holding fp32 values: elements of the fp32 sigma tensor, each op a 0-dim fp32 tensor op"""
    n = len(sigmas32) - 1
    lam = lambda s: torch.log(1 - s) - torch.log(s)
    s0, st = sigmas32[i], sigmas32[i + 1]
    h = lam(st) - lam(s0)
    a, b = st / s0, (1 - st) * (torch.exp(-h) - 1.0)
    order = step_order(i, n, solver_order)
    rinv = 1.0 / ((lam(s0) - lam(sigmas32[i - 1])) / h) if order == 2 else torch.tensor(0.0)
    return order, float(s0), float(a), float(b), float(rinv)


def dpm_step_f32_ops(u, t, gs, x, m1, order, sigma, a, b, rinv):
    """One step on CPU tensors, every line ONE fp32 tensor op: u, t the predictions (bf16 or fp32; t None = no guidance), x the fp32 sample, m1 the
    fp32 x0 of the step before (read at order 2 only). -> (sample, x0, model input in the predictions' dtype)"""
    c = lambda v: torch.tensor(v, dtype=F32)
    assert x.dtype == F32 and (order == 1 or m1.dtype == F32)
    p = u.to(F32)
    if t is not None:
        d = t.to(F32) - p
        d = c(gs) * d
        p = p + d
    sp = c(sigma) * p
    x0 = x - sp
    ax = c(a) * x
    bx = c(b) * x0
    o = ax - bx
    if order == 2:
        d = x0 - m1
        d = c(rinv) * d
        hb = c(0.5) * c(b)
        d = hb * d
        o = o - d
    return o, x0, o.to(u.dtype)


def dpm_step_f64(u, t, gs, x, m1, order, sigma, a, b, rinv):
    """the same update in float64 -> (sample, x0)"""
    p = u.to(F64)
    if t is not None:
        p = p + gs * (t.to(F64) - p)
    x = x.to(F64)
    x0 = x - sigma * p
    o = a * x - b * x0
    if order == 2:
        o = o - (0.5 * b) * (rinv * (x0 - m1.to(F64)))
    return o, x0


def dpm_loop_f64(model, latents, n, guidance_scale=1.0, solver_order=2, flow_shift=3.0):
    """A denoise loop in float64: model(x [B, ...] float64, timestep float64 scalar, negative: bool) -> the flow prediction. With guidance_scale > 1 the model is
    asked twice per step (negative prompt, prompt). -> the final latents"""
    ts, sig = schedule(n, flow_shift)
    x, m1 = latents.to(F64), None
    for i in range(n):
        order, s0, a, b, rinv, _ = coefficients(sig, i, solver_order)
        t = float(ts[i])
        if guidance_scale > 1.0:
            x, m1 = dpm_step_f64(model(x, t, True), model(x, t, False), guidance_scale, x, m1, order, s0, a, b, rinv)
        else:
            x, m1 = dpm_step_f64(model(x, t, False), None, 1.0, x, m1, order, s0, a, b, rinv)
    return x


def special_values(n, dtype, seed=0):
    """n values for the predictions: N(0, 1) with +-0, bf16 subnormals (below 2^-126) and values near the bf16 maximum sprinkled in, exact in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    specials = torch.tensor([0.0, -0.0, 2.0 ** -133, -(2.0 ** -130), 3 * 2.0 ** -133, 2.0 ** -126, 3.3895e38, -3.3895e38, 3.0e38, 1.0e38, -1.0e38])
    idx = torch.randperm(n, generator=g)[:min(n, 4 * len(specials))]
    v[idx] = specials.repeat(4)[:len(idx)]
    return v.to(dtype)
