"""float64 references of the flow-matching objective kernels (csrc/objective.hip: ug_flow_noise, ug_flow_loss, ug_flow_loss_bwd), the
rounding-point variant of the noise kernel's bf16 form, the sweep's data and its bounds. Shared by tests/test_objective_ref_cpu.py (which checks
these against the torch-eager restatement of train.py) and tests/test_objective_gpu.py (which checks the kernels against these).

`slip` makes a reference commit one plausible mistake, so that the CPU test can show that the GPU bounds would catch it:
    "swap_sigma"     sigma and 1 - sigma swapped in the noisy input
    "target_sign"    target = x - noise
    "weight_late"    the weight applied after the mean over the batch (mean of the weights times the unweighted loss) instead of per sample
    "no_batch_mean"  the per-sample losses summed, not averaged, over the batch
    "pack_noisy"     pack applied to the noisy input only, the target left in [B, C, H, W] order
"""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
T_TRAIN = 1000
SCHEMES = ("none", "sigma_sqrt", "cosmap")
SHAPES = [(3, 2, 2), (16, 2, 6), (16, 6, 10), (16, 32, 32), (16, 64, 96)]      # (C, H, W): 12 elements ... several reduction blocks per sample
BATCHES = (1, 2, 3)
# draws that give idx 0, T - 1 (0.9995 * 1000 = 999.5) and the clamp (u = 1.0 -> 1000 -> T - 1; a draw is < 1, but u * T can round up to T)
U_FIXED = (0.0, 1.0, 0.9995)
U_MORE = (0.25, 0.5004, 0.731)

# bounds of the GPU sweep (tests/test_objective_gpu.py), stated once
LOSS_REL = 1e-5              # the project's fp32-twin bound: fp32 accumulation in both forms
GRAD_TWIN_REL = 1e-6
NOISY_TWIN = 2.0 ** -22      # * (|x| + |noise|)
SCALAR_ULPS = 4


def rbf(v: torch.Tensor) -> torch.Tensor:
    """The value a bf16 tensor op stores: computed in fp32, rounded to bf16 (round to nearest even), as float64."""
    return v.to(F32).to(BF).to(F64)


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """fp32 unit in the last place at |v| (float64)."""
    a = v.to(F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    a = v.to(F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def pack(a: torch.Tensor) -> torch.Tensor:
    """FluxPipeline._pack_latents: packed[b][(i, j)][c*4 + dy*2 + dx] = a[b][c][2i + dy][2j + dx]."""
    B, C, H, W = a.shape
    return a.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), C * 4)


def training_sigmas(T: int = T_TRAIN, shift: float = 1.0) -> torch.Tensor:
    """closed form in float64, rounded to fp32 once"""
    s = torch.tensor([(T - i) / T for i in range(T)], dtype=F64)
    return (shift * s / (1 + (shift - 1) * s)).to(F32)


def weight64(scheme: str, sigma: torch.Tensor) -> torch.Tensor:
    """diffusers compute_loss_weighting_for_sd3 in float64"""
    s = sigma.to(F64)
    if scheme == "sigma_sqrt":
        return s ** -2.0
    if scheme == "cosmap":
        return 2 / (math.pi * (1 - 2 * s + 2 * s ** 2))
    return torch.ones_like(s)


def scalars(u: torch.Tensor, table: torch.Tensor, scheme: str, bf16: bool):
    """-> idx, sigma, timestep (the fp32 restatement: values a correct kernel reproduces exactly) and weight (float64, from that sigma)."""
    T = table.numel()
    idx = (u.to(F32) * T).long().clamp(0, T - 1)            # (u * num_train_timesteps).long(), clamped
    s32 = table.to(F32)[idx]
    timestep = (s32 * torch.tensor(float(T), dtype=F32)) / torch.tensor(1000.0, dtype=F32)
    sigma = s32.to(BF).to(F32) if bf16 else s32
    return idx, sigma, timestep, weight64(scheme, sigma)


def flow_noise(x, noise, u, table, scheme: str, do_pack: bool, bf16: bool, slip=None):
    """x, noise: float64 [B, C, H, W] -> dict(noisy, target, sigma, timestep, weight). bf16=True: the rounding-point variant (every stated bf16
    rounding, inputs taken as they are); bf16=False: plain float64 from the fp32 sigma."""
    _, sigma, timestep, weight = scalars(u, table, scheme, bf16)
    r = rbf if bf16 else (lambda v: v)
    s = sigma.to(F64).reshape(-1, 1, 1, 1)
    a, b = r(1.0 - s), s
    if slip == "swap_sigma":
        a, b = b, a
    noisy = r(r(a * x) + r(b * noise))
    target = r(x - noise) if slip == "target_sign" else r(noise - x)
    if do_pack:
        noisy = pack(noisy)
        target = target.reshape(noisy.shape) if slip == "pack_noisy" else pack(target)
    return dict(noisy=noisy, target=target, sigma=sigma, timestep=timestep, weight=weight)


def flow_loss(pred, target, weight, slip=None):
    """float64: per-sample mean of w (pred - target)^2, and the mean of those"""
    B = pred.shape[0]
    d2 = (pred.to(F64) - target.to(F64)).reshape(B, -1) ** 2
    w = weight.to(F64).reshape(B, 1)
    if slip == "weight_late":
        per = d2.mean(1)
        return per, per.mean() * w.mean()
    per = (w * d2).mean(1)
    return per, (per.sum() if slip == "no_batch_mean" else per.mean())


def flow_loss_grad(pred, target, weight, gout: float):
    """float64: gout * 2 w_b (pred - target) / (n B)"""
    B = pred.shape[0]
    n = pred.numel() // B
    w = weight.to(F64).reshape([B] + [1] * (pred.dim() - 1))
    return gout * 2 * w * (pred.to(F64) - target.to(F64)) / (n * B)


_cases = {}


def sweep_case(B: int, shape, seed: int = 0):
    """Seeded bf16-representable latents, noise, prediction (float64 [B, C, H, W]) and the fixed draws u [B]; computed once and shared."""
    key = (B, tuple(shape), seed)
    if key not in _cases:
        C, H, W = shape
        g = torch.Generator().manual_seed(1000 * seed + 97 * B + C * H * W)
        rn = lambda: torch.randn(B, C, H, W, generator=g).to(BF).to(F64)
        us = (U_FIXED + U_MORE)
        first = (SHAPES.index(tuple(shape)) + B) % len(us) if tuple(shape) in SHAPES else 0
        u = torch.tensor([us[(first + i) % len(us)] for i in range(B)], dtype=F32)
        _cases[key] = dict(x=rn(), noise=rn(), pred=rn(), u=u)
    return _cases[key]
