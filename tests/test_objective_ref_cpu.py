"""The float64 references of the flow-matching objective (tests/objective_ref.py) against the torch-eager restatement of the reference's
train.py:603-604 (noisy model input), :607-613 (_pack_latents) and :644-652 (weighting, target, loss): agreement in float64, bit-for-bit equality of
the rounding-point variant with torch's CPU bf16 arithmetic, the loss gradient against torch.autograd, and a slip study - each plausible mistake
exceeds the bounds of the GPU sweep at least tenfold on the sweep's own data, so those bounds are tight enough to catch it."""
import math

import pytest
import torch

from tests import objective_ref as OR
from unigen_amd import objective as _objective  # noqa: F401  (these references describe this module's kernels: without it there is nothing to test)
from unigen_amd.pipeline import pack_latents

F64, F32, BF = OR.F64, OR.F32, OR.BF
TABLE = OR.training_sigmas()


def eager_noisy_target(x, noise, sigmas):
    """train.py:603-604 and :646 in x's dtype: sigmas = get_sigmas(..., n_dim=4, dtype=x.dtype)"""
    s = sigmas.to(x.dtype).reshape(-1, 1, 1, 1)
    return (1.0 - s) * x + s * noise, noise - x


def eager_weighting(scheme, sigmas):
    """diffusers compute_loss_weighting_for_sd3 (train.py:644)"""
    if scheme == "sigma_sqrt":
        return (sigmas ** -2.0).float() if sigmas.dtype != F64 else sigmas ** -2.0
    if scheme == "cosmap":
        bot = 1 - 2 * sigmas + 2 * sigmas ** 2
        return 2 / (math.pi * bot)
    return torch.ones_like(sigmas)


def eager_loss(pred, target, weighting, add_losses, acc=F32):
    """train.py:648-652; `acc` is the `.float()` of the reference (float64 in the float64 restatement)"""
    B = target.shape[0]
    w = weighting.to(acc).reshape([B] + [1] * (target.dim() - 1))
    flow = torch.mean((w * (pred.to(acc) - target.to(acc)) ** 2).reshape(B, -1), 1)
    return flow, flow.mean() + sum(list(add_losses.values()))


CASES = [(B, s) for B in OR.BATCHES for s in OR.SHAPES[:4]]


@pytest.mark.parametrize("B,shape", CASES)
@pytest.mark.parametrize("scheme", OR.SCHEMES)
def test_float64_references_match_the_eager_restatement(B, shape, scheme):
    c = OR.sweep_case(B, shape)
    idx, sigma, timestep, weight = OR.scalars(c["u"], TABLE, scheme, bf16=False)
    assert int(idx.min()) >= 0 and int(idx.max()) <= OR.T_TRAIN - 1
    r = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, scheme, True, bf16=False)
    noisy, target = eager_noisy_target(c["x"], c["noise"], sigma.to(F64))
    assert (r["noisy"] - pack_latents(noisy)).abs().max() <= 1e-12 and (r["target"] - pack_latents(target)).abs().max() <= 1e-12
    r0 = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, scheme, False, bf16=False)
    assert (r0["noisy"] - noisy).abs().max() <= 1e-12 and (r0["target"] - target).abs().max() <= 1e-12
    w = eager_weighting(scheme, sigma.to(F64))
    assert ((r["weight"] - w).abs() <= 1e-12 * w.abs()).all()
    # loss and gradient: the packed prediction against the packed target (the per-sample loss is invariant under the pack permutation)
    pred = pack_latents(c["pred"]).clone().requires_grad_(True)
    add = {"moe_loss": torch.tensor(0.125, dtype=F64)}
    flow, loss = eager_loss(pred, r["target"], w, add, acc=F64)
    per, mean = OR.flow_loss(pred.detach(), r["target"], r["weight"])
    assert ((per - flow).abs() <= 1e-12 * flow.abs()).all() and abs(float(mean + 0.125 - loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    flow_u, _ = eager_loss(c["pred"], target, w, add, acc=F64)          # the reference's own order: unpacked prediction, unpacked target
    assert ((per - flow_u).abs() <= 1e-12 * flow_u.abs()).all()
    (loss * 0.37).backward()
    g = OR.flow_loss_grad(pred.detach(), r["target"], r["weight"], 0.37)
    assert ((g - pred.grad).abs() <= 1e-12 * pred.grad.abs() + 1e-300).all()


@pytest.mark.parametrize("B,shape", CASES)
def test_rounding_point_variant_is_torch_cpu_bf16_bit_for_bit(B, shape):
    c = OR.sweep_case(B, shape)
    _, sigma, _, _ = OR.scalars(c["u"], TABLE, "none", bf16=True)
    noisy, target = eager_noisy_target(c["x"].to(BF), c["noise"].to(BF), sigma)          # torch's CPU bf16 kernels
    for do_pack in (False, True):
        r = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, "none", do_pack, bf16=True)
        e_n, e_t = (pack_latents(noisy), pack_latents(target)) if do_pack else (noisy, target)
        assert torch.equal(r["noisy"].to(BF).view(torch.int16), e_n.contiguous().view(torch.int16))
        assert torch.equal(r["target"].to(BF).view(torch.int16), e_t.contiguous().view(torch.int16))
        assert torch.equal(r["noisy"].to(BF).to(F64), r["noisy"]) and torch.equal(r["target"].to(BF).to(F64), r["target"])   # bf16 values


def test_scalars_cover_index_zero_last_and_the_clamp():
    u = torch.tensor(OR.U_FIXED, dtype=F32)
    idx, sigma, timestep, _ = OR.scalars(u, TABLE, "none", bf16=False)
    assert idx.tolist() == [0, OR.T_TRAIN - 1, OR.T_TRAIN - 1]
    assert int((u * OR.T_TRAIN).long()[1]) == OR.T_TRAIN          # unclamped, the reference would read past the table
    assert float(sigma[0]) == 1.0 and float(timestep[0]) == 1.0 and abs(float(timestep[1]) - 0.001) < 1e-9


@pytest.mark.parametrize("slip", ["swap_sigma", "target_sign", "weight_late", "no_batch_mean", "pack_noisy"])
def test_each_slip_exceeds_the_gpu_bounds_tenfold(slip):
    """On every multi-sample case of the sweep the slipped reference misses the sweep's bound (the fp32 twin's, the wider of the two forms') by 10x."""
    for B in (2, 3):
        for shape in OR.SHAPES[1:4]:
            c = OR.sweep_case(B, shape)
            # sigma_sqrt: the sweep's draws pair sigma = 1 with sigma = 0.001, which cosmap (symmetric about 1/2) weights almost alike
            good = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, "sigma_sqrt", True, bf16=False)
            bad = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, "sigma_sqrt", True, bf16=False, slip=slip)
            pred = OR.pack(c["pred"])
            if slip == "swap_sigma":
                bound = OR.NOISY_TWIN * OR.pack(c["x"].abs() + c["noise"].abs())
                excess = ((bad["noisy"] - good["noisy"]).abs() / bound).max()
            elif slip in ("target_sign", "pack_noisy"):
                excess = ((bad["target"] - good["target"]).abs() / OR.ulp32(good["target"])).max()
            else:
                _, l_good = OR.flow_loss(pred, good["target"], good["weight"])
                _, l_bad = OR.flow_loss(pred, good["target"], good["weight"], slip=slip)
                excess = (l_bad - l_good).abs() / (OR.LOSS_REL * l_good.abs())
            assert float(excess) >= 10.0, (slip, B, shape, float(excess))
