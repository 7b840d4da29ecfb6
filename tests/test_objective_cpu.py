"""Host logic of the flow-matching objective (unigen_amd/objective.py) and the argument checks of its C ABI; nothing here launches a kernel."""
import ctypes as C

import pytest
import torch

from unigen_amd import lib as L
from unigen_amd import objective as O


@pytest.mark.parametrize("shift", [1.0, 3.0])
def test_training_sigmas_closed_form(shift):
    T = 1000
    s = O.training_sigmas(T, shift)
    assert s.dtype == torch.float32 and s.shape == (T,)
    i = torch.arange(T, dtype=torch.float64)
    base = (T - i) / T
    want = (shift * base / (1 + (shift - 1) * base)).to(torch.float32)
    assert torch.equal(s, want)
    assert float(s[0]) == 1.0
    assert float(s[-1]) == float(torch.tensor(shift / T / (1 + (shift - 1) / T), dtype=torch.float32))
    assert bool((s[1:] < s[:-1]).all())
    with pytest.raises(ValueError):
        O.training_sigmas(0)


@pytest.mark.parametrize("scheme", ["none", "sigma_sqrt", "cosmap", "logit_normal", "mode"])
def test_sample_density_range_and_seeded_repeatability(scheme):
    draw = lambda seed: O.sample_density(scheme, 4096, device="cpu", generator=torch.Generator().manual_seed(seed))
    u = draw(3)
    assert u.dtype == torch.float32 and u.shape == (4096,)
    assert float(u.min()) >= 0.0 and float(u.max()) <= 1.0 and bool(torch.isfinite(u).all())
    assert torch.equal(u, draw(3)) and not torch.equal(u, draw(4))
    if scheme == "logit_normal":            # sigmoid of a standard normal: symmetric about 1/2, thinner at the ends than a uniform draw
        assert abs(float(u.mean()) - 0.5) < 0.02 and float(((u < 0.1) | (u > 0.9)).float().mean()) < 0.1
    if scheme == "mode":                    # the mode scheme pushes mass towards the middle too; its map fixes 0 and 1
        assert float(((u < 0.1) | (u > 0.9)).float().mean()) < 0.15
    if scheme in ("none", "sigma_sqrt", "cosmap"):
        assert abs(float(u.mean()) - 0.5) < 0.02 and abs(float(u.var()) - 1 / 12) < 0.01
    with pytest.raises(ValueError):
        O.sample_density("nonsense", 2)


def test_public_names_are_reexported():
    import unigen_amd
    for name in ("FlowMatchObjective", "train_step", "training_sigmas", "sample_density"):
        assert getattr(unigen_amd, name) is getattr(O, name)
    with pytest.raises(ValueError):
        O.FlowMatchObjective("nonsense")


class _StubObjective(O.FlowMatchObjective):
    """the objective's arithmetic in eager torch, so that train_step's control flow runs without a GPU"""

    def prepare(self, latents, noise=None, u=None, generator=None):
        B = latents.shape[0]
        noise = torch.ones_like(latents) if noise is None else noise
        sigma = torch.full((B,), 0.5)
        s = sigma.reshape(-1, 1, 1, 1)
        return (1 - s) * latents + s * noise, noise - latents, sigma.clone(), sigma, torch.ones(B)

    def loss(self, model_pred, target, weight, add_losses=None):
        per = ((model_pred - target) ** 2).reshape(target.shape[0], -1).mean(1)
        return per.mean() + sum(list(add_losses.values())), per.detach()


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.config = type("Cfg", (), dict(guidance_embeds=True))()
        self.seen = []

    def forward(self, hidden_states, timestep, guidance, extra):
        self.seen.append((tuple(timestep.shape), guidance.tolist(), extra))
        return self.w * hidden_states, {"moe_loss": 0.01 * self.w ** 2}, None


class _CountingOptimizer(torch.optim.SGD):
    def __init__(self, params):
        super().__init__(params, lr=0.1)
        self.steps, self.zeroed, self.grad_at_step = 0, 0, []

    def step(self, closure=None):
        self.steps += 1
        self.grad_at_step.append(float(self.param_groups[0]["params"][0].grad))
        return super().step(closure)

    def zero_grad(self, set_to_none=True):
        self.zeroed += 1
        return super().zero_grad(set_to_none)


def test_train_step_accumulation_schedule():
    model, obj = _StubModel(), _StubObjective()
    opt = _CountingOptimizer(model.parameters())
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.5 ** k)
    lat = torch.arange(2 * 4 * 2 * 2, dtype=torch.float32).reshape(2, 4, 2, 2) / 10
    stepped, micro = [], []
    for call in range(1, 7):
        w_before = float(model.w.detach())
        out = O.train_step(model, opt, obj, dict(latents=lat, extra="kw"), accumulation_steps=3, max_grad_norm=None, lr_scheduler=sched, guidance_scale=3.5)
        assert set(out) == {"step_loss", "flow_loss", "moe_loss"} and not any(v.requires_grad for v in out.values())
        assert out["flow_loss"].shape == (2,)
        if float(model.w.detach()) != w_before:
            stepped.append(call)
        micro.append(None if model.w.grad is None else float(model.w.grad))
    assert stepped == [3, 6] and opt.steps == 2 and opt.zeroed == 2             # steps on calls 3 and 6 of 6, gradients zeroed only then
    assert micro[2] is None and micro[5] is None and micro[0] is not None and micro[1] is not None and abs(micro[1]) > abs(micro[0])   # accumulated in between
    assert sched.last_epoch == 2
    assert model.seen[0] == ((2,), [3.5, 3.5], "kw")
    # the accumulated gradient is the mean of the three micro-batch gradients: each backward ran on loss / 3
    m2 = _StubModel()
    noisy, target = obj.prepare(lat)[:2]
    pred, add, _ = m2(noisy, torch.zeros(2), torch.zeros(2), None)
    obj.loss(pred, target, None, add)[0].backward()
    assert abs(opt.grad_at_step[0] - float(m2.w.grad)) <= 1e-6 * abs(float(m2.w.grad))
    with pytest.raises(ValueError):
        O.train_step(model, opt, obj, dict(latents=lat, extra=None), accumulation_steps=0)
    with pytest.raises(ValueError):                # guidance_embeds without a guidance scale
        O.train_step(model, opt, obj, dict(latents=lat, extra=None))


# ---- ABI refusals: every argument is validated before any launch, so these run on a machine without a GPU -------------------------------------
def _noise_args(**over):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = dict(x=p, noise=p, u=p, table=p, T=1000, scheme=L.UG_FLOW_NONE, pack=1, B=1, C=4, H=2, W=2, noisy=p, target=p, sigma=p, timestep=p, weight=p)
    a.update(over)
    return buf, [a[k] for k in ("x", "noise", "u", "table", "T", "scheme", "pack", "B", "C", "H", "W", "noisy", "target", "sigma", "timestep", "weight")] + [None]


@pytest.mark.parametrize("fn", ["ug_flow_noise", "ug_flow_noise_f32"])
@pytest.mark.parametrize("over,code,text", [
    (dict(x=None), L.UG_ERR_BAD_SHAPE, b"null pointer"),
    (dict(weight=None), L.UG_ERR_BAD_SHAPE, b"null pointer"),
    (dict(H=3), L.UG_ERR_BAD_SHAPE, b"pack = 1 needs even H and W"),
    (dict(T=0), L.UG_ERR_BAD_SHAPE, b"T > 0"),
    (dict(scheme=7), L.UG_ERR_UNSUPPORTED, b"unknown weighting scheme 7"),
    (dict(scheme=-1), L.UG_ERR_UNSUPPORTED, b"unknown weighting scheme"),
    (dict(pack=2), L.UG_ERR_UNSUPPORTED, b"pack must be 0 or 1"),
    (dict(C=0), L.UG_ERR_BAD_SHAPE, b"positive C, H, W"),
])
def test_flow_noise_refusals(fn, over, code, text):
    cdll = L.load()
    buf, args = _noise_args(**over)
    assert getattr(cdll, fn)(*args) == code
    err = cdll.ug_last_error()
    assert text in err and fn.encode() in err, err


@pytest.mark.parametrize("suffix", ["", "_f32"])
def test_flow_loss_refusals(suffix):
    cdll = L.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    loss, bwd = getattr(cdll, "ug_flow_loss" + suffix), getattr(cdll, "ug_flow_loss_bwd" + suffix)
    ws = cdll.ug_flow_loss_workspace_bytes(2, 8)
    assert ws >= 2 * 4 and cdll.ug_flow_loss_workspace_bytes(2, 98304) > ws         # more than one block per sample at the largest sweep shape
    for args, code, text in [
        ((None, p, p, 2, 8, p, p, p, ws, None), L.UG_ERR_BAD_SHAPE, b"null pointer"),
        ((p, p, p, 2, 8, None, p, p, ws, None), L.UG_ERR_BAD_SHAPE, b"null output"),
        ((p, p, p, 0, 8, p, p, p, ws, None), L.UG_ERR_BAD_SHAPE, b"B, n > 0"),
        ((p, p, p, 2, 8, p, p, None, ws, None), L.UG_ERR_BAD_SHAPE, b"workspace"),
        ((p, p, p, 2, 8, p, p, p, ws - 1, None), L.UG_ERR_BAD_SHAPE, b"workspace"),
        ((p, p, p, 1 << 20, 8, p, p, p, 1 << 30, None), L.UG_ERR_UNSUPPORTED, b"too large"),
    ]:
        assert loss(*args) == code
        assert text in cdll.ug_last_error(), cdll.ug_last_error()
    for args, code, text in [
        ((p, None, p, p, 2, 8, p, None), L.UG_ERR_BAD_SHAPE, b"null pointer"),
        ((p, p, p, None, 2, 8, p, None), L.UG_ERR_BAD_SHAPE, b"null gout or grad"),
        ((p, p, p, p, 2, 0, p, None), L.UG_ERR_BAD_SHAPE, b"B, n > 0"),
        ((p, p, p, p + 2, 2, 8, p, None), L.UG_ERR_BAD_ALIGN, b"misaligned"),
    ]:
        assert bwd(*args) == code
        assert text in cdll.ug_last_error(), cdll.ug_last_error()
