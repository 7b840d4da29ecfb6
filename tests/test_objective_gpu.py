"""The flow-matching objective kernels (csrc/objective.hip) against the float64 references of tests/objective_ref.py, which
tests/test_objective_ref_cpu.py ties to the torch-eager restatement of train.py:589-652. Shapes are the smallest that reach each path: 12 elements
(scalar head / tail only, and with B > 1 a sample that starts off a 16-byte boundary), 192, a non-square one, 16384 and 98304 (several reduction
blocks per sample). The kernels are called through the C ABI with guard regions around every output; the host surface (FlowMatchObjective,
train_step) is tested on top: autograd, a tiny-model training step against the eager objective, and HIP-graph capture.

Bounds (docs/PARITY_TOLERANCES.md): the bf16 noise kernel is element-wise with stated rounding points - bit for bit; sigma / timestep exactly the
fp32 restatement, the weight within 4 fp32 ulps of float64 (at most 7 fp32 roundings in 2 / (pi (1 - 2s + 2s^2)), measured 2.6 over the whole
table); fp32 twin: target within one fp32 ulp, noisy within 2^-22 (|x| + |noise|) (three roundings of terms bounded by |x| + |noise|); loss 1e-5
relative (fp32 accumulation in both forms); gradient one bf16 ulp + 2^-20 |g| (bf16), 1e-6 relative (twin)."""
import pytest
import torch

from tests import objective_ref as OR
from unigen_amd import lib as L
from unigen_amd import objective as O
from unigen_amd import ops

pytestmark = pytest.mark.gpu
F64, F32, BF = OR.F64, OR.F32, OR.BF
G = 64                      # guard elements on either side of an output
FILL = -768.0               # bf16-representable; no kernel output of the sweep equals it
TABLE = OR.training_sigmas()
CASES = [(B, s) for B in OR.BATCHES for s in OR.SHAPES]
IDS = [f"B{B}-{'x'.join(map(str, s))}" for B, s in CASES]


def _guarded(n, dtype, dev, off=0):
    """-> (whole buffer, the n-element output inside it, `off` elements past a 16-byte boundary)"""
    buf = torch.full((G + off + n + G,), FILL, dtype=dtype, device=dev)
    return buf, buf[G + off:G + off + n]


def _guards_intact(buf, n, off=0):
    return bool((buf[:G + off] == FILL).all()) and bool((buf[G + off + n:] == FILL).all())


def _placed(t, dtype, dev, off=0):
    """a device copy of t (flattened) `off` elements past a 16-byte boundary"""
    buf = torch.zeros(off + t.numel() + 8, dtype=dtype, device=dev)
    buf[off:off + t.numel()] = t.reshape(-1).to(dtype).to(dev)
    return buf[off:off + t.numel()]


def _fn(name, dtype):
    return getattr(L.load(), name + ("_f32" if dtype == F32 else ""))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_noise(dev, dtype, c, shape, scheme, pack, off=0):
    B, (C, H, W) = c["x"].shape[0], shape
    n = B * C * H * W
    x, z = _placed(c["x"], dtype, dev, off), _placed(c["noise"], dtype, dev, off)
    u, table = c["u"].to(dev), TABLE.to(dev)
    outs = {k: _guarded(n, dtype, dev, off) for k in ("noisy", "target")}
    outs.update({k: _guarded(B, F32, dev) for k in ("sigma", "timestep", "weight")})
    p = lambda k: outs[k][1].data_ptr()
    L.check(_fn("ug_flow_noise", dtype)(x.data_ptr(), z.data_ptr(), u.data_ptr(), table.data_ptr(), table.numel(), ops.FLOW_SCHEMES[scheme], int(pack), B, C, H, W,
                                        p("noisy"), p("target"), p("sigma"), p("timestep"), p("weight"), _stream()), "ug_flow_noise")
    torch.cuda.synchronize()
    for k, (buf, view) in outs.items():
        assert _guards_intact(buf, view.numel(), off if k in ("noisy", "target") else 0), f"{k}: written outside the output"
    return {k: v[1].cpu() for k, v in outs.items()}


def check_noise(got, ref, c, dtype, scheme, pack):
    assert torch.equal(got["sigma"], ref["sigma"]) and torch.equal(got["timestep"], ref["timestep"]), (got["sigma"], ref["sigma"], got["timestep"], ref["timestep"])
    werr = ((got["weight"].to(F64) - ref["weight"]).abs() / OR.ulp32(ref["weight"])).max()
    print(f"weight {scheme}: {float(werr):.2f} fp32 ulps")
    if scheme == "none":
        assert torch.equal(got["weight"], torch.ones_like(got["weight"]))
    assert float(werr) <= OR.SCALAR_ULPS, (scheme, got["weight"], ref["weight"])
    rn, rt = ref["noisy"].reshape(-1), ref["target"].reshape(-1)
    if dtype == BF:
        assert torch.equal(got["noisy"].view(torch.int16), rn.to(BF).view(torch.int16)), "noisy differs from the rounding-point variant"
        assert torch.equal(got["target"].view(torch.int16), rt.to(BF).view(torch.int16)), "target differs from the rounding-point variant"
    else:
        et = ((got["target"].to(F64) - rt).abs() / OR.ulp32(rt)).max()
        mag = (c["x"].abs() + c["noise"].abs())
        mag = (OR.pack(mag) if pack else mag).reshape(-1)
        en = ((got["noisy"].to(F64) - rn).abs() / (OR.NOISY_TWIN * mag).clamp_min(1e-300)).max()
        print(f"twin: target {float(et):.3f} ulp, noisy {float(en):.3f} of its bound")
        assert float(et) <= 1.0 and float(en) <= 1.0, (float(et), float(en))


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "nchw"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,shape", CASES, ids=IDS)
def test_flow_noise_sweep(gpu, B, shape, dtype, pack):
    c = OR.sweep_case(B, shape)
    for scheme in OR.SCHEMES:
        ref = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, scheme, pack, bf16=dtype == BF)
        check_noise(run_noise(gpu, dtype, c, shape, scheme, pack), ref, c, dtype, scheme, pack)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flow_noise_scalars_at_index_zero_last_and_the_clamp(gpu, dtype):
    """every fixed draw in one batch: idx 0, T - 1 and u * T = T (clamped), for every scheme"""
    us = torch.tensor(OR.U_FIXED + OR.U_MORE, dtype=F32)
    c = dict(OR.sweep_case(len(us), (16, 2, 6), seed=1), u=us)
    for scheme in OR.SCHEMES:
        ref = OR.flow_noise(c["x"], c["noise"], us, TABLE, scheme, True, bf16=dtype == BF)
        got = run_noise(gpu, dtype, c, (16, 2, 6), scheme, True)
        check_noise(got, ref, c, dtype, scheme, True)
        assert got["sigma"][0] == 1.0 and got["sigma"][1] == got["sigma"][2] and got["timestep"][0] == 1.0


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("pack", [True, False], ids=["pack", "nchw"])
def test_flow_noise_unaligned_pointers_take_the_scalar_path(gpu, dtype, pack):
    """tensors one element past a 16-byte boundary: no 16-byte access is possible, the results are the same"""
    c = OR.sweep_case(2, (16, 6, 10))
    ref = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, "cosmap", pack, bf16=dtype == BF)
    check_noise(run_noise(gpu, dtype, c, (16, 6, 10), "cosmap", pack, off=1), ref, c, dtype, "cosmap", pack)


def _loss_inputs(B, shape):
    """exactly representable in both dtypes: the bf16 prediction and rounding-point target of the sweep, fp32 cosmap weights"""
    c = OR.sweep_case(B, shape)
    r = OR.flow_noise(c["x"], c["noise"], c["u"], TABLE, "cosmap", True, bf16=True)
    return OR.pack(c["pred"]).reshape(B, -1), r["target"].reshape(B, -1), r["weight"].to(F32)


def run_loss(dev, dtype, pred, target, weight, off=0):
    B, n = pred.shape
    p, t, w = _placed(pred, dtype, dev, off), _placed(target, dtype, dev, off), weight.to(dev)
    nbytes = int(L.load().ug_flow_loss_workspace_bytes(B, n))
    ws_buf, ws = _guarded(nbytes // 4, F32, dev)
    per_buf, per = _guarded(B, F32, dev)
    loss_buf, loss = _guarded(1, F32, dev)
    L.check(_fn("ug_flow_loss", dtype)(p.data_ptr(), t.data_ptr(), w.data_ptr(), B, n, per.data_ptr(), loss.data_ptr(), ws.data_ptr(), nbytes, _stream()),
            "ug_flow_loss")
    torch.cuda.synchronize()
    assert _guards_intact(ws_buf, nbytes // 4) and _guards_intact(per_buf, B) and _guards_intact(loss_buf, 1), "written outside an output"
    return per.cpu(), loss.cpu()


def run_grad(dev, dtype, pred, target, weight, gout, off=0):
    B, n = pred.shape
    p, t, w = _placed(pred, dtype, dev, off), _placed(target, dtype, dev, off), weight.to(dev)
    g = torch.tensor([gout], dtype=F32, device=dev)
    buf, grad = _guarded(B * n, dtype, dev, off)
    L.check(_fn("ug_flow_loss_bwd", dtype)(p.data_ptr(), t.data_ptr(), w.data_ptr(), g.data_ptr(), B, n, grad.data_ptr(), _stream()), "ug_flow_loss_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(buf, B * n, off), "written outside the gradient"
    return grad.cpu().reshape(B, n)


def check_loss_and_grad(dev, dtype, pred, target, weight, off=0):
    per64, loss64 = OR.flow_loss(pred, target, weight)
    per, loss = run_loss(dev, dtype, pred, target, weight, off)
    per2, loss2 = run_loss(dev, dtype, pred, target, weight, off)
    e_per, e_loss = float(((per.to(F64) - per64).abs() / per64.abs()).max()), float((loss.to(F64) - loss64).abs() / loss64.abs())
    print(f"loss: per-sample {e_per:.2e}, mean {e_loss:.2e} relative")
    assert e_per <= OR.LOSS_REL and e_loss <= OR.LOSS_REL, (e_per, e_loss)
    assert torch.equal(per.view(torch.int32), per2.view(torch.int32)) and torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), "not reproducible"
    for gout in (1.0, 0.37):
        g32 = float(torch.tensor(gout, dtype=F32))
        ref = OR.flow_loss_grad(pred, target, weight, g32)
        got = run_grad(dev, dtype, pred, target, weight, gout, off).to(F64)
        tol = OR.ulp_bf16(ref) + 2.0 ** -20 * ref.abs() if dtype == BF else OR.GRAD_TWIN_REL * ref.abs()
        worst = float(((got - ref).abs() / tol.clamp_min(1e-300)).max())
        print(f"grad gout={gout}: {worst:.3f} of its bound")
        assert worst <= 1.0, (gout, worst)
    return loss


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,shape", CASES, ids=IDS)
def test_flow_loss_and_gradient_sweep(gpu, B, shape, dtype):
    check_loss_and_grad(gpu, dtype, *_loss_inputs(B, shape))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_flow_loss_unaligned_pointers_and_both_dtypes_agree(gpu, dtype):
    pred, target, weight = _loss_inputs(3, (16, 6, 10))
    aligned = check_loss_and_grad(gpu, dtype, pred, target, weight)
    shifted = check_loss_and_grad(gpu, dtype, pred, target, weight, off=1)
    other = run_loss(gpu, F32 if dtype == BF else BF, pred, target, weight)[1]
    assert abs(float(aligned) - float(shifted)) <= 2 * OR.LOSS_REL * abs(float(aligned))
    assert torch.equal(aligned, other)          # same representable inputs, same fp32 arithmetic in the same order: the two forms agree bit for bit


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_objective_loss_autograd(gpu, dtype):
    """FlowMatchObjective.loss + a fake add-loss, backward: pred.grad is the kernel's output for gout = 1, the loss is the sum"""
    pred64, target64, weight = _loss_inputs(2, (16, 6, 10))
    obj = O.FlowMatchObjective("cosmap")
    pred = pred64.to(dtype).to(gpu).reshape(2, 60, 16).requires_grad_(True)
    target, w = target64.to(dtype).to(gpu).reshape(2, 60, 16), weight.to(gpu)
    a = torch.tensor(0.25, device=gpu, requires_grad=True)
    loss, per = obj.loss(pred, target, w, {"moe_loss": 3 * a})
    assert not per.requires_grad and loss.dim() == 0 and loss.dtype == F32
    k_per, k_loss = ops.flow_loss(pred.detach(), target, w)
    assert torch.equal(per, k_per) and torch.equal(loss.detach(), k_loss + 3 * a.detach())
    loss.backward()
    want = ops.flow_loss_bwd(pred.detach(), target, w, torch.ones(1, device=gpu))
    assert pred.grad.dtype == dtype and pred.grad.shape == pred.shape and torch.equal(pred.grad, want) and float(a.grad) == 3.0
    assert float(pred.grad.abs().max()) > 0
    pred.grad = None
    (obj.loss(pred, target, w)[0] * 0.5).backward()          # no add-losses; the upstream gradient reaches the kernel through device memory
    assert torch.equal(pred.grad, ops.flow_loss_bwd(pred.detach(), target, w, torch.full((1,), 0.5, device=gpu)))


def test_prepare_draws_and_shapes(gpu):
    obj = O.FlowMatchObjective("logit_normal", shift=3.0)
    lat = torch.randn(2, 16, 4, 6, device=gpu).to(BF)
    gen = torch.Generator(device=gpu).manual_seed(4)
    noisy, target, timestep, sigma, weight = obj.prepare(lat, generator=gen)
    assert noisy.shape == target.shape == (2, 6, 64) and noisy.dtype == BF and timestep.shape == sigma.shape == weight.shape == (2,)
    assert bool((weight == 1).all()) and bool((sigma > 0).all()) and bool((sigma <= 1).all())
    again = obj.prepare(lat, generator=torch.Generator(device=gpu).manual_seed(4))
    assert all(torch.equal(p, q) for p, q in zip((noisy, target, timestep, sigma, weight), again))
    flat = O.FlowMatchObjective("none", pack=False).prepare(lat.float())
    assert flat[0].shape == lat.shape and flat[0].dtype == F32
    with pytest.raises(L.UniGenHipError):
        obj.prepare(torch.randn(1, 16, 3, 4, device=gpu).to(BF))          # odd H cannot be packed


def _unpack(p, C, H, W):
    """FluxPipeline._unpack_latents as differentiable torch (train.py:636-641)"""
    B = p.shape[0]
    return p.view(B, H // 2, W // 2, C, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_train_step_matches_the_eager_objective(gpu, dtype):
    """Two accumulation micro-steps and the optimizer step they end in, on the tiny FLUX of tests/test_training_gpu.py: train_step against the same
    sequence written with the torch-eager objective (train.py:598-662) around the same forward, optimizer and clipping. Loss to 1e-5; in the fp32-twin
    model the parameters after the step are equal bit for bit. "Every trainable parameter changed" is checked as: a parameter changes exactly when it
    received a gradient - parameters behind a discarded context output get None in the reference too (tests/test_training_gpu.py) and no optimizer
    moves those - and most do."""
    import importlib
    from oracle import unigen_ref as R
    from tests.test_training_gpu import CONTROL, TINY, _dev
    from unigen_amd import optim
    from unigen_amd.pipeline import pack_latents
    cls = importlib.import_module("src.UniGenTransformer").UniGenFlux
    B, grid, T, C = 2, 8, 64, 16
    H = W = 2 * grid
    rcfg = R.FluxConfig(condition_nums=1, **TINY)
    inp = R.make_inputs(rcfg, B=B, grid=grid, T=T)
    inp.pop("hidden_states")
    kw = {k: _dev(v, gpu, dtype if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    g = torch.Generator().manual_seed(21)
    micro = [dict(latents=torch.randn(B, C, H, W, generator=g).to(BF).to(dtype).to(gpu), noise=torch.randn(B, C, H, W, generator=g).to(BF).to(dtype).to(gpu),
                  u=torch.tensor(us, dtype=F32, device=gpu)) for us in ((0.25, 0.731), (0.5004, 0.9995))]
    state = {}

    def build():
        model = cls.from_config(dict(TINY), device=gpu, dtype=dtype)
        model.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
        if not state:
            model.init_synthetic_(seed=3, std=0.05, bias_std=0.02)
            state.update({k: v.detach().clone() for k, v in model.state_dict().items()})
        else:
            model.load_state_dict(state)
        model.init_trainable_param()
        params = [p for p in model.parameters() if p.requires_grad]
        return model, optim.AdamW(params, lr=1e-3, weight_decay=1e-2)

    # train_step
    model, opt = build()
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    before = {n: model.get_parameter(n).detach().clone() for n in names}
    obj = O.FlowMatchObjective("none")
    outs = [O.train_step(model, opt, obj, dict(m, **kw), accumulation_steps=2, max_grad_norm=1.0) for m in micro]
    assert "grad_norm" not in outs[0] and "grad_norm" in outs[1] and all(not v.requires_grad and v.is_cuda for o in outs for v in o.values())
    assert all(model.get_parameter(n).grad is None for n in names)
    after = {n: model.get_parameter(n).detach().clone() for n in names}

    # the same two micro-steps and optimizer step with the objective in eager torch
    model_e, opt_e = build()
    table = TABLE.to(gpu)
    losses_e = []
    for m in micro:
        idx = (m["u"] * OR.T_TRAIN).long().clamp(max=OR.T_TRAIN - 1)
        s32 = table[idx]
        timesteps = s32 * OR.T_TRAIN                                       # noise_scheduler_copy.timesteps[indices]
        sig = s32.to(dtype).reshape(-1, 1, 1, 1)                           # get_sigmas(timesteps, n_dim=4, dtype=latents.dtype)
        noisy = (1.0 - sig) * m["latents"] + sig * m["noise"]
        pred, add, _ = model_e(hidden_states=pack_latents(noisy), timestep=timesteps / 1000, **kw)
        pred = _unpack(pred, C, H, W)
        weighting = torch.ones_like(sig)
        target = m["noise"] - m["latents"]
        flow = torch.mean((weighting.float() * (pred.float() - target.float()) ** 2).reshape(B, -1), 1)
        loss = flow.mean() + sum(list(add.values()))
        (loss / 2).backward()
        losses_e.append(loss.detach())
    with_grad = {n for n in names if model_e.get_parameter(n).grad is not None}
    norm_e = optim.clip_grad_norm_([model_e.get_parameter(n) for n in names], 1.0)
    opt_e.step()
    opt_e.zero_grad()
    torch.cuda.synchronize()

    for o, le in zip(outs, losses_e):
        rel = abs(float(o["step_loss"]) - float(le)) / abs(float(le))
        print(f"train_step {dtype}: loss {float(o['step_loss']):.7f} vs eager {float(le):.7f} (rel {rel:.2e})")
        assert rel <= 1e-5, (float(o["step_loss"]), float(le))
    changed = {n for n in names if not torch.equal(before[n], after[n])}
    # fp32: a parameter with an all-zero gradient still moves by the weight decay. bf16: that decay (1e-5 relative) moves the fp32 master only
    assert changed <= with_grad and (dtype != F32 or changed == with_grad) and len(changed) > len(names) // 2, \
        (sorted(with_grad - changed)[:8], len(changed), len(with_grad), len(names))
    if dtype == F32:
        assert torch.equal(outs[1]["grad_norm"], norm_e), (float(outs[1]["grad_norm"]), float(norm_e))
        differ = [n for n in names if not torch.equal(after[n], model_e.get_parameter(n).detach())]
        assert not differ, f"{len(differ)} of {len(names)} parameters differ after the step: {differ[:5]}"
    else:
        gn, ge = float(outs[1]["grad_norm"]), float(norm_e)
        assert abs(gn - ge) <= 2e-2 * abs(ge), (gn, ge)


def test_objective_is_hip_graph_capturable(gpu):
    """prepare (pre-drawn u and noise) + flow_loss + flow_loss_bwd on one stream capture into a HIP graph; a replay reproduces the eager outputs bit
    for bit (the precedent of test_denoise_step_is_hip_graph_capturable: single branch, no host copy, no allocation outside the graph's pool)."""
    c = OR.sweep_case(2, (16, 32, 32))
    obj = O.FlowMatchObjective("cosmap")
    lat, noise, pred = (c[k].to(BF).to(gpu) for k in ("x", "noise", "pred"))
    pred = ops.pack_latents(pred)
    u, gout = c["u"].to(gpu), torch.full((1,), 0.37, device=gpu)

    def step():
        noisy, target, timestep, sigma, weight = obj.prepare(lat, noise=noise, u=u)
        per, loss = ops.flow_loss(pred, target, weight)
        return noisy, target, timestep, sigma, weight, per, loss, ops.flow_loss_bwd(pred, target, weight, gout)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for t in out:
        t.zero_()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert float(eager[-1].abs().max()) > 0 and float(eager[6]) > 0
