"""Optimizer step on the GPU (unigen_amd/optim.py, csrc/optim.hip; reference train.py:652-662): clip_grad_norm_ and AdamW against fp64
restatements of torch's arithmetic and against torch itself, the fp32 masters of bf16 params, fused clipping, state round trips, determinism,
no host synchronisation, and three training steps of the tiny model whose inference forward must see the update."""
import pytest
import torch

from tests.step_kernel_ref import AdamWRef64 as _Ref64          # the fp64 recurrence, shared with the kernel sweep

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SIZES = [1, 7, 4095, (1 << 20) + 3]


def _params(gpu, dtype, seed=0, scale=1.0, sizes=SIZES, offset_view=True):
    """Ragged params; with offset_view one more param is a view starting 3 elements (6 or 12 bytes) into a buffer: not 16-byte aligned."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ps = [torch.nn.Parameter((scale * torch.randn(n, generator=g)).to(dtype).to(gpu)) for n in sizes]
    if offset_view:
        buf = (scale * torch.randn(5003, generator=g)).to(dtype).to(gpu)
        p = torch.nn.Parameter(torch.empty(0, device=gpu, dtype=dtype))
        p.data = buf[3:5003]
        assert p.data_ptr() % 16 != 0
        ps.append(p)
    return ps


def _grads(params, step, seed=100, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed + step)
    return [(scale * torch.randn(p.shape, generator=g)).to(p.dtype).to(p.device) for p in params]


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def _cat(ts):
    return torch.cat([t.detach().double().flatten().cpu() for t in ts])


def test_clip_grad_norm_matches_fp64_and_torch(gpu):
    from unigen_amd.optim import clip_grad_norm_
    ps = _params(gpu, torch.float32) + _params(gpu, BF, seed=1)
    grads = _grads(ps, 0, scale=0.5)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    ps[1].grad = None                                    # a param without a grad is skipped
    ps[-1].grad = torch.randn(5003, device=gpu).to(BF)[3:]   # a grad starting mid-buffer
    before = [p.grad.clone() if p.grad is not None else None for p in ps]
    truth = float(torch.cat([b.double().flatten() for b in before if b is not None]).norm())
    total = clip_grad_norm_(ps, 1.0)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.device.type == "cuda"
    print(f"clip_grad_norm_ total norm vs fp64: {abs(float(total) - truth) / truth:.3e}")
    assert abs(float(total) - truth) <= 1e-6 * truth
    coef = torch.clamp((total + 1e-6).reciprocal() * 1.0, max=1.0)
    assert float(coef) < 0.1
    for p, b in zip(ps, before):
        if b is None:
            assert p.grad is None
            continue
        assert torch.equal(p.grad, (b.float() * coef).to(b.dtype))
    # non-finite grads behave as torch's: inf -> coef 0 (inf * 0 = NaN), NaN propagates
    for bad in (float("inf"), float("nan")):
        for dt in (torch.float32, BF):
            a = _params(gpu, dt, seed=2, offset_view=False)
            b = [torch.nn.Parameter(p.detach().clone()) for p in a]
            gs = _grads(a, 1)
            gs[2][17] = bad
            for x, y, g in zip(a, b, gs):
                x.grad, y.grad = g.clone(), g.clone()
            n_ours = clip_grad_norm_(a, 1.0)
            n_torch = torch.nn.utils.clip_grad_norm_(b, 1.0)
            assert torch.equal(n_ours.isnan(), n_torch.isnan()) and torch.equal(n_ours.isinf(), n_torch.isinf()), (bad, dt, n_ours, n_torch)
            for x, y in zip(a, b):
                torch.testing.assert_close(x.grad, y.grad, rtol=0, atol=0, equal_nan=True)
            with pytest.raises(RuntimeError, match="non-finite"):
                clip_grad_norm_(a, 1.0, error_if_nonfinite=True)


def _run_fp32(gpu, steps=10):
    from unigen_amd.optim import AdamW
    a = _params(gpu, torch.float32)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    groups = lambda ps: [dict(params=ps[:3], lr=1e-3, weight_decay=0.05), dict(params=ps[3:], lr=3e-3, weight_decay=0.0)]
    ours = AdamW(groups(a), lr=1e-3, weight_decay=1e-2)
    theirs = torch.optim.AdamW(groups(b), lr=1e-3, weight_decay=1e-2, foreach=False)
    lam = lambda s: 1.0 / (1 + 0.3 * s)
    s1, s2 = torch.optim.lr_scheduler.LambdaLR(ours, lam), torch.optim.lr_scheduler.LambdaLR(theirs, lam)
    ref = _Ref64(a)
    for s in range(steps):
        gs = _grads(a, s)
        for x, y, g in zip(a, b, gs):
            x.grad, y.grad = g.clone(), g.clone()
        lrs = [ours.param_groups[0]["lr"]] * 3 + [ours.param_groups[1]["lr"]] * (len(a) - 3)
        ref.step(gs, lrs, [0.05] * 3 + [0.0] * (len(a) - 3))
        ours.step(); theirs.step(); s1.step(); s2.step()
    return a, b, ref, ours


def test_adamw_fp32_two_groups_with_scheduler(gpu):
    a, b, ref, ours = _run_fp32(gpu)
    e64 = _rel(_cat(a), _cat(ref.p))
    print(f"AdamW fp32, 10 steps, relL2 vs fp64: {e64:.3e}")
    assert e64 <= 1e-6
    # the same fp32 operations in the same order as torch's single-tensor AdamW; torch's kernels contract multiply-adds into FMAs (this
    # library is built with -ffp-contract=off), so the two differ by a few ulps of max(|p|, 0.1) (0.1: the scale of ten updates)
    for x, y in zip(a, b):
        ulp = torch.finfo(torch.float32).eps * y.detach().abs().clamp_min(0.1)
        assert float(((x - y).detach().abs() / ulp).max()) <= 4.0
    st = ours.state[a[0]]
    assert st["exp_avg"].dtype == torch.float32 and "master_param" not in st and float(st["step"]) == 10 and st["step"].device.type == "cpu"


def _run_bf16(gpu, steps, max_grad_norm=None, sizes=SIZES, scale=0.02, lr=1e-4, grad_seed=100, const_grad=False):
    from unigen_amd.optim import AdamW
    ps = _params(gpu, BF, seed=5, scale=scale, sizes=sizes)
    opt = AdamW(ps, lr=lr, weight_decay=1e-2, max_grad_norm=max_grad_norm)
    for s in range(steps):
        for p, g in zip(ps, _grads(ps, 0 if const_grad else s, seed=grad_seed)):
            p.grad = g
        opt.step()
    return ps, opt


def test_adamw_bf16_masters_track_fp64(gpu):
    ps, opt = _run_bf16(gpu, 10, lr=1e-3, scale=1.0)
    ref = _Ref64([p.detach().clone() for p in _params(gpu, BF, seed=5, scale=1.0)])
    for s in range(10):
        ref.step(_grads(ps, s), 1e-3, 1e-2)
    masters = [opt.state[p]["master_param"] for p in ps]
    e = _rel(_cat(masters), _cat(ref.p))
    print(f"AdamW bf16 masters, 10 steps, relL2 vs fp64: {e:.3e}")
    assert e <= 1e-6
    for p, m in zip(ps, masters):
        assert m.dtype == torch.float32 and torch.equal(p.detach(), m.to(BF))


def test_bf16_updates_below_one_ulp_are_kept(gpu):
    """weights ~0.02 (bf16 ulp 2^-13 ~ 1.2e-4), lr = 1e-4, a constant gradient, 20 steps: the fp64 trajectory moves every weight by ~2e-3.
    With fp32 masters the bf16 params follow it to their rounding; torch.optim.AdamW on the bf16 params themselves rounds every update."""
    sizes = [1 << 16]
    ps, _ = _run_bf16(gpu, 20, sizes=sizes, const_grad=True)
    p0 = _params(gpu, BF, seed=5, scale=0.02, sizes=sizes)
    tp = [torch.nn.Parameter(p.detach().clone()) for p in p0]
    topt = torch.optim.AdamW(tp, lr=1e-4, weight_decay=1e-2)
    ref = _Ref64(p0)
    g = _grads(p0, 0)
    for _ in range(20):
        for p, x in zip(tp, g):
            p.grad = x.clone()
        topt.step()
        ref.step(g, 1e-4, 1e-2)
    start, truth = _cat(p0), _cat(ref.p)
    moved = float((truth - start).norm())
    e_ours = float((_cat(ps) - truth).norm()) / moved
    e_torch = float((_cat(tp) - truth).norm()) / moved
    print(f"bf16 lr=1e-4 x 20 steps: |error| / |fp64 displacement|: fp32 masters {e_ours:.3f}, torch.optim.AdamW on bf16 {e_torch:.3f}")
    assert e_ours < 0.05 and e_torch > 0.15 and e_torch > 4 * e_ours


def test_fused_clipping_leaves_grads_and_equals_the_two_step_path(gpu):
    from unigen_amd.optim import AdamW, clip_grad_norm_
    a = _params(gpu, torch.float32)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    fused, plain = AdamW(a, lr=1e-3, max_grad_norm=1.0), AdamW(b, lr=1e-3)
    for s in range(4):
        gs = _grads(a, s, scale=0.1)
        for x, y, g in zip(a, b, gs):
            x.grad, y.grad = g.clone(), g.clone()
        fused.step()
        n = clip_grad_norm_(b, 1.0)
        plain.step()
        for x, g in zip(a, gs):
            assert torch.equal(x.grad, g)                # fused: grads are only read
        assert torch.equal(fused.last_grad_norm, n) and float(n) > 1.0
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    # bf16 grads: the fused path multiplies in fp32 without rounding the scaled grad to bf16 - held to the fp64 recurrence instead
    ps, opt = _run_bf16(gpu, 5, max_grad_norm=1.0, lr=1e-3, scale=1.0)
    ref = _Ref64(_params(gpu, BF, seed=5, scale=1.0))
    for s in range(5):
        gs = _grads(ps, s)
        tot = float(torch.cat([g.double().flatten() for g in gs]).norm())
        ref.step([g.double() * min(1.0, 1.0 / (tot + 1e-6)) for g in gs], 1e-3, 1e-2)
    e = _rel(_cat(opt.state[p]["master_param"] for p in ps), _cat(ref.p))
    print(f"AdamW bf16 + fused clipping, masters relL2 vs fp64: {e:.3e}")
    assert e <= 1e-6


def test_state_dict_round_trip(gpu):
    from unigen_amd.optim import AdamW

    def make():
        return _params(gpu, BF, seed=7, sizes=[4095, 70000]) + _params(gpu, torch.float32, seed=8, sizes=[33, 65537], offset_view=False)

    def feed(ps, s):
        for p, g in zip(ps, _grads(ps, s)):
            p.grad = g

    full = make()
    o = AdamW(full, lr=1e-3, max_grad_norm=1.0)
    for s in range(6):
        feed(full, s); o.step()
    half = make()
    o1 = AdamW(half, lr=1e-3, max_grad_norm=1.0)
    for s in range(3):
        feed(half, s); o1.step()
    sd = o1.state_dict()
    resumed = [torch.nn.Parameter(p.detach().clone()) for p in half]
    o2 = AdamW(resumed, lr=1e-3, max_grad_norm=1.0)
    o2.load_state_dict(sd)
    for p in resumed:
        st = o2.state[p]
        assert st["exp_avg"].dtype == torch.float32 and st["exp_avg_sq"].dtype == torch.float32 and float(st["step"]) == 3
        assert (st["master_param"].dtype == torch.float32) if p.dtype == BF else ("master_param" not in st)
    for s in range(3, 6):
        feed(resumed, s); o2.step()
    for x, y in zip(full, resumed):
        assert torch.equal(x, y)
    for k in ("exp_avg", "exp_avg_sq"):
        assert all(torch.equal(o.state[x][k], o2.state[y][k]) for x, y in zip(full, resumed))
    # a plain torch.optim.AdamW state dict: moments become fp32, the master is seeded from the param
    tp = make()
    to = torch.optim.AdamW(tp, lr=1e-3)
    feed(tp, 0); to.step()
    mine = AdamW([torch.nn.Parameter(p.detach().clone()) for p in tp], lr=1e-3)
    mine.load_state_dict(to.state_dict())
    for p, q in zip(mine.param_groups[0]["params"], tp):
        st = mine.state[p]
        assert st["exp_avg"].dtype == torch.float32 and torch.equal(st["exp_avg"], to.state[q]["exp_avg"].float())
        if p.dtype == BF:
            assert torch.equal(st["master_param"], p.detach().float())
    feed(mine.param_groups[0]["params"], 1); mine.step()
    assert float(mine.state[mine.param_groups[0]["params"][0]]["step"]) == 2


def test_deterministic_and_free_of_host_sync(gpu):
    from unigen_amd.optim import AdamW, clip_grad_norm_
    runs = []
    for _ in range(2):
        ps = _params(gpu, BF, seed=5) + _params(gpu, torch.float32, seed=6, sizes=[70000])
        opt = AdamW(ps, lr=1e-3, max_grad_norm=0.5)
        for s in range(3):
            grads = _grads(ps, s)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                for p, g in zip(ps, grads):                 # new grad tensors every step: the work list is rebuilt and uploaded each time
                    p.grad = g
                opt.step()
                clip_grad_norm_(ps, 0.5)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        runs.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg_sq"].clone() for p in ps], opt.last_grad_norm.clone()))
    (p1, v1, n1), (p2, v2, n2) = runs
    assert all(torch.equal(x, y) for x, y in zip(p1, p2)) and all(torch.equal(x, y) for x, y in zip(v1, v2)) and torch.equal(n1, n2)


def test_tiny_model_training_steps_reach_the_inference_path(gpu):
    from oracle import unigen_ref as R
    from unigen_amd import autograd as A
    from unigen_amd.flux import UniGenFlux
    from unigen_amd.optim import AdamW
    TINY = dict(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
    CONTROL = dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True, single_control_dev=2, single_block_control_method="overall_add",
                   top_num=1, expert_num_each_condition=3)

    def build():
        m = UniGenFlux.from_config(dict(TINY), device=gpu, dtype=BF)
        m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
        return m

    model = build()
    model.init_synthetic_(seed=3, std=0.05, bias_std=0.02)
    model.init_trainable_param()
    rcfg = R.FluxConfig(**TINY)
    B, grid = 2, 8
    inp = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in R.make_inputs(rcfg, B=B, grid=grid, T=64).items()}
    t = torch.full((B,), 0.75, dtype=BF, device=gpu)
    target = torch.randn(B, grid * grid, 64, generator=torch.Generator().manual_seed(5)).to(gpu)
    with torch.no_grad():
        model(timestep=t, **inp)                         # the packs exist from here on: trainable params may be views into them
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    assert names and any(n.startswith("control_") for n in names)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    versions = {n: p._version for n, p in model.named_parameters()}
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    stepped = set()
    for _ in range(3):
        for p in model.parameters():
            p.grad = None
        out, losses, _ = model(timestep=t, **inp)
        (((out.float() - target) ** 2).mean() + losses["moe_loss"]).backward()
        A.clear_activation_cache()
        stepped |= {n for n, p in model.named_parameters() if p.grad is not None}
        opt.step()
    assert stepped and stepped <= names
    assert torch.isfinite(opt.last_grad_norm)
    for n, p in model.named_parameters():
        if n not in names:
            assert torch.equal(p.detach(), before[n]), n                 # frozen: bitwise unchanged
        elif n in stepped:
            assert p._version > versions[n], n
    assert sum(not torch.equal(model.get_parameter(n).detach(), before[n]) for n in stepped) >= len(stepped) // 2
    with torch.no_grad():
        trained = model(timestep=t, **inp)[0]
        fresh = build()
        fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        again = fresh(timestep=t, **inp)[0]
    assert torch.equal(trained, again)
