"""Training the LoRA adapters: ug_lora_wgrad (csrc/lora_bwd.hip) against the float64 references of tests/lora_bwd_ref.py, and the adapters' gradients
through the differentiable forward (unigen_amd/training.py, autograd.Projection) against torch autograd of the CPU oracle whose projections are
peft 0.15's LoRA Linear (R.lora_linear) holding requires_grad A / B tensors. Geometry and adapter placement of tests/test_lora_gpu.py; bounds of
docs/PARITY_TOLERANCES.md ("Backward sweep") for the kernel and of tests/test_training_gpu.py for the gradients.

ug_lora_down_bf16 lost its A/B against ug_gemm_bf16 at N = 64 on the larger shapes and lives in the probe library (tools/probe/csrc/lora_down.hip;
tools/lora_down_ab.py checks it against float64): T = x A_cat^T and dT = dY B_bd run through ug_gemm_bf16, so it has no rows in the product sweep.
The issue's separate bound on "the rows the last, partial M-block feeds" is read as follows for ug_lora_wgrad: every output row sums over all of M,
so the partial block is bounded by a second call on the tail rows alone (test_lora_wgrad_sweep)."""
import importlib

import pytest
import torch

from oracle import unigen_ref as R
from tests import lora_bwd_ref as ref
from tests.test_flux_gpu import CONTROL, TINY, _to_dev
from tests.test_lora_gpu import _adapters
from tests.test_training_gpu import _dev, _step
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 7.0


# ---------------------------------------------------------------------------------------------------------------------
# kernel sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [64, 1536, 3072, 21504])
@pytest.mark.parametrize("R_", [64, 128, 192, 256])
@pytest.mark.parametrize("M", [64, 333, 1000, 4608, 9216 + 77])
def test_lora_wgrad_sweep(gpu, M, R_, J):
    """bf16 and fp32, non-trivial leading dimensions on P, Q and C, a guard band around C compared bit for bit, two runs bit-identical. The output
    rows are rank rows: each sums over all of M, the last partial 64-row block of M included, so "the rows the partial block feeds" are all rows;
    its contribution is bounded separately, from the same kernel run on the tail rows alone."""
    from unigen_amd import ops
    g = torch.Generator().manual_seed(M * 7 + R_ + J)
    p32, q32 = torch.randn(M, R_, generator=g) * 0.5, torch.randn(M, J, generator=g)
    alpha = 0.75
    tail0 = M // 64 * 64
    for dt in (BF, torch.float32):
        p, q = p32.to(dt), q32.to(dt)
        pb = torch.full((M, R_ + 8), GUARD, dtype=dt); pb[:, :R_] = p
        qb = torch.full((M, J + 24), GUARD, dtype=dt); qb[:, 16:16 + J] = q
        pd, qd = pb.to(gpu)[:, :R_], qb.to(gpu)[:, 16:16 + J]
        outs = []
        for _ in range(2):
            buf = torch.full((R_ + 2, J + 40), GUARD, device=gpu, dtype=dt)
            ops.lora_wgrad(pd, qd, buf[1:R_ + 1, 8:8 + J], alpha=alpha)
            outs.append(buf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), "two runs differ"
        got = outs[0][1:R_ + 1, 8:8 + J].cpu()
        band = outs[0].clone(); band[1:R_ + 1, 8:8 + J] = GUARD
        assert bool((band == GUARD).all()), "wrote outside its output"
        truth, var = ref.lora_wgrad(p, q, alpha)
        e, e_row, _ = ref.err(got, truth)
        if dt == torch.float32:
            print(f"lora_wgrad f32 M={M} R={R_} J={J}: rel_l2 {e:.2e} worst row {e_row:.2e}")
            assert e <= 1e-5 and e_row <= 1e-4, (e, e_row)
        else:
            v, v_row, _ = ref.err(var, truth)
            print(f"lora_wgrad bf16 M={M} R={R_} J={J}: rel_l2 {e:.2e} (variant {v:.2e}) worst row {e_row:.2e} (variant {v_row:.2e})")
            assert e <= max(1.5 * v, 2.0 ** -9) and e_row <= max(1.5 * v_row, 2.0 ** -9), (e, v, e_row, v_row)
        if tail0 < M and tail0 > 0:            # the partial block alone: the same call on the tail rows (zero-filled on chip up to 64)
            gt = ops.lora_wgrad(pd[tail0:], qd[tail0:], alpha=alpha).cpu()
            truth_t, var_t = ref.lora_wgrad(p[tail0:], q[tail0:], alpha)
            et, et_row, _ = ref.err(gt, truth_t)
            if dt == torch.float32:
                assert et <= 1e-5 and et_row <= 1e-4, (et, et_row)
            else:
                vt, vt_row, _ = ref.err(var_t, truth_t)
                assert et <= max(1.5 * vt, 2.0 ** -9) and et_row <= max(1.5 * vt_row, 2.0 ** -9), (et, vt, et_row, vt_row)


# ---------------------------------------------------------------------------------------------------------------------
# gradient parity against the oracle's autograd
# ---------------------------------------------------------------------------------------------------------------------
CTL = dict(condition_nums=3, condition_types=["canny", "depth", "openpose"], control_params=dict(CONTROL))
B_, GRID, T_ = 2, 8, 32


def _cls():
    return importlib.import_module("src.UniGenTransformer").MultiCondtionUniGenFlux


def _model(gpu, dtype, state=None, adapters=True):
    m = _cls().from_config(dict(TINY), device=gpu, dtype=dtype)
    m.init_condition_block(**CTL)
    if state is None:
        m.init_synthetic_(seed=7, std=0.05, bias_std=0.02)
    if adapters:
        _adapters(m)
    if state is None:
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():                                   # B large enough for the adapters to move the output (add_lora's 0.02 is too small)
            for lay in m._lora_sites.values():
                for a in lay.lora_B:
                    w = lay.lora_B[a].weight
                    w.copy_((torch.randn(w.shape, generator=g) * 0.3).to(gpu))
    else:
        res = m.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=False)
        assert not res.unexpected_keys and (adapters and not res.missing_keys or not adapters), res
    return m


@pytest.fixture(scope="module")
def world(gpu):
    m = _model(gpu, BF)
    state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    rcfg = R.FluxConfig(condition_nums=3, **TINY)
    inp = R.make_inputs(rcfg, B=B_, grid=GRID, T=T_, n_cond=3)
    t = torch.full((B_,), 0.75, dtype=BF)
    target = torch.randn(B_, GRID * GRID, 64, generator=torch.Generator().manual_seed(5))
    return state, rcfg, inp, t, target


def _live(model, factor=1.0):
    return {n: [(a, lay.scaling[a] * factor) for a in lay.live_adapters()] for n, lay in model._lora_sites.items() if lay.live_adapters()}


def _oracle(world, names, live, dtype):
    state, rcfg, inp, t, target = world
    plain = {k: v for k, v in state.items() if ".lora_" not in k}
    st = {k: (v.to(dtype).clone().requires_grad_(True) if k in names else v.to(dtype)) for k, v in state.items()}
    st[R.LORA_KEY] = {n: [(st[f"{n}.lora_A.{a}.weight"], st[f"{n}.lora_B.{a}.weight"], s) for a, s in ad] for n, ad in live.items()}
    out, loss, _ = _step(lambda: R.unigen_flux_forward(st, rcfg, timestep=t, dtype=dtype, **inp), target, dtype)
    return out, loss, {k: st[k].grad for k in names}, plain


def _hip(world, gpu, dtype, prepare, ctx=None, **fkw):
    """-> (out, loss, {name: grad}, names, live adapters during the forward)"""
    state, rcfg, inp, t, target = world
    model = _model(gpu, dtype, state)
    names = prepare(model)
    kw = {k: _dev(v, gpu, dtype if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    mod = importlib.import_module("src.lora_switching_module")
    import contextlib
    with (mod.enable_lora(list(model.modules()), ctx) if ctx is not None else contextlib.nullcontext()):
        live = _live(model, fkw.get("joint_attention_kwargs", {}).get("scale", 1.0))
        out, loss, _ = _step(lambda: model(timestep=t.to(gpu), **kw, **fkw), target, dtype)
    torch.cuda.synchronize()
    return out, loss, {k: model.get_parameter(k).grad for k in names}, names, live


def _compare(world, gpu, prepare, ctx=None, off=(), **fkw):
    state, rcfg, inp, t, target = world
    out32, loss32, g32, names, live = _hip(world, gpu, torch.float32, prepare, ctx, **fkw)
    assert any(".lora_A." in n for n in names)
    truth_out, truth_loss, truth, plain = _oracle(world, names, live, torch.float32)
    moved = rel_l2(truth_out, R.unigen_flux_forward(plain, rcfg, timestep=t, dtype=torch.float32, **inp)[0].detach())
    assert moved >= 5e-2, f"the adapters move the oracle's output by {moved:.2e} only: the test would not see its subject"
    z = lambda d, k: (d[k].detach().float().cpu() if d[k] is not None else torch.zeros(state[k].shape))
    for k in names:                           # switched-off adapters: None or exact zeros, in the oracle and here
        if any(f".{a}." in k for a in off):
            assert float(z(g32, k).abs().max()) == 0.0 and (truth[k] is None or float(truth[k].abs().max()) == 0.0), k
    dead = {k for k in names if truth[k] is None or float(truth[k].abs().max()) == 0.0}
    live_names = [k for k in names if k not in dead]
    assert len(live_names) > len(names) // 3
    cat = lambda d: torch.cat([z(d, k).flatten() for k in names])
    rel = lambda a, b: float((a - b).norm() / b.norm())
    e_all = rel(cat(g32), cat(truth))
    floor = 1e-3 * float(cat(truth).norm()) / len(names) ** 0.5
    worst = max((float((z(g32, k) - truth[k]).norm() / max(float(truth[k].norm()), floor)), k) for k in live_names)
    assert all(float(z(g32, k).abs().max()) == 0.0 for k in dead), "a parameter behind a discarded output received a gradient"
    print(f"lora training fp32: loss {loss32:.6f} vs {truth_loss:.6f}; gradients rel_l2 {e_all:.3e}; worst {worst[1]} {worst[0]:.3e}; moved {moved:.2e}")
    assert abs(loss32 - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-7 and e_all <= 1e-3 and worst[0] <= 5e-3, (loss32, truth_loss, e_all, worst)
    _, ref_loss, gref, _ = _oracle(world, names, live, BF)
    _, loss16, g16, _, _ = _hip(world, gpu, BF, prepare, ctx, **fkw)
    e_hip, e_ref = rel(cat(g16), cat(truth)), rel(cat(gref), cat(truth))
    print(f"lora training bf16: loss {loss16:.5f} (oracle bf16 {ref_loss:.5f}); gradients vs fp32: hip {e_hip:.3e}, oracle bf16 {e_ref:.3e}")
    assert e_hip <= 1.5 * e_ref + 5e-3, (e_hip, e_ref)


def _adapters_only(model):
    return list(model.set_lora_trainable())


def test_adapter_gradients_all_live(world, gpu):
    _compare(world, gpu, _adapters_only)


def test_adapter_gradients_under_enable_lora(world, gpu):
    _compare(world, gpu, _adapters_only, ctx=["depth", "openpose"], off=("canny",))


def test_adapter_gradients_with_forward_scale(world, gpu):
    _compare(world, gpu, _adapters_only, joint_attention_kwargs={"scale": 0.5})


def test_control_modules_and_adapters_in_one_backward(world, gpu):
    def prepare(model):
        model.init_trainable_param()
        names = list(model.set_lora_trainable(freeze_rest=False))
        assert any(n.startswith("control_joint_trans_blocks.") and ".lora_" not in n for n in names)
        return names
    _compare(world, gpu, prepare)


def test_checkpointed_gradients_are_bit_identical(world, gpu):
    """Blocks recomputed inside backward(), after the forward's scale has been undone, see the adapters as the forward saw them."""
    def prepare_ckpt(model):
        model.enable_gradient_checkpointing()
        return _adapters_only(model)
    kw = dict(joint_attention_kwargs={"scale": 0.5})
    _, l0, g0, names, _ = _hip(world, gpu, BF, _adapters_only, **kw)
    _, l1, g1, _, _ = _hip(world, gpu, BF, prepare_ckpt, **kw)
    assert l0 == l1
    for k in names:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
def test_attached_but_not_live_is_bit_identical(world, gpu):
    state, rcfg, inp, t, target = world
    mod = importlib.import_module("src.lora_switching_module")
    kw = {k: _dev(v, gpu, BF if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    res = []
    for adapters in (False, True):
        m = _model(gpu, BF, {k: v for k, v in state.items() if adapters or ".lora_" not in k}, adapters=adapters)
        m.init_trainable_param()
        names = [n for n, p in m.named_parameters() if p.requires_grad and ".lora_" not in n]
        with mod.enable_lora(list(m.modules()), []):
            out, loss, _ = _step(lambda: m(timestep=t.to(gpu), **kw), target, BF)
        res.append((loss, out, {k: m.get_parameter(k).grad for k in names}))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    for k, g0 in res[0][2].items():
        g1 = res[1][2][k]
        assert (g0 is None and g1 is None) or torch.equal(g0, g1), k


def test_inference_unchanged_by_set_lora_trainable(world, gpu):
    state, rcfg, inp, t, target = world
    m = _model(gpu, BF, state)
    kw = {k: _to_dev(v, gpu) for k, v in inp.items()}
    with torch.no_grad():
        a = m(timestep=t.to(gpu), **kw)[0].clone()
        names = m.set_lora_trainable()
        assert names and all(".lora_" in n for n in names)
        b = m(timestep=t.to(gpu), **kw)[0]
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# a step actually trains
# ---------------------------------------------------------------------------------------------------------------------
def test_twenty_adamw_steps_train_the_adapters(world, gpu):
    from unigen_amd.optim import AdamW
    state, rcfg, inp, t, target = world
    m = _model(gpu, BF, state)
    names = m.set_lora_trainable()
    params = [m.get_parameter(n) for n in names]
    base0 = {k: v.detach().clone() for k, v in m.state_dict().items() if ".lora_" not in k}
    kw = {k: _dev(v, gpu, BF if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    ikw = {k: _to_dev(v, gpu) for k, v in inp.items()}
    with torch.no_grad():
        before = m(timestep=t.to(gpu), **ikw)[0].clone()
    opt = AdamW(params, lr=2e-3, weight_decay=0.0)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        _, loss, _ = _step(lambda: m(timestep=t.to(gpu), **kw), target, BF)
        opt.step()
        losses.append(loss)
    print("lora training losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0], losses
    for k, v in m.state_dict().items():
        if ".lora_" not in k:
            assert torch.equal(v, base0[k]), f"{k}: a frozen base weight changed"
    with torch.no_grad():
        after = m(timestep=t.to(gpu), **ikw)[0].clone()
    assert not torch.equal(after, before), "the inference forward did not see the updated adapters (stale fused operands)"
    fresh = _model(gpu, BF, {k: v for k, v in state.items()})
    for a in ("canny", "depth", "openpose"):
        fresh.load_lora_state_dict(m.lora_state_dict(a), a)
    with torch.no_grad():
        again = fresh(timestep=t.to(gpu), **ikw)[0]
    assert torch.equal(again, after)


# ---------------------------------------------------------------------------------------------------------------------
# UniGenSD3: separate to_q / to_k / to_v launches, dual attention attn2, the context_pre_only block, T = 24 (ragged rows everywhere)
# ---------------------------------------------------------------------------------------------------------------------
def test_sd3_adapter_gradients_match_oracle_autograd(gpu):
    """The adapter placement of tests/test_lora_gpu.py::test_sd3_forward_with_adapters_matches_oracle ("depth" on the base joint blocks' attention,
    attn2 and feed-forward projections, "canny" on the control blocks' attention), both live, B = 0.3 N(0, 1); bounds of the Flux cases."""
    from tests.test_lora_gpu import ATTN
    from tests.test_sd3_gpu import TINY as SD3_TINY
    cls = importlib.import_module("src.UniGenTransformer").UniGenSD3
    targets = ATTN + ["attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_add_out", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
                      "ff.net.0.proj", "ff.net.2"]

    def build(dtype, state=None):
        m = cls.from_config(dict(SD3_TINY), device=gpu, dtype=dtype)
        m.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=False))
        if state is None:
            m.init_synthetic_(seed=5, std=0.05, bias_std=0.02)
        m.add_lora(targets, "depth", 8, 16.0, prefix="transformer_blocks.", init_lora_weights=False, seed=31)
        m.add_lora(ATTN, "canny", 4, 8.0, prefix="control_", init_lora_weights=False, seed=32)
        if state is None:
            g = torch.Generator().manual_seed(12)
            with torch.no_grad():
                for lay in m._lora_sites.values():
                    for a in lay.lora_B:
                        lay.lora_B[a].weight.copy_((torch.randn(lay.lora_B[a].weight.shape, generator=g) * 0.3).to(gpu))
        else:
            res = m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}, strict=False)
            assert not res.missing_keys and not res.unexpected_keys, res
        return m

    base = build(BF)
    assert any(".attn2." in n for n in base._lora_sites) and any(n.startswith("transformer_blocks.2.") for n in base._lora_sites)
    state = {k: v.detach().cpu() for k, v in base.state_dict().items()}
    names = list(base.set_lora_trainable())
    live = _live(base)
    rcfg = R.SD3Config(use_modulate=False, **SD3_TINY)
    B, hw, T = 2, 16, 24
    inp = R.make_sd3_inputs(rcfg, B=B, hw=hw, T=T)
    t = torch.full((B,), 600.0)
    target = torch.randn(B, 16, hw, hw, generator=torch.Generator().manual_seed(5))

    def oracle(dtype):
        st = {k: (v.to(dtype).clone().requires_grad_(True) if k in names else (v.to(dtype) if v.is_floating_point() else v)) for k, v in state.items()}
        st[R.LORA_KEY] = {n: [(st[f"{n}.lora_A.{a}.weight"], st[f"{n}.lora_B.{a}.weight"], s) for a, s in ad] for n, ad in live.items()}
        out, loss, _ = _step(lambda: R.unigen_sd3_forward(st, rcfg, timestep=t, dtype=dtype, **inp), target, dtype)
        return out, loss, {k: st[k].grad for k in names}

    def hip(dtype):
        model = build(dtype, state)
        assert list(model.set_lora_trainable()) == names
        kw = {k: _dev(v, gpu, dtype if k != "gate_uniform" else None) for k, v in inp.items()}
        out, loss, _ = _step(lambda: model(timestep=t.to(gpu), **kw), target, dtype)
        torch.cuda.synchronize()
        return out, loss, {k: model.get_parameter(k).grad for k in names}

    truth_out, truth_loss, truth = oracle(torch.float32)
    plain = {k: (v.float() if v.is_floating_point() else v) for k, v in state.items() if ".lora_" not in k}
    moved = rel_l2(truth_out, R.unigen_sd3_forward(plain, rcfg, timestep=t, dtype=torch.float32, **inp)[0].detach())
    assert moved >= 5e-2, f"the adapters move the oracle's output by {moved:.2e} only"
    dead = {k for k in names if truth[k] is None or float(truth[k].abs().max()) == 0.0}
    live_names = [k for k in names if k not in dead]
    assert len(live_names) > len(names) // 3
    z = lambda d, k: (d[k].detach().float().cpu() if d[k] is not None else torch.zeros(state[k].shape))
    cat = lambda d: torch.cat([z(d, k).flatten() for k in names])
    rel = lambda a, b: float((a - b).norm() / b.norm())
    _, loss32, g32 = hip(torch.float32)
    e_all = rel(cat(g32), cat(truth))
    floor = 1e-3 * float(cat(truth).norm()) / len(names) ** 0.5
    worst = max((float((z(g32, k) - truth[k]).norm() / max(float(truth[k].norm()), floor)), k) for k in live_names)
    print(f"lora training sd3 fp32: loss {loss32:.6f} vs {truth_loss:.6f}; gradients rel_l2 {e_all:.3e}; worst {worst[1]} {worst[0]:.3e}; moved {moved:.2e}; dead {len(dead)}")
    assert all(float(z(g32, k).abs().max()) == 0.0 for k in dead), "a parameter behind a discarded output received a gradient"
    assert abs(loss32 - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-7 and e_all <= 1e-3 and worst[0] <= 5e-3, (loss32, truth_loss, e_all, worst)
    _, ref_loss, gref = oracle(BF)
    _, loss16, g16 = hip(BF)
    e_hip, e_ref = rel(cat(g16), cat(truth)), rel(cat(gref), cat(truth))
    print(f"lora training sd3 bf16: loss {loss16:.5f} (oracle bf16 {ref_loss:.5f}); gradients vs fp32: hip {e_hip:.3e}, oracle bf16 {e_ref:.3e}")
    assert e_hip <= 1.5 * e_ref + 5e-3, (e_hip, e_ref)


# ---------------------------------------------------------------------------------------------------------------------
# one autograd.Projection with adapters against the float64 reference and its rounding-point variant
# ---------------------------------------------------------------------------------------------------------------------
def test_single_layer_backward_against_rounding_point_variant(gpu):
    """n = 3 projections of one x at ragged M = 333, separate (non-adjacent) weights: projection 0 carries two adapters, projection 1 one adapter but
    receives no dy, projection 2 carries none. bf16: dx, dA, dB within max(1.5 x the rounding-point variant's error, 2^-9) of the float64 truth (the
    variant of dx: each launch's output rounded, launches added in order); projection 1's adapter gets exact zeros; fp32 twins within 1e-5."""
    from unigen_amd import autograd as A_
    from unigen_amd.lora import LoRALinear, fuse_adapters_autograd
    M, K, Ns = 333, 256, [128, 64, 192]
    g = torch.Generator().manual_seed(21)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    x0, dys0 = rn(M, K), [rn(M, Ns[0]), None, rn(M, Ns[2])]
    spec = [[("a", 8, 16.0), ("b", 4, 4.0)], [("c", 16, 8.0)], []]
    w0 = [rn(N, K, std=0.05) for N in Ns]
    ad0 = [[(rn(r, K, std=K ** -0.5), rn(N, r, std=0.3)) for _, r, _ in sp] for sp, N in zip(spec, Ns)]
    for dt in (torch.float32, BF):
        x = x0.to(dt).to(gpu).requires_grad_(True)
        lays = []
        for N, w, sp, ab in zip(Ns, w0, spec, ad0):
            lay = LoRALinear(K, N, bias=False, device=gpu, dtype=dt)
            with torch.no_grad():
                lay.weight.copy_(w.to(gpu))
            for (name, r, alpha), (a, b) in zip(sp, ab):
                lay.add_adapter(name, r, alpha, A=a, B=b)
                lay.lora_A[name].weight.requires_grad_(True); lay.lora_B[name].weight.requires_grad_(True)
            lays.append(lay)
        a_cat, b_bd, has = fuse_adapters_autograd([l if s else None for l, s in zip(lays, spec)], Ns, dt, gpu)
        assert has == (True, True, False) and a_cat.shape[0] == 64
        outs = A_.linear_n(x, [l.weight for l in lays], [None] * 3, lora=(a_cat, b_bd, has))
        torch.autograd.backward([outs[0], outs[2]], [dys0[0].to(dt).to(gpu), dys0[2].to(dt).to(gpu)])
        torch.cuda.synchronize()
        q = lambda t: t.to(dt)
        refs = [ref.lora_linear_bwd(q(x0), q(w0[i]), [q(a) for a, _ in ad0[i]], [q(b) for _, b in ad0[i]], [al / r for _, r, al in spec[i]], q(dys0[i]))
                for i in (0, 2)]
        dx_t = refs[0]["dx"] + refs[1]["dx"]
        dx_r = ref.bf16(refs[0]["dx_r"] + refs[1]["dx"])
        checks = [("dx", x.grad, dx_t, dx_r)]
        for j, (name, _, _) in enumerate(spec[0]):
            checks.append((f"dA.{name}", lays[0].lora_A[name].weight.grad, refs[0]["dA"][j], refs[0]["dA_r"][j]))
            checks.append((f"dB.{name}", lays[0].lora_B[name].weight.grad, refs[0]["dB"][j], refs[0]["dB_r"][j]))
        for what, got, truth, var in checks:
            e, e_row, _ = ref.err(got.detach().cpu(), truth)
            v, v_row, _ = ref.err(var, truth)
            print(f"single layer {dt} {what}: rel_l2 {e:.2e} (variant {v:.2e}) worst row {e_row:.2e} ({v_row:.2e})")
            if dt == torch.float32:
                assert e <= 1e-5 and e_row <= 1e-4, (what, e, e_row)
            else:
                assert e <= max(1.5 * v, 2.0 ** -9) and e_row <= max(1.5 * v_row, 2.0 ** -9), (what, e, v, e_row, v_row)
        for side in (lays[1].lora_A["c"], lays[1].lora_B["c"]):                   # no dy reached projection 1
            assert side.weight.grad is None or float(side.weight.grad.abs().max()) == 0.0
