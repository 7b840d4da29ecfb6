"""Training through unigen_amd.sana: loss and gradients of SanaTransformerBlock and the 2-layer SanaTransformer2DModel after set_trainable(), against
float64 autograd of tests/sana_ref.SanaBlockRef / SanaModelRef on the same seeded weights and inputs (tiny configurations "a" and "b", all four
TINY_RUNS). The loss is the mean of (output x a fixed seeded tensor); compared are the gradients of every parameter and of hidden_states /
encoder_hidden_states.

Bounds (tests/test_training_gpu.py's; docs/PARITY_TOLERANCES.md, "Sana backward"): fp32 parameters (the `_f32` twins end to end) - all gradients
together within rel-L2 1e-3 of float64, the worst single tensor within 5e-3; bf16 - e_hip <= 1.5 e_ref + 5e-3, e_ref the reference's own bf16 autograd
on the CPU. Also: checkpointing on / off and two runs give the same bits; parameters outside set_trainable() get no gradient; after one AdamW step
the next forward - inference included - runs on the updated weights; without set_trainable() the "inference only" refusal stands."""
import pytest
import torch

from tests import sana_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
F32_GRADS, F32_WORST, GRAD_BF16 = 1e-3, 5e-3, (1.5, 5e-3)
# The bf16 loss. tests/test_training_gpu.py bounds its loss relative to the loss (3e-2); that loss is a mean of squares. This one is a mean of SIGNED
# products that cancels to about a hundredth of mean |output x weight|, while the elements' bf16 errors (2^-9 relative each) do not cancel with it: the
# reference's own bf16 evaluation is up to 6 % of the loss away. So the error is measured against the cancellation-free magnitude mean |output x weight|
# of the float64 evaluation and bounded in the gradients' form: e_hip <= 1.5 e_ref + 5e-3.
LOSS_BF16 = (1.5, 5e-3)
BLOCK_KW = ("num_attention_heads", "attention_head_dim", "num_cross_attention_heads", "cross_attention_head_dim", "cross_attention_dim", "attention_bias",
            "norm_eps", "mlp_ratio")
PRE = "transformer_blocks.0."
INPUTS = ("hidden_states", "encoder_hidden_states")
_CACHE = {}


def _weights(name):
    if ("w", name) not in _CACHE:
        _CACHE[("w", name)] = R.tiny_state_dict(name)
    return _CACHE[("w", name)]


def _loss_weight(shape, run, kind):
    """the fixed tensor of the loss: N(0, 1) on the bf16 grid, so that every evaluation reads the same numbers"""
    g = torch.Generator().manual_seed(9100 + 10 * run + (kind == "model"))
    return torch.randn(shape, generator=g).to(BF)


def _inputs(run, kind):
    name, H, W, T, _ = R.TINY_RUNS[run]
    if kind == "model":
        i = R.tiny_inputs(run)
        return i["x"], i["enc"], i["t"], i["mask"]
    b = R.block_inputs(run)
    return b["h"], b["enc"], b["t"], b["mask"]


def _reference(run, kind, dtype):
    """-> (loss, {name: gradient as float64}) of the plain-torch reference evaluated in `dtype` on the CPU; once per process"""
    key = ("ref", run, kind, dtype)
    if key not in _CACHE:
        name, H, W, T, _ = R.TINY_RUNS[run]
        m = R.build_ref(name, _weights(name), dtype)
        x, enc, t, mask = _inputs(run, kind)
        x, enc = x.to(dtype).requires_grad_(True), enc.to(dtype).requires_grad_(True)
        if kind == "model":
            out, params = m(x, enc, t.to(F64) if dtype == F64 else t, mask), dict(m.named_parameters())
        else:
            blk = m.transformer_blocks[0]
            out, params = blk(x, None, enc, mask, t.to(dtype), H, W), dict(blk.named_parameters())
        loss = (out.to(F64 if dtype == F64 else F32) * _loss_weight(out.shape, run, kind).to(F64 if dtype == F64 else F32)).mean()
        loss.backward()
        g = {k: p.grad.to(F64) for k, p in params.items()}
        g["hidden_states"], g["encoder_hidden_states"] = x.grad.to(F64), enc.grad.to(F64)
        if dtype == F64:
            _CACHE[("scale", run, kind)] = float((out.detach() * _loss_weight(out.shape, run, kind).to(F64)).abs().mean())
        _CACHE[key] = (float(loss.detach()), g)
    return _CACHE[key]


def _build(run, kind, dtype, dev):
    from unigen_amd.sana import SanaTransformer2DModel, SanaTransformerBlock
    name = R.TINY_RUNS[run][0]
    c, sd = R.TINY[name], _weights(name)
    if kind == "model":
        m = SanaTransformer2DModel(c, device=dev, dtype=dtype)
        m.load_state_dict(sd)
    else:
        m = SanaTransformerBlock(c["num_attention_heads"] * 32, **{k: c[k] for k in BLOCK_KW}, device=dev, dtype=dtype)
        m.load_state_dict({k[len(PRE):]: v for k, v in sd.items() if k.startswith(PRE)})
    return m


def _call(m, run, kind, dtype, dev, grad_inputs=True):
    """one forward: -> (out, x, enc)"""
    name, H, W, T, _ = R.TINY_RUNS[run]
    x, enc, t, mask = _inputs(run, kind)
    x, enc = x.to(dev, dtype).requires_grad_(grad_inputs), enc.to(dev, dtype).requires_grad_(grad_inputs)
    mask = None if mask is None else mask.to(dev)
    out = m(x, enc, t.to(dev), mask) if kind == "model" else m(x, None, enc, mask, t.to(dev, dtype), H, W)
    return out, x, enc


def _hip(run, kind, dtype, dev, patterns=True, ckpt=False):
    """-> (loss, {name: gradient tensor on the device, None where there is none}, the module)"""
    m = _build(run, kind, dtype, dev).set_trainable(patterns)
    if ckpt:
        m.enable_gradient_checkpointing()
    out, x, enc = _call(m, run, kind, dtype, dev)
    loss = (out.float() * _loss_weight(out.shape, run, kind).to(dev).float()).mean()
    loss.backward()
    torch.cuda.synchronize()
    g = {k: t.grad for k, t in m.state_dict().items()}
    g["hidden_states"], g["encoder_hidden_states"] = x.grad, enc.grad
    return float(loss.detach()), g, m


def _errs(g, truth):
    cat = lambda d: torch.cat([d[k].detach().to(F64).cpu().flatten() for k in truth])
    gt = cat(truth)
    e_all = float((cat(g) - gt).norm() / gt.norm())
    floor = 1e-3 * float(gt.norm()) / len(truth) ** 0.5               # a gradient that is itself rounding noise does not count (tests/test_training_gpu.py)
    worst = max((float((g[k].detach().to(F64).cpu() - truth[k]).norm() / max(float(truth[k].norm()), floor)), k) for k in truth)
    return e_all, worst


@pytest.mark.parametrize("kind", ["block", "model"])
@pytest.mark.parametrize("run", range(len(R.TINY_RUNS)))
def test_gradients_against_float64_autograd(gpu, run, kind):
    truth_loss, truth = _reference(run, kind, F64)
    loss32, g32, m = _hip(run, kind, F32, gpu)
    assert set(m.trainable_parameters()) == set(truth) - set(INPUTS) and all(g32[k] is not None for k in truth), "every parameter and both inputs take a gradient"
    e_all, worst = _errs(g32, truth)
    print(f"{kind} run {run} fp32: loss {loss32:.6f} vs {truth_loss:.6f}; all gradients rel-L2 {e_all:.3e} (bound {F32_GRADS:.0e}); worst {worst[1]} {worst[0]:.3e} "
          f"({F32_WORST:.0e})")
    assert abs(loss32 - truth_loss) <= 1e-4 * abs(truth_loss) + 1e-6 and e_all <= F32_GRADS and worst[0] <= F32_WORST, (loss32, truth_loss, e_all, worst)
    ref_loss, gref = _reference(run, kind, BF)
    loss16, g16, _ = _hip(run, kind, BF, gpu)
    assert all(bool(torch.isfinite(g16[k]).all()) for k in truth)
    e_hip, e_ref = _errs(g16, truth)[0], _errs(gref, truth)[0]
    print(f"{kind} run {run} bf16: loss {loss16:.5f} (reference bf16 {ref_loss:.5f}, float64 {truth_loss:.5f}); gradients vs float64: hip {e_hip:.3e}, "
          f"reference bf16 {e_ref:.3e}, bound {GRAD_BF16[0] * e_ref + GRAD_BF16[1]:.3e}")
    assert e_hip <= GRAD_BF16[0] * e_ref + GRAD_BF16[1], (e_hip, e_ref)
    scale = _CACHE[("scale", run, kind)]
    l_hip, l_ref = abs(loss16 - truth_loss) / scale, abs(ref_loss - truth_loss) / scale
    print(f"{kind} run {run} bf16 loss error over mean |output x weight| = {scale:.4f}: hip {l_hip:.3e}, reference bf16 {l_ref:.3e}, "
          f"bound {LOSS_BF16[0] * l_ref + LOSS_BF16[1]:.3e}")
    assert l_hip <= LOSS_BF16[0] * l_ref + LOSS_BF16[1], (loss16, ref_loss, truth_loss, scale)


@pytest.mark.parametrize("kind", ["block", "model"])
def test_checkpointing_and_a_second_run_give_the_same_bits(gpu, kind):
    run = 2                                                            # configuration "b", a prefix mask with two different lengths
    _, g0, _ = _hip(run, kind, BF, gpu)
    _, g1, _ = _hip(run, kind, BF, gpu)
    _, g2, _ = _hip(run, kind, BF, gpu, ckpt=True)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), ("two backward runs differ", k)
        assert torch.equal(g0[k], g2[k]), ("gradient checkpointing changes the gradient", k)


def test_only_the_selected_parameters_take_gradients(gpu):
    run = 1
    pats = ["transformer_blocks.1.attn2.*", "transformer_blocks.1.ff.conv_depth.*", "proj_out.weight", "caption_norm.weight"]
    import fnmatch
    _, g, m = _hip(run, "model", BF, gpu, patterns=pats)
    chosen = {k for k in m.state_dict() if any(fnmatch.fnmatchcase(k, p) for p in pats)}
    assert len(chosen) == 12 and set(m.trainable_parameters()) == chosen
    for k in m.state_dict():
        assert (g[k] is not None) == (k in chosen), k
    # the frozen parameters run from their packed copies: the selected gradients and the inputs' are still the reference's, by the bf16 bound
    truth = {k: v for k, v in _reference(run, "model", F64)[1].items() if k in chosen or k in INPUTS}
    e_hip, e_ref = _errs(g, truth)[0], _errs(_reference(run, "model", BF)[1], truth)[0]
    print(f"selected parameters: hip {e_hip:.3e}, reference bf16 {e_ref:.3e}")
    assert e_hip <= GRAD_BF16[0] * e_ref + GRAD_BF16[1], (e_hip, e_ref)
    _, g, m = _hip(run, "block", BF, gpu, patterns=False)             # nothing trainable: the gradients still reach the inputs
    assert not m.trainable_parameters() and all(g[k] is None for k in m.state_dict()) and g["hidden_states"] is not None


@pytest.mark.parametrize("dtype", [F32, BF])
def test_a_forward_after_an_optimizer_step_sees_the_new_weights(gpu, dtype):
    from unigen_amd.optim import AdamW
    from unigen_amd.sana import SanaTransformer2DModel
    run, kind = 1, "model"
    name = R.TINY_RUNS[run][0]
    _, _, m = _hip(run, kind, dtype, gpu)
    with torch.no_grad():
        before = _call(m, run, kind, dtype, gpu, grad_inputs=False)[0].clone()
    opt = AdamW(list(m.trainable_parameters().values()), lr=1e-2, weight_decay=0.0)
    opt.step()
    torch.cuda.synchronize()
    with torch.no_grad():
        after = _call(m, run, kind, dtype, gpu, grad_inputs=False)[0].clone()       # the inference path, on the re-packed copies
    out_train = _call(m, run, kind, dtype, gpu)[0].detach()                         # the differentiable path reads the named tensors
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(sd[k].cpu().to(F32), _weights(name)[k].to(F32)) for k in sd), "the step moved nothing"
    fresh = SanaTransformer2DModel(R.TINY[name], device=gpu, dtype=dtype)
    fresh.load_state_dict(sd)
    with torch.no_grad():
        want = _call(fresh, run, kind, dtype, gpu, grad_inputs=False)[0]
    assert torch.equal(after, want), "the forward after the step does not run on the updated weights (stale packed copies)"
    rel = lambda a, b: float((a.to(F64).cpu() - b.to(F64).cpu()).norm() / b.to(F64).cpu().norm())
    # against the reference with the same update, in float64
    ref = R.build_ref(name, {k: v.cpu() for k, v in sd.items()}, F64)
    x, enc, t, mask = _inputs(run, kind)
    with torch.no_grad():
        truth = ref(x.to(F64), enc.to(F64), t.to(F64), mask)
        if dtype == BF:
            e_ref = rel(R.build_ref(name, {k: v.cpu() for k, v in sd.items()}, BF)(x, enc, t, mask), truth)
    e_after, e_train, e_before = rel(after, truth), rel(out_train, truth), rel(before, truth)
    bound = 1e-3 if dtype == F32 else 1.25 * e_ref                    # the forward's bounds (tests/test_sana_gpu.py)
    print(f"{dtype}: after the step {e_after:.3e} (training path {e_train:.3e}) from the updated reference, bound {bound:.3e}; the old output {e_before:.3e}")
    assert not torch.equal(before, after) and e_before > 2 * bound, ("the step is too small to be seen", e_before, bound)
    assert e_after <= bound and e_train <= (bound if dtype == F32 else 1.5 * e_ref + 5e-3), (e_after, e_train, bound)


def test_steps_of_a_partly_trainable_model_keep_memory_flat(gpu):
    """Frozen parameters run from their packed copies, whose transposes autograd caches by address and version. An optimizer step must not make the
    copies of UNCHANGED parameters move (each move would leave a pinned transpose behind), and a copy that packs a trainable tensor beside a
    frozen one (to_k | to_v) is rebuilt in its buffer with its stale transposes dropped: the cache and the allocated bytes stay what they are."""
    from unigen_amd import autograd as A
    from unigen_amd.optim import AdamW
    run, kind = 1, "model"
    pats = ["transformer_blocks.1.attn2.to_k.*", "transformer_blocks.0.attn1.to_q.weight", "transformer_blocks.1.ff.conv_inverted.*"]
    m = _build(run, kind, BF, gpu).set_trainable(pats)
    opt = AdamW(list(m.trainable_parameters().values()), lr=1e-3, weight_decay=0.0)
    seen = []
    for step in range(6):
        for t in m.trainable_parameters().values():
            t.grad = None
        out = _call(m, run, kind, BF, gpu)[0]
        (out.float() * _loss_weight(out.shape, run, kind).to(gpu).float()).mean().backward()
        opt.step()
        with torch.no_grad():
            del out
            _call(m, run, kind, BF, gpu, grad_inputs=False)           # an inference forward between the steps: the in-place rebuilds
        A.clear_activation_cache()
        torch.cuda.synchronize()
        seen.append((len(A._wt_cache), torch.cuda.memory_allocated()))
    print("transposes cached / bytes allocated after each step:", seen)
    assert seen[2][0] > 0 and all(s == seen[2] for s in seen[3:]), seen


def test_load_state_dict_after_the_opt_in_keeps_the_selection(gpu):
    run, kind = 1, "model"
    pats = ["transformer_blocks.1.attn2.*", "proj_out.weight"]
    _, g0, m = _hip(run, kind, BF, gpu, patterns=pats)
    chosen = set(m.trainable_parameters())
    m.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    assert set(m.trainable_parameters()) == chosen and len(chosen) == 9
    out, x, enc = _call(m, run, kind, BF, gpu)
    (out.float() * _loss_weight(out.shape, run, kind).to(gpu).float()).mean().backward()
    for k, t in m.state_dict().items():                               # the blocks hold the new leaves: the same gradients arrive at them
        assert (t.grad is not None) == (k in chosen) and (t.grad is None or torch.equal(t.grad, g0[k])), k


def test_without_the_opt_in_the_refusal_stands(gpu):
    for kind in ("block", "model"):
        m = _build(1, kind, BF, gpu)
        with pytest.raises(RuntimeError, match="inference only"):
            _call(m, 1, kind, BF, gpu)
        assert m.trainable_parameters() == {}
        m.set_trainable(True)
        with pytest.raises(NotImplementedError, match="attention_mask.*follow-up"):
            x, enc, t, mask = _inputs(1, kind)
            am = torch.ones(2, 64, device=gpu)
            m(x.to(gpu), enc.to(gpu), t.to(gpu), None, am) if kind == "model" else m(x.to(gpu), am, enc.to(gpu), None, t.to(gpu), 8, 8)
