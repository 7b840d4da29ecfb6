"""The guidance-embedding branch (`guidance_embeds=True`, FLUX.1-dev; the reference's script/infer.sh passes --guidance_scale 3.5) on the device:
the three `guidance_embedder` MLPs (time_text_embed, control_time_text_embed, control_condition_embed - the last once per condition) behind
ug_timestep_embed at `guidance.to(bf16) * 1000`, through the inference engine, the pipeline's denoise loop, a HIP graph, the differentiable
forward and train_step - against the CPU oracle on the same seeded weights and inputs.

No tolerance of its own: the forward bounds are tests/test_flux_gpu.py's (err_hip <= 1.25 err_ref + 1e-3 against the fp32 oracle, <= 2e-2 against
the bf16 oracle, fp32 twins <= 1e-3), the gradient bounds tests/test_training_gpu.py's constants, the train_step bound tests/test_objective_gpu.py's.
The floor 5e-2 (SEEN) is a condition on the INPUTS, from the oracle alone: silencing any one embedder, or guidance 1.0 for 3.5, moves the fp32
oracle's output by 0.12 - 0.62 here (the floor itself is 2.5 x the loosest forward bound, 2e-2), so a HIP path that dropped or mis-wired one
embedder cannot pass."""
import importlib

import pytest
import torch

from oracle import unigen_ref as R
from tests.test_flux_gpu import _build, _to_dev
from tests.util import report, rel_l2

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SEEN = 5e-2
EMBEDDERS = ("time_text_embed", "control_time_text_embed", "control_condition_embed")
MODELS = {"single": ("UniGenFlux", 1), "three": ("MultiCondtionUniGenFlux", 3)}
GUIDANCE = {"mixed": [3.5, 1.0], "7": [7.0, 7.0]}          # per-sample values that differ within one batch; one value for all


def _cast32(k, v, gpu):
    """an input of the fp32 verification model: floating tensors in fp32, ids and the gate's uniform draw as they are"""
    if isinstance(v, (list, tuple)):
        return [_cast32(k, x, gpu) for x in v]
    return v.to(gpu) if (k == "gate_uniform" or k.endswith("_ids") or not v.is_floating_point()) else v.to(gpu).float()


def _twin32(gpu, cls_name, n_cond, state, **cfg_over):
    from tests.test_flux_gpu import CONTROL, TINY
    cls = getattr(importlib.import_module("src.UniGenTransformer"), cls_name)
    m32 = cls.from_config(dict(TINY, **cfg_over), device=gpu, dtype=F32)
    m32.init_condition_block(condition_nums=n_cond, condition_types=["canny", "depth", "openpose"][:n_cond], control_params=dict(CONTROL))
    m32.load_state_dict({k: v.float() for k, v in state.items()})
    return m32


@pytest.fixture(scope="module")
def built(gpu):
    """{"single" | "three": (bf16 model, state, oracle config)}: built once, the state is shared and never written"""
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = _build(gpu, *MODELS[which], guidance_embeds=True)
            assert sum(".guidance_embedder." in k for k in cache[which][1]) == 12
        return cache[which]
    return get


@pytest.mark.parametrize("which,gname,B,grid,T", [("single", "mixed", 2, 8, 32), ("single", "7", 2, 8, 32), ("three", "mixed", 2, 8, 32), ("three", "7", 2, 8, 32),
                                                  ("single", "mixed", 1, 6, 20)])
def test_forward_with_guidance_matches_oracle(gpu, built, which, gname, B, grid, T):
    """tests/test_flux_gpu.py::test_forward_matches_oracle with a guidance tensor, plus the fp32 verification twins"""
    (cls_name, n_cond), (model, state, rcfg) = MODELS[which], built(which)
    inp = R.make_inputs(rcfg, B=B, grid=grid, T=T, n_cond=n_cond)
    t = torch.full((B,), 0.75, dtype=BF)
    g = torch.tensor(GUIDANCE[gname][:B])
    truth, _, _ = R.unigen_flux_forward(state, rcfg, timestep=t, guidance=g, dtype=F32, **inp)
    ref16, loss16, cnt16 = R.unigen_flux_forward(state, rcfg, timestep=t, guidance=g, dtype=BF, **inp)
    out, losses, outs = model(timestep=t.to(gpu), guidance=g.to(gpu), conditioning_scale=1.0, **{k: _to_dev(v, gpu) for k, v in inp.items()})
    torch.cuda.synchronize()
    assert out.shape == truth.shape and out.dtype == BF
    err_hip, err_ref = rel_l2(out, truth), rel_l2(ref16, truth)
    m32 = _twin32(gpu, cls_name, n_cond, state, guidance_embeds=True)
    out32 = m32(timestep=t.to(gpu), guidance=g.to(gpu), **{k: _cast32(k, v, gpu) for k, v in inp.items()})[0]
    e32 = rel_l2(out32, truth)
    m = report(f"forward_guidance_{which}_{gname}_B{B}_g{grid}", out, ref16, err_hip_vs_fp32=err_hip, err_oraclebf16_vs_fp32=err_ref, err_f32_twins=e32)
    assert torch.isfinite(out.float()).all()
    assert err_hip <= 1.25 * err_ref + 1e-3, m
    assert m["rel_l2"] <= 2e-2, m
    assert torch.equal(outs["expert_counts"].cpu(), cnt16["expert_counts"]), (outs["expert_counts"], cnt16["expert_counts"])
    assert abs(float(losses["moe_loss"]) - float(loss16["moe_loss"])) <= 1e-3 * abs(float(loss16["moe_loss"]))
    assert e32 <= 1e-3, m


@pytest.mark.parametrize("which", list(MODELS))
def test_the_oracle_sees_every_guidance_embedder(built, which):
    """Conditions on the inputs of the test above (oracle only, fp32): with any ONE embedder's guidance MLP silenced (linear_2 weight and bias
    zeroed), and with guidance 1.0 in place of 3.5, the truth moves by at least SEEN - for each guidance tensor the parity test uses."""
    (_, n_cond), (_, state, rcfg) = MODELS[which], built(which)
    inp = R.make_inputs(rcfg, B=2, grid=8, T=32, n_cond=n_cond)
    t = torch.full((2,), 0.75, dtype=BF)
    fwd = lambda st, g: R.unigen_flux_forward(st, rcfg, timestep=t, guidance=g, dtype=F32, **inp)[0]
    seen = {}
    for gname, vals in GUIDANCE.items():
        g = torch.tensor(vals)
        truth = fwd(state, g)
        for p in EMBEDDERS:
            st = dict(state)
            for s in ("weight", "bias"):
                st[f"{p}.guidance_embedder.linear_2.{s}"] = torch.zeros_like(state[f"{p}.guidance_embedder.linear_2.{s}"])
            seen[f"{gname}: {p} silenced"] = rel_l2(fwd(st, g), truth)
    seen["3.5 vs 1.0"] = rel_l2(fwd(state, torch.full((2,), 1.0)), fwd(state, torch.full((2,), 3.5)))
    print(f"guidance sensitivity, {which}: " + ", ".join(f"{k} {v:.3f}" for k, v in seen.items()))
    assert min(seen.values()) >= SEEN, seen


def test_flag_semantics_and_repeatability(gpu, built):
    model, state, rcfg = built("single")
    inp = {k: _to_dev(v, gpu) for k, v in R.make_inputs(rcfg, B=2, grid=8, T=32).items()}
    t = torch.full((2,), 0.5, dtype=BF, device=gpu)
    g = torch.tensor([3.5, 1.0], device=gpu)
    with pytest.raises(ValueError, match="guidance"):
        model(timestep=t, **inp)
    with pytest.raises(ValueError, match="guidance"):
        model(timestep=t, guidance=None, **inp)
    # two identical calls: the timestep MLP and the guidance MLP share the `tte_h` workspace, a stale row of either would show here
    a = model(timestep=t, guidance=g, **inp)[0].clone()
    b = model(timestep=t, guidance=g, **inp)[0].clone()
    assert torch.equal(a, b)
    c = model(timestep=t, guidance=g.flip(0), **inp)[0].clone()
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert torch.equal(model(timestep=t, guidance=g, **inp)[0], a)           # and after a call with other guidance
    # the differentiable forward refuses a missing guidance too
    model.init_trainable_param()
    try:
        with pytest.raises(ValueError, match="guidance"):
            model(timestep=t, **inp)
    finally:
        model.requires_grad_(False)
    # guidance_embeds=False: a guidance tensor is ignored, bit for bit
    plain, _, rcfg0 = _build(gpu, "UniGenFlux", 1)
    assert not any(".guidance_embedder." in k for k in plain.state_dict())
    assert torch.equal(plain(timestep=t, guidance=g, **inp)[0].clone(), plain(timestep=t, **inp)[0])


def test_pipeline_passes_guidance_scale_to_the_model(gpu, built):
    """UniGenFLUXPipeline(guidance_scale=3.5) on a guidance model: denoise_loop's `full([B], guidance_scale)` against the oracle's loop"""
    model, state, rcfg = built("single")
    inp = R.make_inputs(rcfg, B=2, grid=8, T=32)
    uni = [inp["gate_uniform"]] * 2
    fw = {k: v for k, v in inp.items() if k not in ("hidden_states", "gate_uniform")}
    ref, ref1 = (R.denoise(state, rcfg, latents=inp["hidden_states"], num_steps=2, dtype=BF, gate_uniforms=uni, guidance=torch.full((2,), s), **fw) for s in (3.5, 1.0))
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=None)
    pipe.transformer = model
    res = pipe(prompt_embeds=inp["encoder_hidden_states"], pooled_prompt_embeds=inp["pooled_projections"],
               condition_pooled_prompt_embeds=inp["condition_pooled_projections"], control_image=inp["condition_hidden_states"],
               latents=inp["hidden_states"], height=128, width=128, num_inference_steps=2, guidance_scale=3.5, output_type="latent", dtype=BF,
               gate_uniforms=[inp["gate_uniform"].to(gpu)] * 2)
    m = report("denoise2_guidance_3.5", res.images, ref, scale_moves_output=rel_l2(ref1, ref))
    assert m["scale_moves_output"] > SEEN, m                # the scale demonstrably reaches the model
    assert m["rel_l2"] <= 2e-2, m


def test_denoise_step_with_guidance_is_hip_graph_capturable(gpu, built):
    """tests/test_flux_gpu.py::test_denoise_step_is_hip_graph_capturable on the guidance model (the loop also builds the guidance tensor on the
    device): one stream, a single branch; the replay is bitwise identical to the eager run."""
    from unigen_amd.pipeline import denoise_loop, prepare_latent_image_ids
    model, state, rcfg = built("single")
    inp = {k: _to_dev(v, gpu) for k, v in R.make_inputs(rcfg, B=2, grid=8, T=32).items()}
    ids, txt = prepare_latent_image_ids(8, 8, gpu, BF), torch.zeros(32, 3, device=gpu, dtype=BF)
    lat0 = inp["hidden_states"].clone()

    def step(scale=3.5):
        return denoise_loop(model, latents=lat0.clone(), control_tokens=inp["condition_hidden_states"], prompt_embeds=inp["encoder_hidden_states"],
                            pooled_prompt_embeds=inp["pooled_projections"], condition_pooled_prompt_embeds=inp["condition_pooled_projections"],
                            text_ids=txt, latent_image_ids=ids, condition_ids=ids, num_inference_steps=2, guidance_scale=scale,
                            gate_uniforms=[inp["gate_uniform"]] * 2)
    eager = step().clone()
    assert not torch.equal(step(1.0), eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_guidance_embedder_gradients_match_oracle_autograd(gpu):
    """tests/test_training_gpu.py::test_control_module_gradients_match_oracle_autograd, case (1, "UniGenFlux", 1), on a guidance model with guidance
    [3.5, 1.0] - its assertions and tolerances, then the control branch's guidance embedders one parameter at a time."""
    from tests import test_training_gpu as TT
    r = TT.check_control_module_gradients(gpu, 1, "UniGenFlux", 1, guidance=torch.tensor([3.5, 1.0]), guidance_embeds=True)
    names, truth, z = r["names"], r["truth"], r["z"]
    mine = [f"{p}.guidance_embedder.linear_{i}.{s}" for p in EMBEDDERS[1:] for i in (1, 2) for s in ("weight", "bias")]
    assert all(p in r["model"].trainable_control_modules for p in EMBEDDERS[1:]) and set(mine) <= set(names) and not set(mine) & r["dead"]
    # the base model's embedder is frozen: not trainable, and (asserted inside the shared check) no frozen parameter received a gradient
    assert "time_text_embed" not in r["model"].trainable_control_modules and not any(n.startswith("time_text_embed.") for n in names)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for k in mine:
        assert float(truth[k].abs().max()) > 0 and float(z(r["g32"], k).abs().max()) > 0 and float(z(r["g16"], k).abs().max()) > 0, k
        e = float((z(r["g32"], k) - truth[k]).norm() / max(float(truth[k].norm()), r["floor"]))
        assert e <= TT.F32_WORST_PARAM, (k, e)
    cat = lambda d: torch.cat([z(d, k).flatten() for k in mine])
    e32, e_hip, e_ref = rel(cat(r["g32"]), cat(truth)), rel(cat(r["g16"]), cat(truth)), rel(cat(r["gref"]), cat(truth))
    report("train_guidance_embedder_grads", cat(r["g16"]), cat(truth), err_f32_twins=e32, err_hip_vs_fp32=e_hip, err_oraclebf16_vs_fp32=e_ref)
    assert e32 <= TT.F32_GRADS and e_hip <= TT.GRAD_BF16[0] * e_ref + TT.GRAD_BF16[1], (e32, e_hip, e_ref)


def test_train_step_supplies_the_guidance(gpu):
    """objective.train_step(guidance_scale=3.5) on the fp32-twin guidance model (train.py:616-620: `full(guidance_scale).expand(B)`), one micro-step
    that ends in the optimizer step, against the same step written with the eager objective around the same forward - as
    tests/test_objective_gpu.py::test_train_step_matches_the_eager_objective; loss to 1e-5. Without guidance_scale: ValueError."""
    from tests import objective_ref as OR
    from tests.test_objective_gpu import TABLE, _unpack
    from tests.test_training_gpu import CONTROL, TINY, _dev
    from unigen_amd import objective as O
    from unigen_amd import optim
    from unigen_amd.pipeline import pack_latents
    cls = importlib.import_module("src.UniGenTransformer").UniGenFlux
    B, grid, T, C = 2, 8, 64, 16
    H = W = 2 * grid
    cfg = dict(TINY, guidance_embeds=True)
    rcfg = R.FluxConfig(condition_nums=1, **cfg)
    inp = R.make_inputs(rcfg, B=B, grid=grid, T=T)
    inp.pop("hidden_states")
    kw = {k: _dev(v, gpu, F32 if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    gen = torch.Generator().manual_seed(21)
    batch = dict(latents=torch.randn(B, C, H, W, generator=gen).to(BF).float().to(gpu), noise=torch.randn(B, C, H, W, generator=gen).to(BF).float().to(gpu),
                 u=torch.tensor((0.25, 0.731), dtype=F32, device=gpu))
    state = {}

    def build():
        model = cls.from_config(dict(cfg), device=gpu, dtype=F32)
        model.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
        if not state:
            model.init_synthetic_(seed=3, std=0.05, bias_std=0.02)
            state.update({k: v.detach().clone() for k, v in model.state_dict().items()})
        else:
            model.load_state_dict(state)
        model.init_trainable_param()
        return model, optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2)

    model, opt = build()
    obj = O.FlowMatchObjective("none")
    with pytest.raises(ValueError, match="guidance_scale"):
        O.train_step(model, opt, obj, dict(batch, **kw))
    assert getattr(opt, "_unigen_micro_steps", 0) == 0 and all(p.grad is None for p in model.parameters())
    out = O.train_step(model, opt, obj, dict(batch, **kw), max_grad_norm=1.0, guidance_scale=3.5)

    model_e, opt_e = build()
    s32 = TABLE.to(gpu)[(batch["u"] * OR.T_TRAIN).long().clamp(max=OR.T_TRAIN - 1)]
    sig = s32.reshape(-1, 1, 1, 1)
    noisy = (1.0 - sig) * batch["latents"] + sig * batch["noise"]
    run = lambda s: model_e(hidden_states=pack_latents(noisy), timestep=s32 * OR.T_TRAIN / 1000, guidance=torch.full((B,), s, device=gpu), **kw)
    pred, add, _ = run(3.5)
    target = batch["noise"] - batch["latents"]
    loss = torch.mean(((_unpack(pred, C, H, W).float() - target.float()) ** 2).reshape(B, -1), 1).mean() + sum(list(add.values()))
    loss.backward()
    norm_e = optim.clip_grad_norm_([p for p in model_e.parameters() if p.requires_grad], 1.0)
    with torch.no_grad():
        pred1 = run(1.0)[0]
    rel = abs(float(out["step_loss"]) - float(loss)) / abs(float(loss))
    print(f"train_step with guidance: loss {float(out['step_loss']):.7f} vs eager {float(loss):.7f} (rel {rel:.2e}); guidance 1.0 moves the prediction {rel_l2(pred1, pred.detach()):.3f}")
    assert rel_l2(pred1, pred.detach()) > SEEN                # the eager side would not match with another scale
    assert rel <= 1e-5, (float(out["step_loss"]), float(loss))
    assert torch.equal(out["grad_norm"], norm_e), (float(out["grad_norm"]), float(norm_e))
