"""LoRA files on the device: the in-place merge GEMM against float64 (`merge_ref`), a fused forward against the CPU oracle on host-merged weights,
live against fused, the exact undo, the forward guard, the caches a merge must invalidate, and UniGenSD3 through its pipeline.

Forward tolerances are those of tests/test_lora_gpu.py: fp32 verification twins <= 1e-3 against the fp32 oracle, the bf16 product path no further from
it than 1.25 x the oracle's own bf16 evaluation + 1e-3. Conditions on the inputs (fp32 oracle alone, asserted): the adapter moves the output by
>= 5e-2, and dropping only its merge-only entries, or only its live ones, moves the output by >= 4 bf16 tolerances - so a merge that skipped either
kind sits >= 3 tolerances from the truth. The lora_up gains below were chosen on the CPU from three seeded draws (docs/PARITY_TOLERANCES.md, "LoRA merge").

The merge bound. W' = bf16(W + P) with P = Bs A_cat accumulated in fp32 and rounded once (ug_gemm's fp32 epilogue, then ug_add_rowbcast_f32). Per element:
    |out - exact| <= 0.5 ulp_bf16(max(|out|, |exact|)) + (R + 2) 2^-24 (|W| + sum_j |Bs_nj A_jk|)
the final bf16 rounding, and fp32 accumulation of R products plus the residual add in any order. fp32 models: the second term alone. Derived, not
measured (DESIGN.md section 7a addendum)."""
import importlib

import pytest
import torch

from oracle import unigen_ref as R
from tests import lora_io_ref as LR
from tests.test_flux_gpu import CONTROL, TINY, _to_dev
from tests.util import report, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FLUX_UP_GAIN = 4.0          # on lora_up's N(0, 0.02^2): see docs/PARITY_TOLERANCES.md "LoRA merge"
SD3_UP_GAIN = 6.0
MOVED_FLOOR, EACH_OVER_TOL = 5e-2, 4.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. the merge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("adapters", [[(1, 1.0)], [(4, 2.0)], [(64, 0.5)], [(72, 0.25)], [(4, 2.0), (64, 0.375)]], ids=["r1", "r4", "r64", "r72", "r4+r64"])
@pytest.mark.parametrize("N,K", [(96, 64), (200, 192), (256, 256)])
def test_merge_against_float64(gpu, N, K, adapters, dtype):
    """One weight in the middle of a three-member pack (torch.cat + views, as engine._pack makes them); one or two adapters - two share ONE rounding."""
    from unigen_amd.engine import HipModule
    g = torch.Generator().manual_seed(N * 131 + K + len(adapters) * 7 + adapters[0][0])
    n0, n2 = 40, 24
    pack = (torch.randn(n0 + N + n2, K, generator=g) * 0.05).to(dtype).to(gpu)
    before = pack.clone()
    w = pack[n0:n0 + N]
    blocks = [((torch.randn(r, K, generator=g) / K ** 0.5).to(dtype), (torch.randn(N, r, generator=g) * 0.3).to(dtype), s) for r, s in adapters]
    HipModule._merge_into(w, [(a.to(gpu), b.to(gpu), s) for a, b, s in blocks])
    torch.cuda.synchronize()
    assert torch.equal(pack[:n0], before[:n0]) and torch.equal(pack[n0 + N:], before[n0 + N:]), "the merge wrote outside its weight"
    exact, mag, P = LR.merge_ref(before[n0:n0 + N].cpu(), blocks, dtype)
    out = w.cpu().double()
    Rk = sum(r for r, _ in adapters)
    acc = (Rk + 2) * 2.0 ** -24 * mag
    bound = acc.clone()
    if dtype == BF:
        bound += 0.5 * LR.ulp_bf16(torch.maximum(out.abs(), exact.abs()))
    err = (out - exact).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    moved = float((exact - before[n0:n0 + N].cpu().double()).abs().max())
    print(f"merge {N}x{K} {adapters} {dtype}: max err / bound = {worst:.3f}, max |delta W| = {moved:.3e}")
    assert moved > 1e-2, "the adapters barely change the weight"
    assert bool((err <= bound).all()), (worst, float(err.max()))


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", ["k60", "column_slice"])
def test_merge_of_a_misaligned_weight_is_staged(gpu, case, dtype):
    """Weights the kernels' alignment rules refuse - K_in no multiple of 8, or a column slice whose rows start 8 bytes off a 16-byte boundary - go
    through the padded temporary of `_merge_into`: same bound, nothing written around the weight."""
    from unigen_amd.engine import HipModule
    g = torch.Generator().manual_seed(5 if case == "k60" else 6)
    N, K, n0, n2 = 72, (60 if case == "k60" else 64), 16, 8
    width, c0 = (K, 0) if case == "k60" else (K + 8, 4 if dtype == BF else 2)       # 8 bytes into the row
    pack = (torch.randn(n0 + N + n2, width, generator=g) * 0.05).to(dtype).to(gpu)
    before = pack.clone()
    w = pack[n0:n0 + N, c0:c0 + K]
    assert K % 8 != 0 or w.data_ptr() % 16 != 0
    blocks = [((torch.randn(r, K, generator=g) / K ** 0.5).to(dtype), (torch.randn(N, r, generator=g) * 0.3).to(dtype), s) for r, s in [(4, 2.0), (8, 0.5)]]
    HipModule._merge_into(w, [(a.to(gpu), b.to(gpu), s) for a, b, s in blocks])
    torch.cuda.synchronize()
    band = pack.clone(); band[n0:n0 + N, c0:c0 + K] = before[n0:n0 + N, c0:c0 + K]
    assert torch.equal(band, before), "the merge wrote outside its weight"
    exact, mag, _ = LR.merge_ref(before[n0:n0 + N, c0:c0 + K].cpu(), blocks, dtype)
    out = w.cpu().double()
    bound = 14 * 2.0 ** -24 * mag
    if dtype == BF:
        bound += 0.5 * LR.ulp_bf16(torch.maximum(out.abs(), exact.abs()))
    err = (out - exact).abs()
    assert float((exact - before[n0:n0 + N, c0:c0 + K].cpu().double()).abs().max()) > 1e-2
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# forward level
# ---------------------------------------------------------------------------------------------------------------------
def _cls(name="UniGenFlux"):
    return getattr(importlib.import_module("src.UniGenTransformer"), name)


def _flux(gpu, dtype, state=None):
    m = _cls().from_config(dict(TINY), device=gpu, dtype=dtype)
    m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
    if state is None:
        m.init_synthetic_(seed=7, std=0.05, bias_std=0.02)
    else:
        res = m.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=False)
        assert not res.missing_keys and not res.unexpected_keys, res
    return m


def _shapes(state):
    return {k[:-len(".weight")]: tuple(v.shape) for k, v in state.items() if k.endswith(".weight") and v.dim() == 2}


def flux_adapter(state, gain=FLUX_UP_GAIN):
    """A kohya-named all-linear adapter on the base blocks: attention, MLPs, img_mod / txt_mod / modulation, img_in, txt_in, time_in, vector_in, final_layer."""
    return LR.make_bfl_adapter(_shapes(state), LR.bfl_modules(TINY["num_layers"], TINY["num_single_layers"]), seed=3, b_std=0.02 * gain)


def oracle_set(state, canon, rcfg, inp, t, live, fwd=None):
    """fp32 oracle outputs on host-merged weights: everything merged, nothing merged, only the live-capable modules, only the merge-only modules."""
    fwd = fwd or R.unigen_flux_forward
    run = lambda st, dt=torch.float32: fwd(st, rcfg, timestep=t, dtype=dt, **inp)[0]
    m32 = LR.merged_state(state, canon, torch.float32)
    m16 = LR.merged_state(state, canon, BF)
    o = dict(truth32=run(m32), plain=run(state), live_only=run(LR.merged_state(state, canon, torch.float32, only=set(live))),
             merge_only=run(LR.merged_state(state, canon, torch.float32, only=set(canon) - set(live))), truth16=run(m16), ref16=run(m16, BF), m32=m32)
    o["tol16"] = 1.25 * rel_l2(o["ref16"], o["truth16"]) + 1e-3
    o["moved"] = rel_l2(o["truth32"], o["plain"])
    o["without_merge_only"] = rel_l2(o["live_only"], o["truth32"])
    o["without_live"] = rel_l2(o["merge_only"], o["truth32"])
    return o


def assert_input_conditions(o):
    assert o["moved"] >= MOVED_FLOOR, f"the adapter barely changes the oracle's output ({o['moved']:.2e})"
    assert min(o["without_merge_only"], o["without_live"]) >= EACH_OVER_TOL * o["tol16"], \
        f"dropping one kind of entry moves the oracle's output by less than {EACH_OVER_TOL} bf16 tolerances: {o['without_merge_only']:.2e}, {o['without_live']:.2e}, {o['tol16']:.2e}"


@pytest.fixture(scope="module")
def world(gpu):
    model = _flux(gpu, BF)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    rcfg = R.FluxConfig(condition_nums=1, **TINY)
    inp = R.make_inputs(rcfg, B=2, grid=8, T=32)
    t = torch.full((2,), 0.75, dtype=BF)
    dinp = {k: _to_dev(v, gpu) for k, v in inp.items()}
    out0 = model(timestep=t.to(gpu), **dinp)[0].clone()
    bfl, canon = flux_adapter(state)
    live = [m for m in canon if model.lora_capable(m)]
    o = oracle_set(state, canon, rcfg, inp, t, live)
    return dict(model=model, state=state, rcfg=rcfg, inp=inp, dinp=dinp, t=t, out0=out0, bfl=bfl, canon=canon, live=live, o=o)


def _sites_off(model):
    return all(not model._lora_live([p]) for p in model._lora_sites)


def test_fused_forward_matches_oracle(world, gpu):
    w = world
    model, o, t, dinp = w["model"], w["o"], w["t"], w["dinp"]
    assert_input_conditions(o)
    rep = model.load_lora_weights(LR.write_kohya(w["bfl"]), adapter_name="style")
    try:
        assert rep.live and rep.merge_only and set(rep.live) == set(w["live"]) and set(rep.live) | set(rep.merge_only) == set(w["canon"])
        model.fuse_lora()
        out = model(timestep=t.to(gpu), **dinp)[0]
        m32 = _flux(gpu, torch.float32, w["state"])
        m32.load_lora_weights(LR.write_kohya(w["bfl"]), adapter_name="style")
        m32.fuse_lora(backup=None)
        out32 = m32(timestep=t.to(gpu), **dinp)[0]
        torch.cuda.synchronize()
        e32, err_hip = rel_l2(out32, o["truth32"]), rel_l2(out, o["truth16"])
        e_unfused = rel_l2(w["out0"], o["truth16"])
        m = report("lora_fused_forward", out, o["ref16"], err_f32_twins=e32, err_hip_vs_fp32=err_hip, tol16=o["tol16"], adapters_move_output=o["moved"],
                   without_merge_only=o["without_merge_only"], without_live=o["without_live"], err_unfused=e_unfused)
        assert e32 <= 1e-3, m
        assert err_hip <= o["tol16"], m
        assert e_unfused > o["tol16"], m                          # the adapter-free model must fail the tolerance
        assert _sites_off(model) and _sites_off(m32)
    finally:
        model.unload_lora_weights("style")
    assert torch.equal(model(timestep=t.to(gpu), **dinp)[0], w["out0"])


def test_live_versus_fused(world, gpu):
    """The file restricted to LORA_CAPABLE modules: live (the K-segment of the launches), then merged - both against the same truth."""
    w = world
    model, o, t, dinp, state = w["model"], w["o"], w["t"], w["dinp"], w["state"]
    mods = LR.bfl_modules(TINY["num_layers"], TINY["num_single_layers"])
    bfl = {k: v for k, v in w["bfl"].items() if all(model.lora_capable(m) for m in mods[k])}
    assert {m for k in bfl for m in mods[k]} == set(w["live"])
    run = lambda dt: R.unigen_flux_forward(LR.merged_state(state, w["canon"], torch.float32, only=set(w["live"])), w["rcfg"], timestep=t, dtype=dt, **w["inp"])[0]
    truth, ref16 = o["live_only"], run(BF)
    tol16 = 1.25 * rel_l2(ref16, truth) + 1e-3
    rep = model.load_lora_weights(LR.write_kohya(bfl), adapter_name="style")
    try:
        assert not rep.merge_only and set(rep.live) == set(w["live"])
        live = model(timestep=t.to(gpu), **dinp)[0].clone()
        assert not _sites_off(model)
        model.fuse_lora()
        fused = model(timestep=t.to(gpu), **dinp)[0].clone()
        assert model._lora_sites and _sites_off(model)
        mod = importlib.import_module("src.lora_switching_module")
        with mod.enable_lora(list(model.modules()), ["style"]):                # a fused adapter stays out of the launches whatever the switch says
            assert _sites_off(model)
            assert torch.equal(model(timestep=t.to(gpu), joint_attention_kwargs={"scale": 0.5}, **dinp)[0], fused)
        for lay in model._lora_sites.values():
            lay.unscale_layer(None)
        e_live, e_fused = rel_l2(live, truth), rel_l2(fused, truth)
        m = report("lora_live_vs_fused", fused, live, err_live=e_live, err_fused=e_fused, tol16=tol16, moved=rel_l2(truth, o["plain"]))
        assert rel_l2(truth, o["plain"]) >= EACH_OVER_TOL * tol16, m
        assert e_live <= tol16 and e_fused <= tol16, m
    finally:
        model.unload_lora_weights("style")


@pytest.mark.parametrize("backup", ["device", "host"])
def test_exact_undo(world, gpu, backup):
    from unigen_amd import lib as L
    w = world
    model, t, dinp = w["model"], w["t"], w["dinp"]
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sites0, mo0 = dict(model._lora_sites), dict(model._lora_merge_only)
    assert not sites0 and not mo0
    model.load_lora_weights(LR.write_kohya(w["bfl"]), adapter_name="style")
    touched = model.fuse_lora(backup=backup)
    assert set(touched) == {m + ".weight" for m in w["canon"]}
    assert all(v.device.type == ("cuda" if backup == "device" else "cpu") for v in model._lora_backup.values())
    assert not torch.equal(model.get_parameter("x_embedder.weight"), before["x_embedder.weight"])
    with pytest.raises(L.UniGenHipError, match="already fused"):
        model.fuse_lora(["style"])
    model.unfuse_lora()
    sd = model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in before.items())
    with pytest.raises(L.UniGenHipError, match="fuse_lora"):                    # unfused again: the merge-only entries are pending
        model(timestep=t.to(gpu), **dinp)
    model.unload_lora_weights("style")
    assert model._lora_sites == sites0 and model._lora_merge_only == mo0 and set(model.state_dict()) == set(before)
    assert torch.equal(model(timestep=t.to(gpu), **dinp)[0], w["out0"])


def test_no_backup_cannot_unfuse_and_unload_restores_the_registries(world, gpu):
    from unigen_amd import lib as L
    m = _flux(gpu, BF, world["state"])
    m.load_lora_weights(LR.write_kohya(world["bfl"]), adapter_name="style")
    m.fuse_lora(backup=None)
    assert m._lora_backup is None
    with pytest.raises(L.UniGenHipError, match="backup"):
        m.unfuse_lora()
    with pytest.raises(L.UniGenHipError, match="backup"):
        m.unload_lora_weights("style")


def test_guard_names_fuse_lora_and_is_a_no_op_without_a_loaded_file(world, gpu):
    from unigen_amd import lib as L
    w = world
    t, dinp = w["t"], w["dinp"]
    m = _flux(gpu, BF, w["state"])
    assert not m._lora_merge_only and not m._lora_merged and m._lora_backup is None
    # never loaded a file: the registries are empty, so the guard is a no-op and the forward gives the bits this code gave before any adapter existed in
    # the process. (That those bits are the ones of the commit before this feature is not something a test of one tree can show: the forward's
    # launches are untouched by it, and the existing parity tests of tests/test_flux_gpu.py hold them to the oracle.)
    assert torch.equal(m(timestep=t.to(gpu), **dinp)[0], w["out0"])
    m.load_lora_weights(LR.write_kohya(w["bfl"]), adapter_name="style")
    with pytest.raises(L.UniGenHipError, match="fuse_lora"):
        m(timestep=t.to(gpu), **dinp)
    m.init_trainable_param()
    with pytest.raises(L.UniGenHipError, match="fuse_lora"), torch.enable_grad():
        m(timestep=t.to(gpu), **dinp)
    from unigen_amd import training
    with pytest.raises(L.UniGenHipError, match="fuse_lora"), torch.enable_grad():
        training.flux_forward(m, timestep=t.to(gpu), **dinp)


def test_merge_invalidates_the_transposed_weight_cache(world, gpu):
    """One joint block of the differentiable forward (fp32 twins), backward before the merge - which fills autograd._wt_cache with the transposes of
    the frozen weights - and after it: dX must be that of the MERGED weights (torch autograd of the oracle's block), and differ from the earlier one."""
    from unigen_amd import autograd, training
    w = world
    state, canon = w["state"], w["canon"]
    p, D = "transformer_blocks.0", TINY["attention_head_dim"] * TINY["num_attention_heads"]
    m = _flux(gpu, torch.float32, state)
    g = torch.Generator().manual_seed(21)
    x0, enc0, temb0 = torch.randn(1, 64, D, generator=g), torch.randn(1, 32, D, generator=g), torch.randn(1, D, generator=g)
    gx, ge = torch.randn(1, 64, D, generator=g), torch.randn(1, 32, D, generator=g)
    txt_ids, img_ids = torch.zeros(32, 3), R.make_ids(8, 8).float()
    rope_dev = m._rope([txt_ids.to(gpu), img_ids.to(gpu)], None)

    def hip_dx():
        x = x0.to(gpu).requires_grad_(True)
        with torch.enable_grad():
            e_o, x_o = training._double_block(m, p, x, enc0.to(gpu), temb0.to(gpu), rope_dev, True)
            ((x_o * gx.to(gpu)).sum() + (e_o * ge.to(gpu)).sum()).backward()
        return x.grad.detach().cpu()

    def oracle_dx(st):
        x = x0.clone().requires_grad_(True)
        rope = R.flux_pos_embed(torch.cat([txt_ids, img_ids], 0), w["rcfg"].axes_dims_rope)
        e_o, x_o = R.flux_double_block({k: v.float() for k, v in st.items()}, p, w["rcfg"], x, enc0, temb0, rope)
        ((x_o * gx).sum() + (e_o * ge).sum()).backward()
        return x.grad.detach()

    dx_pre = hip_dx()
    assert autograd._wt_cache, "the backward cached no transposed weight: the test would not see a stale one"
    assert rel_l2(dx_pre, oracle_dx(state)) <= 1e-3
    m.load_lora_weights(LR.write_kohya({k: v for k, v in w["bfl"].items() if k.startswith("double_blocks.0.")}), adapter_name="style")
    m.fuse_lora()
    assert not autograd._wt_cache
    dx_post = hip_dx()
    truth = oracle_dx(LR.merged_state(state, {k: v for k, v in canon.items() if k.startswith(p + ".")}, torch.float32))
    e, apart = rel_l2(dx_post, truth), rel_l2(dx_pre, dx_post)
    print(f"merge / wt cache: relL2(dX after merge, oracle) = {e:.2e}; relL2(dX before, dX after) = {apart:.2e}")
    assert e <= 1e-3, e
    assert apart > 1e-3, apart
    m.unload_lora_weights("style")                                             # unfuses first: the original weights, and their transposes, are back
    assert torch.equal(hip_dx(), dx_pre)


# ---------------------------------------------------------------------------------------------------------------------
# 7. UniGenSD3 through its pipeline
# ---------------------------------------------------------------------------------------------------------------------
def sd3_adapter(state, n_layers, gain=SD3_UP_GAIN):
    """diffusers-named: attention (both streams, attn2), feed-forwards and the AdaLN linears of the base joint blocks, the embedders, norm_out, proj_out."""
    shapes = _shapes(state)
    leaves = ["attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_add_out", "attn2.to_q", "attn2.to_k",
              "attn2.to_v", "attn2.to_out.0", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2", "norm1.linear", "norm1_context.linear"]
    mods = [f"transformer_blocks.{i}.{x}" for i in range(n_layers) for x in leaves if f"transformer_blocks.{i}.{x}" in shapes]
    mods += ["context_embedder", "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2", "time_text_embed.text_embedder.linear_1",
             "norm_out.linear", "proj_out"]
    _, canon = LR.make_bfl_adapter(shapes, {m: [m] for m in mods}, seed=4, b_std=0.02 * gain)
    return canon


def test_sd3_pipeline_load_and_fuse_matches_oracle(gpu):
    from tests.test_sd3_gpu import TINY as SD3_TINY
    from unigen_amd.pipeline import UniGenSD3Pipeline
    cls = _cls("UniGenSD3")

    def build(dtype):
        m = cls.from_config(dict(SD3_TINY), device=gpu, dtype=dtype)
        m.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=False))
        return m

    model = build(BF)
    model.init_synthetic_(seed=5, std=0.05, bias_std=0.02)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    m32 = build(torch.float32)
    m32.load_state_dict({k: v.float() for k, v in state.items()})
    rcfg = R.SD3Config(use_modulate=False, **SD3_TINY)
    inp = R.make_sd3_inputs(rcfg, B=2, hw=16, T=24)
    t = torch.full((2,), 600.0)
    dinp = {k: v.to(gpu) for k, v in inp.items()}
    canon = sd3_adapter(state, SD3_TINY["num_layers"])
    live = [m for m in canon if model.lora_capable(m)]
    o = oracle_set(state, canon, rcfg, inp, t, live, fwd=R.unigen_sd3_forward)
    assert_input_conditions(o)
    out0 = model(timestep=t.to(gpu), **dinp)[0].clone()
    sd = LR.write_diffusers(canon)
    outs = []
    for mdl, kw in ((model, {}), (m32, dict(backup="host"))):
        pipe = UniGenSD3Pipeline(transformer=mdl)
        rep = pipe.load_lora_weights(sd, adapter_name="style")
        assert set(rep.live) == set(live) and rep.merge_only and not rep.ignored
        pipe.fuse_lora(**kw)
        outs.append(mdl(timestep=t.to(gpu), **dinp)[0])
    torch.cuda.synchronize()
    e32, err_hip, e_unfused = rel_l2(outs[1], o["truth32"]), rel_l2(outs[0], o["truth16"]), rel_l2(out0, o["truth16"])
    m = report("lora_sd3_fused_forward", outs[0], o["ref16"], err_f32_twins=e32, err_hip_vs_fp32=err_hip, tol16=o["tol16"], adapters_move_output=o["moved"],
               without_merge_only=o["without_merge_only"], without_live=o["without_live"], err_unfused=e_unfused)
    assert e32 <= 1e-3, m
    assert err_hip <= o["tol16"], m
    assert e_unfused > o["tol16"], m
    UniGenSD3Pipeline(transformer=model).unfuse_lora()
    UniGenSD3Pipeline(transformer=model).unload_lora_weights()
    assert torch.equal(model(timestep=t.to(gpu), **dinp)[0], out0)
