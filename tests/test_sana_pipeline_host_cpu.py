"""Host logic of unigen_amd/sana_pipeline.py without a GPU: what the scheduler, the pipeline and the ug_dpm_step entry refuse, loading from a
directory, and the loop's bookkeeping (prompt rows, masks, the learned-sigma chunk, callbacks, output_type="latent") on stand-in components, with
ops.dpm_step replaced by the CPU op sequence of tests/sana_pipeline_ref.py. The entry is called with fake aligned pointers: every refusal comes
before any launch."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sana_pipeline_ref as R
from unigen_amd import sana_pipeline as SP
from unigen_amd.sana_pipeline import DPMSolverMultistepScheduler, SANA_SCHEDULER_CONFIG, SanaPipeline, SanaPipelineOutput, sana_denoise_loop

BF, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------- the scheduler ------------------------------------------------------------
@pytest.mark.parametrize("kw, names", [
    (dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(use_exponential_sigmas=True), "use_exponential_sigmas"),
    (dict(use_beta_sigmas=True), "use_beta_sigmas"), (dict(use_lu_lambdas=True), "use_lu_lambdas"), (dict(thresholding=True), "thresholding"),
    (dict(algorithm_type="sde-dpmsolver++"), "sde-dpmsolver"), (dict(algorithm_type="sde-dpmsolver"), "sde-dpmsolver"), (dict(algorithm_type="dpmsolver"), "dpmsolver"),
    (dict(solver_order=3), "solver_order = 3"), (dict(solver_order=0), "solver_order = 0"), (dict(solver_type="heun"), "heun"),
    (dict(prediction_type="epsilon"), "epsilon"), (dict(prediction_type="sample"), "sample"), (dict(prediction_type="v_prediction"), "v_prediction"),
    (dict(euler_at_final=True), "euler_at_final"), (dict(final_sigmas_type="sigma_min"), "sigma_min"), (dict(use_flow_sigmas=False), "use_flow_sigmas"),
    (dict(lower_order_final=False), "lower_order_final"), (dict(variance_type="learned"), "variance_type"),
])
def test_scheduler_refuses_what_it_does_not_implement(kw, names):
    with pytest.raises(NotImplementedError, match=names):
        DPMSolverMultistepScheduler(**dict(SANA_SCHEDULER_CONFIG, **kw))


def test_scheduler_defaults_are_diffusers_and_unknown_keys_raise():
    with pytest.raises(NotImplementedError, match="epsilon"):                    # diffusers' default prediction type: a config must say flow_prediction
        DPMSolverMultistepScheduler()
    with pytest.raises(ValueError, match=r"\['flow_shfit'\]"):
        DPMSolverMultistepScheduler(**dict(SANA_SCHEDULER_CONFIG, flow_shfit=3.0))
    s = DPMSolverMultistepScheduler(**dict(SANA_SCHEDULER_CONFIG, _class_name="DPMSolverMultistepScheduler", _diffusers_version="0.32.2", solver_order=1))
    assert s.config.num_train_timesteps == 1000 and s.config.flow_shift == 3.0 and s.config.solver_order == 1 and s.init_noise_sigma == 1.0
    x = torch.zeros(3)
    assert s.scale_model_input(x, 5) is x


def test_scheduler_from_config_and_from_pretrained(tmp_path):
    cfg = dict(SANA_SCHEDULER_CONFIG, _class_name="DPMSolverMultistepScheduler", beta_schedule="linear", num_train_timesteps=1000)
    a = DPMSolverMultistepScheduler.from_config(cfg)
    b = DPMSolverMultistepScheduler.from_config(a.config, flow_shift=2.0)
    assert a.config.flow_shift == 3.0 and b.config.flow_shift == 2.0
    d = tmp_path / "model" / "scheduler"
    d.mkdir(parents=True)
    (d / "scheduler_config.json").write_text(json.dumps(cfg))
    for s in (DPMSolverMultistepScheduler.from_pretrained(d), DPMSolverMultistepScheduler.from_pretrained(tmp_path / "model", subfolder="scheduler"),
              DPMSolverMultistepScheduler.from_pretrained(d / "scheduler_config.json")):
        assert vars(s.config) == vars(a.config)
    with pytest.raises(OSError, match="not a local scheduler_config.json"):
        DPMSolverMultistepScheduler.from_pretrained(tmp_path / "nowhere")
    (d / "scheduler_config.json").write_text(json.dumps(dict(cfg, use_karras_sigmas=True)))
    with pytest.raises(NotImplementedError, match="use_karras_sigmas"):
        DPMSolverMultistepScheduler.from_pretrained(d)


@pytest.mark.parametrize("n", (1, 2, 20))
def test_set_timesteps_matches_the_float64_schedule(n):
    s = DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
    s.set_timesteps(n)
    ts, sig = R.schedule(n)
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), ts)
    assert s.sigmas.dtype == F32 and np.array_equal(s.sigmas.numpy(), sig.astype(np.float32)) and s.num_inference_steps == n and s.step_index is None
    for i in range(n):
        assert s._coef[i] == R.coefficients_f32(s.sigmas, i), i
    assert s._coef[-1][2:4] == (0.0, -1.0) and [c[0] for c in s._coef] == [R.step_order(i, n) for i in range(n)]
    with pytest.raises(NotImplementedError, match="custom timesteps"):
        s.set_timesteps(n, timesteps=[999, 500])
    with pytest.raises(NotImplementedError, match="custom timesteps"):
        s.set_timesteps(n, sigmas=[1.0, 0.5])
    with pytest.raises(ValueError):
        s.set_timesteps(0)
    s1 = DPMSolverMultistepScheduler(**dict(SANA_SCHEDULER_CONFIG, solver_order=1))
    s1.set_timesteps(n)
    assert {c[0] for c in s1._coef} == {1}


def _cpu_dpm_step(calls=None):
    """ops.dpm_step on CPU tensors through the reference op sequence"""
    def dpm_step(pred_uncond, pred_text, guidance_scale, sample, x0_prev, model_in, *, order, sigma, a, b, rinv=0.0):
        if calls is not None:
            calls.append(dict(guided=pred_text is not None, gs=guidance_scale, order=order, copies=0 if model_in is None else model_in.numel() // sample.numel(),
                              m1=x0_prev.clone()))
        o, x0, mi = R.dpm_step_f32_ops(pred_uncond, pred_text, guidance_scale, sample, x0_prev, order, sigma, a, b, rinv)
        sample.copy_(o)
        x0_prev.copy_(x0)
        if model_in is not None:
            model_in.view(-1, *sample.shape).copy_(mi.expand(model_in.numel() // sample.numel(), *sample.shape))
        return sample
    return dpm_step


def test_step_keeps_diffusers_surface(monkeypatch):
    calls = []
    monkeypatch.setattr(SP.ops, "dpm_step", _cpu_dpm_step(calls))
    s = DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
    x = torch.randn(2, 8, 4, 4, generator=torch.Generator().manual_seed(0))
    with pytest.raises(RuntimeError, match="set_timesteps"):
        s.step(x.to(BF), 999, x)
    s.set_timesteps(3)
    for dt in (BF, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="torch.float32"):
            s.step(x.to(BF), s.timesteps[0], x.to(dt))
    with pytest.raises(ValueError, match="contiguous"):
        s.step(x.to(BF), s.timesteps[0], x.transpose(2, 3))
    assert s.step_index is None or s.step_index == 0
    want, m1 = x.clone(), None
    for i, t in enumerate(s.timesteps):
        v = torch.randn(x.shape, generator=torch.Generator().manual_seed(10 + i)).to(BF)
        want, m1, _ = R.dpm_step_f32_ops(v, None, 1.0, want, m1, *R.coefficients_f32(s.sigmas, i))
        out = s.step(v, t, x)
        assert out.prev_sample is x and s.step_index == i + 1 and torch.equal(x, want) and torch.equal(s._x0_prev, m1)
    assert torch.equal(x, m1)                                                    # the last step returns x0
    assert [c["order"] for c in calls] == [1, 2, 1] and not any(c["guided"] or c["copies"] for c in calls)
    with pytest.raises(IndexError, match="set_timesteps"):
        s.step(v, t, x)
    s.set_timesteps(3)                                                           # the history and the index start again
    assert s.step_index is None and s._x0_prev is None and s.lower_order_nums == 0
    n_calls = len(calls)
    assert s.step(v, s.timesteps[1], x, return_dict=False)[0] is x and s.step_index == 2       # entered in the middle: the timestep's own index ...
    assert len(calls) == n_calls + 1 and calls[-1]["order"] == 1                               # ... and, without a history, first order
    with pytest.raises(RuntimeError, match="shape or device changed"):
        s.step(v[:1], s.timesteps[2], x[:1].clone())


# ---------------------------------------------------------------- the C entry --------------------------------------------------------------
P = 1 << 20                # a fake device address, 4096-byte aligned
DPM = dict(pred_uncond=P, pred_text=2 * P, gs=4.5, sample=3 * P, x0_prev=4 * P, model_in=5 * P, copies=2, order=2, sigma=0.9, a=0.8, b=-0.1, rinv=1.1, n=64)
DPM_ORDER = ("pred_uncond", "pred_text", "gs", "sample", "x0_prev", "model_in", "copies", "order", "sigma", "a", "b", "rinv", "n")


def _call(fn, **kw):
    from unigen_amd import lib
    cdll = lib.load()
    a = dict(DPM)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(cdll, fn)(*[a[n] for n in DPM_ORDER], None)
    return rc, cdll.ug_last_error().decode()


@pytest.mark.parametrize("fn", ("ug_dpm_step", "ug_dpm_step_f32"))
def test_dpm_step_entry_refusals(fn):
    from unigen_amd import lib

    def refused(code, **kw):
        rc, msg = _call(fn, **kw)
        assert rc == code and msg.split(":")[0] == "ug_dpm_step", (fn, kw, rc, msg)
    for n in (4, 12, 63, -8):
        refused(lib.UG_ERR_BAD_ALIGN, n=n)
    for name in ("pred_uncond", "pred_text", "sample", "x0_prev", "model_in"):
        for off in (2, 4, 8):
            refused(lib.UG_ERR_BAD_ALIGN, **{name: DPM[name] + off})
    for order in (0, 3, -1):
        refused(lib.UG_ERR_UNSUPPORTED, order=order)
    refused(lib.UG_ERR_BAD_SHAPE, copies=-1)
    refused(lib.UG_ERR_BAD_SHAPE, copies=1, model_in=None)
    for name in ("pred_uncond", "sample", "x0_prev"):
        refused(lib.UG_ERR_BAD_SHAPE, **{name: None})
    refused(lib.UG_ERR_UNSUPPORTED, n=1 << 40)
    # n == 0 is served without a launch, whatever else is passed
    assert _call(fn, n=0)[0] == lib.UG_OK and _call(fn, n=0, sample=None, order=7)[0] == lib.UG_OK
    assert lib.F32_TWIN_OF["ug_dpm_step"] == "ug_dpm_step_f32"


# ---------------------------------------------------------------- the loop and the pipeline on stand-ins ----------------------------------
class _Transformer:
    """prediction = 0.5 x + the mean of the row's live prompt values + t / 1000, `extra` channels appended when it predicts a variance too"""

    def __init__(self, channels=8, out_channels=8, dtype=BF):
        self.config, self.dtype, self.device, self.calls = dict(in_channels=channels, out_channels=out_channels), dtype, torch.device("cpu"), []

    def __call__(self, hidden_states, encoder_hidden_states, timestep, encoder_attention_mask=None):
        assert hidden_states.dtype == self.dtype and encoder_hidden_states.dtype == self.dtype and timestep.dtype == F32 and timestep.is_contiguous()
        assert timestep.shape == (hidden_states.shape[0],) and encoder_hidden_states.shape[0] == hidden_states.shape[0]
        self.calls.append(dict(x=hidden_states.clone(), enc=encoder_hidden_states, t=timestep.clone(), mask=encoder_attention_mask, x_ptr=hidden_states.data_ptr()))
        m = torch.ones(encoder_hidden_states.shape[:2]) if encoder_attention_mask is None else encoder_attention_mask.float()
        e = (encoder_hidden_states.float().mean(-1) * m).sum(1) / m.sum(1)
        v = 0.5 * hidden_states.float() + e[:, None, None, None] + timestep[:, None, None, None] / 1000
        C, O = self.config["in_channels"], self.config["out_channels"]
        return torch.cat([v, torch.full_like(v, 7.0)], 1).to(self.dtype) if O == 2 * C else v.to(self.dtype)


def _prompt(B, T=6, seed=0, live=None):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(B, T, 16, generator=g).to(BF)
    m = (torch.arange(T)[None] < torch.tensor(live or [T] * B)[:, None]).long()
    return e, m


def _unfused(tr, lat, pos, pmask, neg, nmask, n, gs):
    """the loop as diffusers writes it, on the reference step"""
    ts, sig = R.schedule(n)
    s32 = torch.from_numpy(sig.astype(np.float32))
    cfg = gs > 1
    emb = torch.cat([neg, pos]) if cfg else pos
    mask = torch.cat([nmask, pmask]) if cfg else pmask
    x, m1, B = lat.clone(), None, lat.shape[0]
    for i in range(n):
        xin = (torch.cat([x] * 2) if cfg else x).to(tr.dtype)
        out = tr(xin, emb, torch.tensor(float(ts[i])).expand(xin.shape[0]).contiguous(), mask)
        if tr.config["out_channels"] // 2 == x.shape[1]:
            out = out.chunk(2, dim=1)[0].contiguous()
        x, m1, _ = R.dpm_step_f32_ops(out[:B], out[B:] if cfg else None, gs, x, m1, *R.coefficients_f32(s32, i))
    return x


@pytest.mark.parametrize("gs", (4.5, 1.0))
@pytest.mark.parametrize("learned_sigma", (False, True))
def test_loop_rows_masks_and_learned_sigma(monkeypatch, gs, learned_sigma):
    calls = []
    monkeypatch.setattr(SP.ops, "dpm_step", _cpu_dpm_step(calls))
    tr = _Transformer(8, 16 if learned_sigma else 8)
    sched = DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
    lat = torch.randn(2, 8, 4, 4, generator=torch.Generator().manual_seed(1))
    (pos, pmask), (neg, nmask) = _prompt(2, seed=1, live=[6, 3]), _prompt(2, seed=2, live=[1, 6])
    out = sana_denoise_loop(tr, sched, latents=lat.clone(), prompt_embeds=pos, prompt_attention_mask=pmask, negative_prompt_embeds=neg,
                            negative_prompt_attention_mask=nmask, num_inference_steps=3, guidance_scale=gs)
    cfg = gs > 1
    rows = 4 if cfg else 2
    assert len(tr.calls) == 3 and len({c["x_ptr"] for c in tr.calls}) == 1                      # one forward per step on ONE standing input buffer
    ts, _ = R.schedule(3)
    for i, c in enumerate(tr.calls):
        assert tuple(c["x"].shape) == (rows, 8, 4, 4) and torch.equal(c["t"], torch.full((rows,), float(ts[i])))
        assert torch.equal(c["enc"], torch.cat([neg, pos]) if cfg else pos) and torch.equal(c["mask"], torch.cat([nmask, pmask]) if cfg else pmask)
        assert c["mask"] is tr.calls[0]["mask"] and c["enc"] is tr.calls[0]["enc"]               # the same objects every step: nothing is rebuilt
        if cfg:
            assert torch.equal(c["x"][:2], c["x"][2:])
    assert torch.equal(tr.calls[0]["x"][:2], lat.to(BF))
    assert [(c["guided"], c["order"], c["copies"]) for c in calls] == [(cfg, o, rows // 2) for o in (1, 2, 1)]
    ref = _unfused(_Transformer(8, 16 if learned_sigma else 8), lat, pos, pmask, neg, nmask, 3, gs)
    assert out.dtype == F32 and torch.equal(out, ref)
    assert torch.equal(sched._x0_prev, out)                                                      # the last step wrote x0


def test_loop_callback_and_refusals(monkeypatch):
    monkeypatch.setattr(SP.ops, "dpm_step", _cpu_dpm_step())
    tr, sched = _Transformer(), DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
    lat = torch.randn(1, 8, 4, 4, generator=torch.Generator().manual_seed(1))
    pos, pmask = _prompt(1, seed=1)
    seen = []

    def cb(pipe, i, t, kw):
        seen.append((pipe, i, int(t), sorted(kw)))
        return {"latents": kw["latents"] * 0.5} if i == 0 else {}
    out = sana_denoise_loop(tr, sched, latents=lat.clone(), prompt_embeds=pos, prompt_attention_mask=pmask, num_inference_steps=3, guidance_scale=1.0,
                            callback_on_step_end=cb, callback_on_step_end_tensor_inputs=("latents", "noise_pred"), pipeline="me")
    assert seen == [("me", i, t, ["latents", "noise_pred"]) for i, t in enumerate(R.schedule(3)[0].tolist())]
    first = R.dpm_step_f32_ops(_Transformer()(lat.to(BF), pos, torch.tensor([999.0]), pmask), None, 1.0, lat, None, *R.coefficients_f32(sched.sigmas, 0))[0]
    assert torch.equal(tr.calls[1]["x"], (first * 0.5).to(BF)) and torch.isfinite(out).all()      # the replaced latents reached the next forward
    with pytest.raises(TypeError, match="float32"):
        sana_denoise_loop(tr, sched, latents=lat.to(BF), prompt_embeds=pos, num_inference_steps=2, guidance_scale=1.0)
    with pytest.raises(ValueError, match="negative_prompt_embeds"):
        sana_denoise_loop(tr, sched, latents=lat.clone(), prompt_embeds=pos, num_inference_steps=2, guidance_scale=4.5)
    with pytest.raises(ValueError, match="negative_prompt_attention_mask"):
        sana_denoise_loop(tr, sched, latents=lat.clone(), prompt_embeds=pos, prompt_attention_mask=pmask, negative_prompt_embeds=pos, num_inference_steps=2)
    with pytest.raises(ValueError, match="prompt rows"):
        sana_denoise_loop(tr, sched, latents=lat.clone(), prompt_embeds=_prompt(2)[0], num_inference_steps=2, guidance_scale=1.0)
    with pytest.raises(ValueError, match="channels"):
        sana_denoise_loop(_Transformer(8, 12), sched, latents=lat.clone(), prompt_embeds=pos, num_inference_steps=2, guidance_scale=1.0)


def _pipe(**kw):
    vae = SimpleNamespace(spatial_factor=4, config=SimpleNamespace(scaling_factor=0.5), dtype=BF, device=torch.device("cpu"))
    return SanaPipeline(None, None, kw.pop("vae", vae), _Transformer(**kw), DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG))


def test_pipeline_refusals(tmp_path):
    pipe = _pipe()
    pos, pmask = _prompt(1)
    common = dict(prompt_embeds=pos, prompt_attention_mask=pmask, guidance_scale=1.0, height=16, width=16, output_type="latent")
    for kw, names in ((dict(use_resolution_binning=True), "use_resolution_binning"), (dict(clean_caption=True), "clean_caption"),
                      (dict(timesteps=[999, 1]), "custom timesteps"), (dict(sigmas=[1.0, 0.5]), "custom timesteps"),
                      (dict(attention_kwargs={"scale": 0.5}), "attention_kwargs")):
        with pytest.raises(NotImplementedError, match=names):
            pipe(**dict(common, **kw))
    with pytest.raises(ValueError, match="exactly one"):
        pipe(**dict(common, prompt_embeds=None))
    with pytest.raises(ValueError, match="exactly one"):
        pipe(**dict(common, prompt="a cat"))
    with pytest.raises(ValueError, match="multiples of 4"):
        pipe(**dict(common, height=18))
    with pytest.raises(ValueError, match="text encoder"):
        pipe(**dict(common, prompt_embeds=None, prompt="a cat"))
    with pytest.raises(ValueError, match="text encoder"):                        # guidance with the default negative prompt "" and nothing to encode it
        pipe(**dict(common, guidance_scale=4.5))
    with pytest.raises(ValueError, match="latents"):
        pipe(**dict(common, latents=torch.zeros(1, 8, 3, 4)))
    with pytest.raises(ValueError, match="needs a VAE"):
        _pipe(vae=None)(**dict(common, output_type="pt", height=32, width=32))
    for bad in (tmp_path / "nowhere", "org/some-model"):
        with pytest.raises(OSError, match="not a local directory"):
            SanaPipeline.from_pretrained(bad)
    with pytest.raises(TypeError, match="unknown arguments"):
        SanaPipeline.from_pretrained(tmp_path, revision="main")
    assert pipe.to("cpu", BF) is pipe
    with pytest.raises(NotImplementedError, match="has no to"):
        SanaPipeline(None, None, None, SimpleNamespace(device=torch.device("cpu"), dtype=BF, config=dict(in_channels=8))).to(dtype=F32)


def test_pipeline_from_pretrained_reads_every_component(tmp_path):
    """the tiny components of the GPU tests, built on the host, written in diffusers' layout and read back through each component's own from_pretrained"""
    from safetensors.torch import save_file
    from tests import dcae_ref as DR
    from tests import gemma_ref as GR
    from tests import sana_ref as SR
    from unigen_amd.dcae import AutoencoderDC
    from unigen_amd.gemma import Gemma2Model
    from unigen_amd.sana import SanaTransformer2DModel
    tcfg = dict(SR.TINY["a"], caption_channels=128)
    tr = SanaTransformer2DModel(tcfg, dtype=BF).init_synthetic_(3)
    gcfg, std, seed = GR.TINY["a"]
    te = Gemma2Model.from_config(gcfg, dtype=BF)
    te.load_state_dict(GR.tiny_state(gcfg, std, seed))
    vae = AutoencoderDC(DR.TINY["a"], dtype=BF)
    vae.load_state_dict(DR.tiny_state_dict("a"))
    for name, m, cfg, fn in (("transformer", tr, tcfg, "diffusion_pytorch_model.safetensors"), ("text_encoder", te, gcfg, "model.safetensors"),
                             ("vae", vae, DR.TINY["a"], "diffusion_pytorch_model.safetensors")):
        (tmp_path / name).mkdir()
        (tmp_path / name / "config.json").write_text(json.dumps(dict(cfg, _class_name=type(m).__name__)))
        save_file({k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}, str(tmp_path / name / fn))
    with pytest.raises(OSError):                                                 # no scheduler/ yet
        SanaPipeline.from_pretrained(tmp_path)
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(SANA_SCHEDULER_CONFIG, flow_shift=2.5, _class_name="DPMSolverMultistepScheduler")))
    pipe = SanaPipeline.from_pretrained(tmp_path)
    assert pipe.tokenizer is None and pipe.vae_scale_factor == 4 and pipe.scheduler.config.flow_shift == 2.5 and pipe.image_processor.vae_scale_factor == 4
    for a, b in ((tr, pipe.transformer), (te, pipe.text_encoder), (vae, pipe.vae)):
        sa, sb = a.state_dict(), b.state_dict()
        assert type(a) is type(b) and set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    given = DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)
    assert SanaPipeline.from_pretrained(tmp_path, scheduler=given, vae=vae).scheduler is given      # a component passed as a keyword is taken as it is


def test_pipeline_latent_output_and_image_order(monkeypatch):
    monkeypatch.setattr(SP.ops, "dpm_step", _cpu_dpm_step())
    pipe = _pipe()
    (pos, pmask), (neg, nmask) = _prompt(2, seed=3, live=[6, 2]), _prompt(2, seed=4, live=[3, 6])
    kw = dict(prompt_embeds=pos, prompt_attention_mask=pmask, negative_prompt_embeds=neg, negative_prompt_attention_mask=nmask, num_inference_steps=2,
              height=16, width=24, output_type="latent")
    out = pipe(generator=torch.Generator().manual_seed(5), **kw)
    assert isinstance(out, SanaPipelineOutput) and out.images.dtype == F32 and tuple(out.images.shape) == (2, 8, 4, 6)
    tup = pipe(generator=torch.Generator().manual_seed(5), return_dict=False, **kw)
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], out.images)
    lat = torch.randn(2, 8, 4, 6, generator=torch.Generator().manual_seed(5))
    assert torch.equal(pipe(latents=lat, **kw).images, out.images) and torch.equal(lat, torch.randn(2, 8, 4, 6, generator=torch.Generator().manual_seed(5)))
    ref = _unfused(_Transformer(), lat, pos, pmask, neg, nmask, 2, 4.5)
    assert torch.equal(out.images, ref)
    # two images per prompt: each prompt's images are adjacent, the negative rows come first in the model's batch
    pipe.transformer.calls.clear()
    lat4 = torch.randn(4, 8, 4, 6, generator=torch.Generator().manual_seed(6))
    out4 = pipe(latents=lat4, num_images_per_prompt=2, **kw).images
    c = pipe.transformer.calls[0]
    assert torch.equal(c["enc"], torch.cat([neg.repeat_interleave(2, 0), pos.repeat_interleave(2, 0)]))
    assert torch.equal(c["mask"], torch.cat([nmask.repeat_interleave(2, 0), pmask.repeat_interleave(2, 0)]))
    for j in range(4):
        one = _unfused(_Transformer(), lat4[j:j + 1], pos[j // 2:j // 2 + 1], pmask[j // 2:j // 2 + 1], neg[j // 2:j // 2 + 1], nmask[j // 2:j // 2 + 1], 2, 4.5)
        assert torch.equal(out4[j:j + 1], one), j
