"""ug_dpm_step, sana_denoise_loop and SanaPipeline on the GPU.

  - the kernel, both twins, against tests/sana_pipeline_ref.dpm_step_f32_ops BIT FOR BIT (sample, x0_prev, model_in): one chunk, one block minus and plus
    a chunk, one chunk past the launcher's grid cap (2048 blocks x 256 threads x 8 elements: the stride loop turns), both orders, no guidance and scales
    1.0 and 4.5, 0 / 1 / 2 copies, the last step, inputs with +-0, bf16 subnormals and values near the bf16 maximum. A NaN (inf - inf at the far
    end of the range) must be a NaN on both sides; its payload is not compared;
  - the loop against an unfused loop (below: the same device transformer, guidance, conversion and update as torch fp32 ops in the kernel's
    order) bit for bit, with and without guidance, with a callback that replaces the latents, and twice for identical bytes;
  - the whole pipeline on the tiny Sana, Gemma and DC-AE configurations of the other GPU tests; through the fp32 twins against a float64 loop
    (tests/sana_ref.SanaModelRef + the float64 scheduler) under the tolerance of docs/PARITY_TOLERANCES.md, "Sana pipeline"."""
import numpy as np
import pytest
import torch

from tests import dcae_ref as DR
from tests import gemma_ref as GR
from tests import sana_pipeline_ref as R
from tests import sana_ref as SR

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GRID_CAP = 2048                                          # ug_grid1d(n / 8, 256, 2048) in csrc/sched.hip
SIZES = [8, 8 * 256 - 8, 8 * 256 + 8, GRID_CAP * 256 * 8 + 8]
PAD = 64                                                 # sentinel elements behind every output
# (order, sigma, a, b, rinv): a middle step of the 20-step schedule, and its last step
MIDDLE = lambda order: (order,) + R.coefficients_f32(torch.from_numpy(R.schedule(20)[1].astype(np.float32)), 7)[1:]
LAST = R.coefficients_f32(torch.from_numpy(R.schedule(20)[1].astype(np.float32)), 19)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def assert_same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    same = (_bits(got) == _bits(want)) | (torch.isnan(got) & torch.isnan(want))
    assert bool(same.all()), (what, int((~same).sum()), got[~same][:4], want[~same][:4])


def _padded(t, gpu, extra=0):
    """a device buffer holding t, then `extra` elements of room, then PAD sentinel elements"""
    buf = torch.full((t.numel() + extra + PAD,), 77.0, dtype=t.dtype, device=gpu)
    buf[:t.numel()] = t.to(gpu).flatten()
    return buf


def _run_kernel(gpu, dt, n, order, gs, copies, coef, seed):
    """one launch on seeded inputs against the CPU op sequence; -> nothing, asserts"""
    from unigen_amd import lib, ops
    u, t = R.special_values(n, dt, seed), R.special_values(n, dt, seed + 1)
    x, m1 = R.special_values(n, F32, seed + 2), R.special_values(n, F32, seed + 3)
    if gs is None:
        t = None
    _, sigma, a, b, rinv = coef
    want_o, want_x0, want_mi = R.dpm_step_f32_ops(u, t, gs if gs is not None else 1.0, x, m1, order, sigma, a, b, rinv)
    ud, td = u.to(gpu), None if t is None else t.to(gpu)
    xb, mb = _padded(x, gpu), _padded(m1, gpu)
    ib = torch.full((copies * n + PAD,), 77.0, dtype=dt, device=gpu)
    fn = getattr(lib.load(), "ug_dpm_step" if dt == BF else "ug_dpm_step_f32")
    rc = fn(ud.data_ptr(), None if td is None else td.data_ptr(), gs if gs is not None else 1.0, xb.data_ptr(), mb.data_ptr(), ib.data_ptr() if copies else None,
            copies, order, sigma, a, b, rinv, n, ops._stream())
    assert rc == 0, lib.load().ug_last_error()
    torch.cuda.synchronize()
    tag = f"n={n} order={order} gs={gs} copies={copies} {dt}"
    assert_same_bits(xb[:n], want_o, "sample " + tag)
    assert_same_bits(mb[:n], want_x0, "x0_prev " + tag)
    for k in range(copies):
        assert_same_bits(ib[k * n:(k + 1) * n], want_mi, f"model_in[{k}] " + tag)
    for buf, used in ((xb, n), (mb, n), (ib, copies * n)):
        assert bool((buf[used:] == 77.0).all()), "wrote past the end: " + tag
    assert torch.equal(ud.cpu(), u) and (t is None or torch.equal(td.cpu(), t)), "the predictions were written: " + tag


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", (BF, F32), ids=("bf16", "f32"))
def test_dpm_step_kernel_bit_for_bit(gpu, dt, n):
    big = n > 8 * 256 * 8
    combos = [(o, gs, c) for o in (1, 2) for gs in (None, 1.0, 4.5) for c in (0, 1, 2)]
    if big:                                              # 4 M elements: the stride loop is the subject; every axis still takes each of its values once
        combos = [(1, None, 0), (2, 4.5, 2), (1, 1.0, 1), (2, None, 1)]
    for j, (order, gs, copies) in enumerate(combos):
        _run_kernel(gpu, dt, n, order, gs, copies, MIDDLE(order), 100 + j)
    for j, (gs, copies) in enumerate([(4.5, 2)] if big else [(None, 0), (4.5, 2), (1.0, 1)]):
        _run_kernel(gpu, dt, n, 1, gs, copies, LAST, 200 + j)


@pytest.mark.parametrize("dt", (BF, F32), ids=("bf16", "f32"))
def test_step_ends(gpu, dt):
    """three steps through ops.dpm_step on ordinary values: after the first step x0_prev holds what the second step's reference reads, and the last step
    (a = 0, b = -1) writes exactly x0"""
    from unigen_amd import ops
    n_steps, shape = 3, (2, 8, 4, 6)
    s32 = torch.from_numpy(R.schedule(n_steps)[1].astype(np.float32))
    g = torch.Generator().manual_seed(9)
    x = torch.randn(shape, generator=g)
    xd, m1d, mi = x.to(gpu), torch.empty(shape, dtype=F32, device=gpu), torch.empty((2,) + shape, dtype=dt, device=gpu)
    want, m1 = x.clone(), None
    for i in range(n_steps):
        u, t = torch.randn(shape, generator=g).to(dt), torch.randn(shape, generator=g).to(dt)
        order, sigma, a, b, rinv = R.coefficients_f32(s32, i)
        want, m1, wmi = R.dpm_step_f32_ops(u, t, 4.5, want, m1, order, sigma, a, b, rinv)
        out = ops.dpm_step(u.to(gpu), t.to(gpu), 4.5, xd, m1d, mi, order=order, sigma=sigma, a=a, b=b, rinv=rinv)
        assert out is xd
        assert_same_bits(xd, want, f"sample after step {i}")
        assert_same_bits(m1d, m1, f"x0_prev after step {i}")
        assert_same_bits(mi[0], wmi, f"model_in after step {i}")
        assert torch.equal(mi[0], mi[1])
    assert (a, b) == (0.0, -1.0) and torch.equal(xd, m1d) and torch.equal(mi[0], m1d.to(dt))


# ---------------------------------------------------------------- the loop ---------------------------------------------------------------
_MODELS = {}


def sana_model(gpu, dtype, caption_channels=64):
    from unigen_amd.sana import SanaTransformer2DModel
    key = ("sana", dtype, caption_channels)
    if key not in _MODELS:
        if caption_channels == 64:                       # configuration "a" with the fixture's weights (exact in bf16)
            m = SanaTransformer2DModel(SR.TINY["a"], device=gpu, dtype=dtype)
            m.load_state_dict(SR.tiny_state_dict("a"))
        else:                                            # as tests/test_gemma_gpu.py: the tiny Gemma's hidden width
            m = SanaTransformer2DModel(dict(SR.TINY["a"], caption_channels=caption_channels), device=gpu, dtype=dtype).init_synthetic_(3)
        _MODELS[key] = m
    return _MODELS[key]


def dcae_model(gpu, dtype):
    from unigen_amd.dcae import AutoencoderDC
    if ("dcae", dtype) not in _MODELS:
        m = AutoencoderDC(DR.TINY["a"], device=gpu, dtype=dtype)
        m.load_state_dict(DR.tiny_state_dict("a"))
        _MODELS[("dcae", dtype)] = m
    return _MODELS[("dcae", dtype)]


def gemma_model(gpu, dtype):
    from unigen_amd.gemma import Gemma2Model
    if ("gemma", dtype) not in _MODELS:
        cfg, std, seed = GR.TINY["a"]
        m = Gemma2Model.from_config(cfg, device=gpu, dtype=dtype)
        m.load_state_dict(GR.tiny_state(cfg, std, seed))
        _MODELS[("gemma", dtype)] = m
    return _MODELS[("gemma", dtype)]


def scheduler():
    from unigen_amd.sana_pipeline import DPMSolverMultistepScheduler, SANA_SCHEDULER_CONFIG
    return DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG)


def loop_inputs(B=2, H=4, W=6, T=12, C=8, width=64, dtype=BF):
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(B, C, H, W, generator=g)
    pos, neg = torch.randn(B, T, width, generator=g).to(dtype), torch.randn(B, T, width, generator=g).to(dtype)
    pmask = (torch.arange(T)[None] < torch.tensor([T, 5][:B])[:, None]).long()
    nmask = (torch.arange(T)[None] < torch.tensor([3, T][:B])[:, None]).long()
    return lat, pos, pmask, neg, nmask


def unfused_loop(tr, lat, pos, pmask, neg, nmask, n, gs, replace_at=None):
    """The loop as diffusers writes it, on the device: the same transformer; guidance, conversion and update as single torch fp32 tensor ops in the
    kernel's order (every scalar a 0-dim fp32 tensor, as the scheduler holds them)."""
    dev = tr.device
    ts, sig = R.schedule(n)
    s32 = torch.from_numpy(sig.astype(np.float32))
    c = lambda v: torch.tensor(v, dtype=F32, device=dev)
    cfg = gs > 1
    emb = (torch.cat([neg, pos]) if cfg else pos).to(dev)
    mask = (torch.cat([nmask, pmask]) if cfg else pmask).to(dev)
    x, m1, B = lat.to(dev).clone(), None, lat.shape[0]
    for i in range(n):
        xin = (torch.cat([x] * 2) if cfg else x).to(tr.dtype)
        out = tr(xin, encoder_hidden_states=emb, timestep=torch.full((xin.shape[0],), float(ts[i]), dtype=F32, device=dev), encoder_attention_mask=mask)
        order, sigma, a, b, rinv = R.coefficients_f32(s32, i)
        p = out[:B].float()
        if cfg:
            d = out[B:].float() - p
            d = c(gs) * d
            p = p + d
        sp = c(sigma) * p
        x0 = x - sp
        ax = c(a) * x
        bx = c(b) * x0
        o = ax - bx
        if order == 2:
            d = x0 - m1
            d = c(rinv) * d
            hb = c(0.5) * c(b)
            d = hb * d
            o = o - d
        x, m1 = o, x0
        if replace_at == i:
            x = x * 0.5
    return x


@pytest.mark.parametrize("gs", (4.5, 1.0), ids=("guided", "unguided"))
@pytest.mark.parametrize("dt", (BF, F32), ids=("bf16", "f32"))
def test_loop_matches_the_unfused_loop_bit_for_bit(gpu, dt, gs):
    from unigen_amd.sana_pipeline import sana_denoise_loop
    tr = sana_model(gpu, dt)
    lat, pos, pmask, neg, nmask = loop_inputs(dtype=dt)
    kw = dict(prompt_embeds=pos.to(gpu), prompt_attention_mask=pmask.to(gpu), negative_prompt_embeds=neg.to(gpu), negative_prompt_attention_mask=nmask.to(gpu),
              num_inference_steps=3, guidance_scale=gs)
    sched = scheduler()
    got = sana_denoise_loop(tr, sched, latents=lat.to(gpu), **kw)
    want = unfused_loop(tr, lat, pos, pmask, neg, nmask, 3, gs)
    assert got.dtype == F32 and bool(torch.isfinite(got).all()) and not torch.equal(got.cpu(), lat)
    assert_same_bits(got, want, "final latents")
    assert torch.equal(sched._x0_prev, got) and sched.step_index == 3                       # the last step returned x0
    again = sana_denoise_loop(tr, sched, latents=lat.to(gpu), **kw)                          # the same scheduler object: set_timesteps starts it again
    assert_same_bits(again, got, "a second identical run")
    # a callback that replaces the latents after the second step
    seen = []

    def cb(pipe, i, t, tensors):
        seen.append((i, int(t)))
        return {"latents": tensors["latents"] * 0.5} if i == 1 else {}
    got_cb = sana_denoise_loop(tr, sched, latents=lat.to(gpu), callback_on_step_end=cb, **kw)
    assert seen == list(enumerate(R.schedule(3)[0].tolist()))
    assert_same_bits(got_cb, unfused_loop(tr, lat, pos, pmask, neg, nmask, 3, gs, replace_at=1), "with a callback replacing the latents")
    assert not torch.equal(got_cb, got)


def test_loop_keeps_the_first_half_of_a_learned_sigma_prediction(gpu):
    """out_channels = 2 x in_channels: the first half of the channels is the flow, through one contiguous copy"""
    from unigen_amd.sana import SanaTransformer2DModel
    from unigen_amd.sana_pipeline import sana_denoise_loop
    tr = SanaTransformer2DModel(dict(SR.TINY["a"], out_channels=16), device=gpu, dtype=BF).init_synthetic_(5)
    lat, pos, pmask, neg, nmask = loop_inputs()
    got = sana_denoise_loop(tr, scheduler(), latents=lat.to(gpu), prompt_embeds=pos.to(gpu), prompt_attention_mask=pmask.to(gpu), negative_prompt_embeds=neg.to(gpu),
                            negative_prompt_attention_mask=nmask.to(gpu), num_inference_steps=3, guidance_scale=4.5)

    class FirstHalf:
        dtype, device, config = tr.dtype, tr.device, tr.config

        def __call__(self, *a, **kw):
            return tr(*a, **kw).chunk(2, dim=1)[0].contiguous()
    assert_same_bits(got, unfused_loop(FirstHalf(), lat, pos, pmask, neg, nmask, 3, 4.5), "learned sigma")


# ---------------------------------------------------------------- the whole pipeline --------------------------------------------------
def tiny_pipeline(gpu):
    from unigen_amd.sana_pipeline import SanaPipeline
    return SanaPipeline(None, gemma_model(gpu, BF), dcae_model(gpu, BF), sana_model(gpu, BF, 128), scheduler())


def test_pipeline_output_types_latents_and_image_order(gpu):
    from unigen_amd.sana_pipeline import SanaPipelineOutput
    pipe = tiny_pipeline(gpu)
    ids, mask = GR.tiny_inputs()
    neg = (ids.flip(1).contiguous(), mask.flip(0).contiguous())
    kw = dict(prompt=(ids, mask), negative_prompt=neg, num_inference_steps=2, height=64, width=64, max_sequence_length=16)
    shape = (2, 8, 16, 16)
    lat = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    out = pipe(generator=torch.Generator().manual_seed(5), output_type="latent", **kw)
    assert isinstance(out, SanaPipelineOutput) and out.images.dtype == F32 and tuple(out.images.shape) == shape and out.images.is_cuda
    assert bool(torch.isfinite(out.images).all())
    given = pipe(latents=lat, output_type="latent", return_dict=False, **kw)
    assert isinstance(given, tuple) and torch.equal(given[0], out.images)                    # supplied latents are honoured (and equal the generator's draw)
    assert not torch.equal(pipe(latents=lat.flip(0).contiguous(), output_type="latent", **kw).images, out.images)
    pt = pipe(latents=lat, output_type="pt", **kw).images
    assert pt.dtype == BF and tuple(pt.shape) == (2, 3, 64, 64) and float(pt.min()) >= 0 and float(pt.max()) <= 1
    pil = pipe(latents=lat, output_type="pil", **kw).images
    assert isinstance(pil, list) and len(pil) == 2 and all(im.size == (64, 64) and im.mode == "RGB" for im in pil)
    u8 = (pt.float() * 255).round().clamp(0, 255).permute(0, 2, 3, 1).cpu().numpy()
    assert max(np.abs(np.asarray(im).astype(np.float64) - a).max() for im, a in zip(pil, u8)) <= 1      # the same image, rounded once more
    # two images per prompt: rows 0, 1 belong to prompt 0 and rows 2, 3 to prompt 1 - with the same noise, a prompt's two images agree
    lat4 = lat.repeat_interleave(2, 0)
    four = pipe(latents=lat4, num_images_per_prompt=2, output_type="latent", **kw).images
    rel = lambda a, b: float((a - b).norm() / b.norm())
    same, other = max(rel(four[0], four[1]), rel(four[2], four[3])), min(rel(four[0], four[2]), rel(four[1], four[3]))
    print(f"num_images_per_prompt = 2: a prompt's two images differ by {same:.3e}, the two prompts' images by {other:.3e}")
    assert tuple(four.shape) == (4, 8, 16, 16) and same <= 0.1 * other and other > 0
    assert rel(four[0], out.images[0]) <= 0.1 * other and rel(four[2], out.images[1]) <= 0.1 * other


def test_from_pretrained_of_a_local_directory_returns_images(gpu, tmp_path):
    """the tiny components written out in diffusers' layout and read back: the same images as the pipeline built from the objects, from prompt_embeds"""
    import json
    from safetensors.torch import save_file
    from unigen_amd.sana_pipeline import SANA_SCHEDULER_CONFIG, SanaPipeline
    built = tiny_pipeline(gpu)
    parts = {"transformer": (built.transformer, dict(SR.TINY["a"], caption_channels=128), "diffusion_pytorch_model.safetensors"),
             "text_encoder": (built.text_encoder, GR.TINY["a"][0], "model.safetensors"), "vae": (built.vae, DR.TINY["a"], "diffusion_pytorch_model.safetensors")}
    for name, (m, cfg, fn) in parts.items():
        (tmp_path / name).mkdir()
        (tmp_path / name / "config.json").write_text(json.dumps(dict(cfg, _class_name=type(m).__name__)))
        save_file({k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}, str(tmp_path / name / fn))
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(SANA_SCHEDULER_CONFIG, _class_name="DPMSolverMultistepScheduler")))
    pipe = SanaPipeline.from_pretrained(tmp_path, device=gpu)
    assert pipe.tokenizer is None and pipe.vae_scale_factor == 4 and pipe.device.type == "cuda" and pipe.to(gpu, BF) is pipe
    _, pos, pmask, neg, nmask = loop_inputs(T=16, width=128)
    kw = dict(prompt_embeds=pos.to(gpu), prompt_attention_mask=pmask.to(gpu), negative_prompt_embeds=neg.to(gpu), negative_prompt_attention_mask=nmask.to(gpu),
              num_inference_steps=2, height=64, width=64, generator=torch.Generator().manual_seed(11))
    images = pipe(output_type="pt", **kw).images
    kw["generator"] = torch.Generator().manual_seed(11)
    assert tuple(images.shape) == (2, 3, 64, 64) and bool(torch.isfinite(images).all()) and torch.equal(images, built(output_type="pt", **kw).images)


FP64_TOLERANCE = 2.9e-6   # measured on an MI355X: 1.467e-06; a factor 2 for box-to-box variation (docs/PARITY_TOLERANCES.md, "Sana pipeline")


def test_fp32_pipeline_against_the_float64_loop(gpu):
    """The fp32 components (ug_dpm_step_f32 and the fp32 twins of the transformer's kernels) against a float64 loop: tests/sana_ref.SanaModelRef in
    float64 and the float64 scheduler of tests/sana_pipeline_ref.py, 64 x 64 pixels (16 x 16 latents), 3 steps, guidance 4.5, B = 2 with masked prompts.
    rel_l2 of the final latents; the bound is twice the value measured on an MI355X (docs/PARITY_TOLERANCES.md, "Sana pipeline")."""
    from unigen_amd.sana_pipeline import SanaPipeline
    pipe = SanaPipeline(None, None, dcae_model(gpu, F32), sana_model(gpu, F32), scheduler())
    lat, pos, pmask, neg, nmask = loop_inputs(H=16, W=16, dtype=F32)
    out = pipe(prompt_embeds=pos.to(gpu), prompt_attention_mask=pmask.to(gpu), negative_prompt_embeds=neg.to(gpu), negative_prompt_attention_mask=nmask.to(gpu),
               latents=lat, num_inference_steps=3, guidance_scale=4.5, height=64, width=64, output_type="latent").images
    ref = SR.build_ref("a", SR.tiny_state_dict("a"), F64)

    def model(x, t, negative):
        with torch.no_grad():
            return ref(x, (neg if negative else pos).to(F64), torch.full((x.shape[0],), t, dtype=F64), nmask if negative else pmask)
    want = R.dpm_loop_f64(model, lat, 3, guidance_scale=4.5)
    err = float((out.cpu().double() - want).norm() / want.norm())
    print(f"fp32 Sana pipeline vs the float64 loop: rel_l2 {err:.3e} (bound {FP64_TOLERANCE})")
    assert out.dtype == F32 and err <= FP64_TOLERANCE
