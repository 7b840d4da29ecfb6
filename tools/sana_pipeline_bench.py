"""SanaPipeline on the GPU at the published geometry - Sana-1.6B transformer, gemma-2-2b text encoder, dc-ae-f32c32 autoencoder, synthetic weights - at
1024 x 1024, B = 1, 20 steps, guidance 4.5: the record behind profiles/sana_pipeline_bench.log.

    python tools/sana_pipeline_bench.py [--out profiles/sana_pipeline_bench.log] [--rounds 7] [--steps 20]

Stages: the prompt encode (prompt and negative prompt, 300 tokens each), the denoise loop, the decode (vae.decode + postprocess to "pt") and the whole
call, each a host clock around work that ends in a device synchronise, after two warm calls; median / min / max over the rounds.
Fused against unfused, interleaved in this one process, round by round (fused, torch, fused, torch, ...):
  - the loop with ug_dpm_step against the same loop with the step as torch fp32 tensor ops and `torch.cat([latents] * 2).to(bf16)` (the results are
    compared bit for bit first);
  - the step alone on the 1024^2 latent ([1, 32, 32, 32], predictions [2, 32, 32, 32] bf16): 200 launches between one pair of device events, against
    200 runs of the torch-op sequence."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigen_amd import lib as L  # noqa: E402
from unigen_amd import ops  # noqa: E402
from unigen_amd.dcae import DCAE_F32C32_SANA, AutoencoderDC  # noqa: E402
from unigen_amd.gemma import Gemma2Model  # noqa: E402
from unigen_amd.sana import SanaTransformer2DModel  # noqa: E402
from unigen_amd.sana_pipeline import SANA_SCHEDULER_CONFIG, DPMSolverMultistepScheduler, SanaPipeline, sana_denoise_loop  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SANA_1600M = dict(in_channels=32, out_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                  cross_attention_head_dim=112, cross_attention_dim=2240, caption_channels=2304, mlp_ratio=2.5, attention_bias=False, sample_size=32,
                  patch_size=1, norm_eps=1e-6, interpolation_scale=None)
GEMMA_2_2B = dict(vocab_size=256000, hidden_size=2304, num_hidden_layers=26, num_attention_heads=8, num_key_value_heads=4, head_dim=256, intermediate_size=9216,
                  rms_norm_eps=1e-6, query_pre_attn_scalar=256, attn_logit_softcapping=50.0, sliding_window=4096, hidden_activation="gelu_pytorch_tanh")


def torch_step(pu, pt, gs, x, m1, coef):
    """the step as torch evaluates it: one fp32 tensor op per line of ug_dpm_step's definition -> (sample, x0)"""
    order, sigma, a, b, rinv = coef
    p = pu.float()
    if pt is not None:
        p = p + gs * (pt.float() - p)
    x0 = x - sigma * p
    o = a * x - b * x0
    if order == 2:
        o = o - (0.5 * b) * (rinv * (x0 - m1))
    return o, x0


@torch.no_grad()
def torch_loop(tr, sched, latents, embeds, mask, steps, gs):
    """sana_denoise_loop with the step unfused; embeds / mask already cat([negative, positive])"""
    sched.set_timesteps(steps, device=latents.device)
    x, m1, B = latents, None, latents.shape[0]
    t_rows = sched.timesteps.to(F32)[:, None].expand(steps, 2 * B).contiguous()
    for i in range(steps):
        xin = torch.cat([x] * 2).to(tr.dtype)
        out = tr(xin, encoder_hidden_states=embeds, timestep=t_rows[i], encoder_attention_mask=mask)
        x, m1 = torch_step(out[:B], out[B:], gs, x, m1, sched._coef[i])
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sana_pipeline_bench.log"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=20, help="transformer layers (20 = Sana-1.6B); the text encoder keeps its 26")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sana_pipeline_bench.py measures on the GPU: no GPU visible")
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds")
    dev = torch.device("cuda:0")
    L.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(0)
    tr = SanaTransformer2DModel(dict(SANA_1600M, num_layers=a.layers), device=dev, dtype=BF).init_synthetic_(0)
    enc = Gemma2Model(GEMMA_2_2B, device=dev, dtype=BF)
    for t in enc.state_dict().values():                  # on the device: the embedding alone is 590 M values
        t.copy_(torch.randn(t.shape, generator=g, device=dev) * ((0.7 / t.shape[1] ** 0.5) if t.dim() == 2 else 0.1))
    vae = AutoencoderDC(DCAE_F32C32_SANA, device=dev).init_synthetic_(0)
    pipe = SanaPipeline(None, enc, vae, tr, DPMSolverMultistepScheduler(**SANA_SCHEDULER_CONFIG))
    gs, steps, size = 4.5, a.steps, 1024
    ids = torch.randint(0, 256000, (1, 300), generator=g, device=dev, dtype=torch.int32)
    mask = torch.ones(1, 300, dtype=torch.int64, device=dev)
    mask[0, 211:] = 0
    nids, nmask = torch.randint(0, 256000, (1, 300), generator=g, device=dev, dtype=torch.int32), torch.zeros(1, 300, dtype=torch.int64, device=dev)
    nmask[0, :2] = 1                                     # an empty negative prompt: the start token and little else
    lat = torch.randn(1, 32, size // 32, size // 32, generator=g, device=dev, dtype=F32)
    say(f"# tools/sana_pipeline_bench.py on {torch.cuda.get_device_name(0)}; Sana-1.6B ({a.layers} layers) + gemma-2-2b + dc-ae-f32c32 geometry, synthetic weights, bf16")
    say(f"# {size} x {size}, B = 1, {steps} steps, guidance {gs}, 300 text tokens; host clock around a device synchronise; {a.rounds} rounds after 2 warm calls")

    def encode():
        e, m = pipe._encode("prompt", (ids, mask), None, None, 1, 300, None)
        ne, nm = pipe._encode("negative_prompt", (nids, nmask), None, None, 1, 300, None)
        return e, m, ne, nm
    e, m, ne, nm = encode()
    loop_kw = dict(prompt_embeds=e, prompt_attention_mask=m, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm, num_inference_steps=steps, guidance_scale=gs)
    cat_e, cat_m = torch.cat([ne, e]).contiguous(), torch.cat([nm, m])
    fused = lambda: sana_denoise_loop(tr, pipe.scheduler, latents=lat.clone(), **loop_kw)
    unfused = lambda: torch_loop(tr, pipe.scheduler, lat.clone(), cat_e, cat_m, steps, gs)
    out_f, out_u = fused(), unfused()
    torch.cuda.synchronize()
    same = bool(((out_f.view(torch.int32) == out_u.view(torch.int32)) | (torch.isnan(out_f) & torch.isnan(out_u))).all())
    say(f"# final latents of the fused and the torch-op loop: {'bit-identical' if same else 'DIFFERENT'}; finite: {bool(torch.isfinite(out_f).all())}")
    final = out_f

    def decode():
        img = vae.decode(final.to(vae.dtype) / vae.config.scaling_factor).sample
        return pipe.image_processor.postprocess(img, output_type="pt")
    whole = lambda: pipe(prompt=(ids, mask), negative_prompt=(nids, nmask), num_inference_steps=steps, guidance_scale=gs, height=size, width=size, latents=lat,
                         output_type="pt", max_sequence_length=300).images

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    runs = (("prompt encode (2 prompts)", encode), ("denoise loop, fused step", fused), ("denoise loop, torch-op step", unfused), ("decode + postprocess", decode),
            ("whole call", whole))
    for _, f in runs:
        f(); f()
    ms = {n: [] for n, _ in runs}
    for _ in range(a.rounds):                            # interleaved: every round takes each stage once, the two loops next to each other
        for n, f in runs:
            ms[n].append(clock(f))
    say("# stage                            median ms      min      max")
    for n, v in ms.items():
        say(f"  {n:30s} {statistics.median(v):10.2f} {min(v):8.2f} {max(v):8.2f}")
    mf, mu = statistics.median(ms["denoise loop, fused step"]), statistics.median(ms["denoise loop, torch-op step"])
    spread = max(max(v) - min(v) for k, v in ms.items() if k.startswith("denoise"))
    say(f"# loop: torch-op step minus fused step = {mu - mf:+.2f} ms of {mu:.2f} ms ({100 * (mu - mf) / mu:+.2f} %); the two loops' own spread (max - min) is up to {spread:.2f} ms")

    # the step alone
    n_it = 200
    pred = torch.randn(2, 32, 32, 32, generator=g, device=dev).to(BF)
    x, m1, mi = lat.clone(), torch.randn_like(lat), torch.empty(2, 32, 32, 32, device=dev, dtype=BF)
    coef = (2, 0.7, 0.9, -0.08, 1.1)

    def k_fused():
        for _ in range(n_it):
            ops.dpm_step(pred[:1], pred[1:], gs, x, m1, mi, order=2, sigma=coef[1], a=coef[2], b=coef[3], rinv=coef[4])

    def k_torch():
        xx, mm = x, m1
        for _ in range(n_it):
            o, x0 = torch_step(pred[:1], pred[1:], gs, xx, mm, coef)
            torch.cat([o] * 2).to(BF)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_it
    k_fused(); k_torch()
    us = {"ug_dpm_step": [], "torch ops": []}
    for _ in range(a.rounds):
        us["ug_dpm_step"].append(events(k_fused)); us["torch ops"].append(events(k_torch))
    say(f"# the step alone, [1, 32, 32, 32] fp32 latents, order 2 with guidance and 2 copies; microseconds per step between device events over {n_it} back-to-back steps")
    for n, v in us.items():
        say(f"  {n:30s} {statistics.median(v):10.2f} {min(v):8.2f} {max(v):8.2f}")
    say(f"# per step {statistics.median(us['torch ops']) - statistics.median(us['ug_dpm_step']):.2f} us less, x {steps} steps = "
        f"{(statistics.median(us['torch ops']) - statistics.median(us['ug_dpm_step'])) * steps / 1e3:.3f} ms of a {mf:.2f} ms loop")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
