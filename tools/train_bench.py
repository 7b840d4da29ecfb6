"""One training step (forward + backward of the control modules, reference train.py:622-662) at the FLUX-schnell geometry + canny control,
random weights and inputs: seconds per step, samples/s, peak memory. Not the headline metric (BASELINE.json measures inference); the
SURVEY 8(f) rank-4 row. --optim adds the optimizer step of train.py:658-660 (unigen_amd.optim.AdamW(max_grad_norm=1.0): clipping fused, fp32 masters)
to each timed step; --optim --lowp runs that optimizer without masters and with bf16 moments (master_weights=False, state_dtype=bf16: 4 B of state
per trainable element instead of 12) and reports the state's bytes beside the step time and the peak, to be read against a run without --lowp.
--lora R trains rank-R LoRA adapters on the attention projections of the control branch instead, everything else frozen
(HipModule.set_lora_trainable; UniGenFlux only), and also times the same differentiable forward with the adapters switched off.
--objective SCHEME runs every step through unigen_amd.objective.train_step (train.py:589-662: noisy input, timesteps and loss weighting from the
HIP objective kernels, loss, backward, the --optim optimizer) instead of the inline MSE against a fixed target, times the whole step, and then
times the objective's own launches (prepare + loss forward / backward, HIP events) beside the torch-eager restatement of the same lines.
usage: python tools/train_bench.py [--batch 1] [--size 1024] [--ckpt] [--layers 19 38] [--optim [--lowp]] [--lora R] [--objective SCHEME]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unigen_amd.flux import UniGenFlux
from unigen_amd.pipeline import prepare_latent_image_ids

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--ckpt", action="store_true")
ap.add_argument("--layers", type=int, nargs=2, default=None)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--sd3", action="store_true", help="UniGenSD3 (SD3.5-medium geometry, depth control, transformer-block experts) instead of UniGenFlux")
ap.add_argument("--no-gradnorm", action="store_true", help="skip the per-step gradient-norm diagnostic (hundreds of small torch kernels: keep it out of rocprofv3 kernel statistics)")
ap.add_argument("--shapes", action="store_true", help="per-shape table of the last step's GEMM / attention launches (grouped by FLOPs per launch)")
ap.add_argument("--optim", action="store_true", help="time unigen_amd.optim.AdamW(lr=1e-4, weight_decay=1e-2, max_grad_norm=1.0).step() after each backward")
ap.add_argument("--lowp", action="store_true", help="with --optim: AdamW(master_weights=False, state_dtype=torch.bfloat16), stochastic rounding")
ap.add_argument("--lora", type=int, default=0, metavar="R", help="train rank-R adapters on the control branch's attention projections, base and control modules frozen")
ap.add_argument("--objective", default=None, metavar="SCHEME", help="run the step through unigen_amd.objective.train_step with this weighting scheme (none, sigma_sqrt, cosmap, "
                "logit_normal, mode); implies --optim (same AdamW, clipping fused into its step)")
a = ap.parse_args()
if a.objective:
    a.optim = True
if a.lowp and not a.optim:
    ap.error("--lowp is an option of --optim (or --objective)")
if a.lora and a.sd3:
    ap.error("--lora is implemented for UniGenFlux only")
dev, BF = torch.device("cuda:0"), torch.bfloat16
B = a.batch
g = torch.Generator(device=dev).manual_seed(5)
rn = lambda *s: torch.randn(*s, generator=g, device=dev)
if a.sd3:
    from unigen_amd.sd3 import UniGenSD3
    model = UniGenSD3.from_config({}, device=dev, dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=False))
    model.init_synthetic_(seed=0, std=0.02)
    model.init_trainable_param()
    if a.ckpt:
        model.enable_gradient_checkpointing()
    hw = a.size // 8
    c = model.config
    inp = dict(hidden_states=rn(B, c.in_channels, hw, hw).to(BF), condition_hidden_states=rn(B, c.in_channels, hw, hw).to(BF),
               encoder_hidden_states=(0.1 * rn(B, 333, c.joint_attention_dim)).to(BF), pooled_projections=rn(B, c.pooled_projection_dim).to(BF),
               condition_pooled_projections=rn(B, c.pooled_projection_dim).to(BF))
    t = torch.full((B,), 600.0, device=dev)
    fwd = lambda: model(timestep=t, **inp)
    target = rn(B, 16, hw, hw)
    latents = rn(B, c.in_channels, hw, hw).to(BF)
else:
    cfg = {} if a.layers is None else {"num_layers": a.layers[0], "num_single_layers": a.layers[1]}
    model = UniGenFlux.from_config(cfg, device=dev, dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(
        use_rope=True, use_shared_expert=True, use_consis_module=False, use_single_trans_blocks=True, single_control_dev=2,
        single_block_control_method="overall_add", top_num=1, expert_num_each_condition=3))
    model.init_synthetic_(seed=0, std=0.02)
    if a.lora:
        model.add_lora(["attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0"], "canny", a.lora, 2.0 * a.lora, prefix="control_", init_lora_weights=False)
        model.set_lora_trainable()
    else:
        model.init_trainable_param()
    if a.ckpt:
        model.enable_gradient_checkpointing()
    grid, T = a.size // 16, 512
    N = grid * grid
    inp = dict(hidden_states=rn(B, N, 64).to(BF), condition_hidden_states=rn(B, N, 64).to(BF), encoder_hidden_states=(0.1 * rn(B, T, 4096)).to(BF),
               pooled_projections=rn(B, 768).to(BF), condition_pooled_projections=rn(B, 768).to(BF))
    ids = prepare_latent_image_ids(grid, grid, dev, BF)
    txt = torch.zeros(T, 3, device=dev, dtype=BF)
    t = torch.full((B,), 0.75, device=dev, dtype=BF)
    fwd = lambda: model(timestep=t, img_ids=ids, txt_ids=txt, condition_ids=ids, **inp)
    target = rn(B, N, 64)
    latents = rn(B, 16, 2 * grid, 2 * grid).to(BF)
n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
n_all = sum(p.numel() for p in model.parameters())
from unigen_amd import ops
opt = None
if a.optim:
    from unigen_amd.optim import AdamW
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0,
                **(dict(master_weights=False, state_dtype=BF, seed=0) if a.lowp else {}))
times, opt_times = [], []
objective = batch = None
if a.objective:
    from unigen_amd.objective import FlowMatchObjective, train_step
    objective = FlowMatchObjective(a.objective, pack=not a.sd3, shift=3.0 if a.sd3 else 1.0, timestep_scale=1000.0 if a.sd3 else 1.0)
    batch = dict({k: v for k, v in inp.items() if k != "hidden_states"}, latents=latents)
    if not a.sd3:
        batch.update(img_ids=ids, txt_ids=txt, condition_ids=ids)
timer = None
if a.lora:                         # the same differentiable forward with every adapter switched off (no adapter launch): what the adapters add to it
    from unigen_amd.lora import enable_lora
    fw_off = []
    with enable_lora(list(model.modules()), []):
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.time()
            o_ = fwd()
            torch.cuda.synchronize(); fw_off.append(time.time() - t0)
            del o_
    for m_ in model._lora_sites.values():
        m_.unscale_layer(None)         # enable_lora's exit multiplies by alpha / r again (the reference's behaviour): back to alpha / r
    torch.cuda.reset_peak_memory_stats()
for step in range(a.steps + 1):
    if step == a.steps:            # HIP events around every GEMM / attention launch of the last step (not part of the timed minimum)
        timer = ops.KernelTimer(kinds=("gemm", "attn", "attn_bwd")); ops.set_timer(timer)
    for p in model.parameters():
        p.grad = None
    if objective is not None:          # the whole of train.py:589-662 in one call; clipping is fused into the optimizer's step (as with --optim alone)
        from unigen_amd import autograd as A_
        torch.cuda.synchronize(); t0 = time.time()
        res = train_step(model, opt, objective, batch, max_grad_norm=None, generator=g)
        A_.clear_activation_cache()
        torch.cuda.synchronize(); t1 = time.time()
        if step and timer is None:
            times.append((t1 - t0, 0.0)); opt_times.append(0.0)
        print(f"step {step}: loss {float(res['step_loss']):.5f} grad-norm {float(opt.last_grad_norm):.4e} train_step {t1 - t0:.3f}s", flush=True)
        continue
    torch.cuda.synchronize(); t0 = time.time()
    out, losses, _ = fwd()
    torch.cuda.synchronize(); t1 = time.time()
    loss = ((out.float() - target) ** 2).reshape(B, -1).mean(1).mean() + losses["moe_loss"]
    loss.backward()
    from unigen_amd import autograd as A_
    A_.clear_activation_cache()      # the last activation transposes (and the tensors they pin) must not outlive the step
    torch.cuda.synchronize(); t2 = time.time()
    if step and timer is None:
        times.append((t1 - t0, t2 - t1))
    if opt is not None:
        opt.step()
        torch.cuda.synchronize(); t3 = time.time()
        if step and timer is None:
            opt_times.append(t3 - t2)
    gn = float("nan") if a.no_gradnorm else float(torch.sqrt(sum((p.grad.float() ** 2).sum() for p in model.parameters() if p.grad is not None)))
    print(f"step {step}: loss {float(loss):.5f} grad-norm {gn:.4e} forward {t1 - t0:.3f}s backward {t2 - t1:.3f}s", flush=True)
ops.set_timer(None)
rates = {k: dict(launches=v["launches"], ms=round(v["ms"], 1), tflops=round(v["flops"] / v["ms"] / 1e9, 1)) for k, v in timer.summary().items()}
fw, bw = min(x[0] for x in times), min(x[1] for x in times)
extra = {}
if opt is not None:
    op = min(opt_times)
    extra = dict(optimizer_s=round(op, 4), step_s=round(fw + bw + op, 4), step_samples_per_s=round(B / (fw + bw + op), 3), optimizer_grad_norm=round(float(opt.last_grad_norm), 5),
                 optimizer_state="no masters, bf16 moments" if a.lowp else "fp32 masters and moments",
                 optimizer_state_gb=round(sum(t.numel() * t.element_size() for st in opt.state.values() for t in st.values() if torch.is_tensor(t) and t.is_cuda) / 2 ** 30, 2))
if objective is not None:              # the step is timed as a whole: forward_s holds it, backward_s / optimizer_s are 0
    extra.update(objective=a.objective, step_s=round(fw, 4))
    # the objective's own launches by HIP events, beside the torch-eager restatement of train.py:598-613 and :644-652 (without get_sigmas' host
    # synchronisation per sample, which eager cannot avoid in the reference: this comparison favours eager)
    from unigen_amd.pipeline import pack_latents
    pred = (rn(*((B, 16, a.size // 8, a.size // 8) if a.sd3 else (B, N, 64))).to(BF)).requires_grad_(True)
    noise, u = torch.randn_like(latents), torch.rand(B, device=dev)
    table, T_ = objective.sigma_table(dev), objective.num_train_timesteps

    def hip_lines():
        noisy, tgt, ts, sig, w = objective.prepare(latents, noise=noise, u=u)
        objective.loss(pred, tgt, w)[0].backward()

    def eager_lines():
        s32 = table[(u * T_).long().clamp(max=T_ - 1)]
        ts = s32 * T_ / 1000
        sig = s32.to(BF).reshape(-1, 1, 1, 1)
        noisy = (1.0 - sig) * latents + sig * noise
        tgt = noise - latents
        if not a.sd3:
            noisy, tgt = pack_latents(noisy), pack_latents(tgt)
        weighting = torch.ones_like(sig) if a.objective != "cosmap" else 2 / (3.141592653589793 * (1 - 2 * sig + 2 * sig ** 2))
        if a.objective == "sigma_sqrt":
            weighting = (sig ** -2.0).float()
        flow = torch.mean((weighting.float().reshape(B, *([1] * (pred.dim() - 1))) * (pred.float() - tgt.float()) ** 2).reshape(B, -1), 1)
        flow.mean().backward()

    def timed(fn, reps=50):
        for _ in range(5):
            fn(); pred.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = float("inf")
        for _ in range(3):
            torch.cuda.synchronize(); e0.record()
            for _ in range(reps):
                fn(); pred.grad = None
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps)
        return best
    hip_ms, eager_ms = timed(hip_lines), timed(eager_lines)
    extra.update(objective_hip_ms=round(hip_ms, 4), objective_eager_ms=round(eager_ms, 4), objective_share_of_step=round(hip_ms * 1e-3 / fw, 6))
if a.lora:
    extra.update(lora_rank=a.lora, lora_sites=len(model._lora_sites), forward_adapters_off_s=round(min(fw_off[1:]), 3), backward_over_forward=round(bw / fw, 2))
print("TRAIN_BENCH", json.dumps(dict(**extra, model="UniGenSD3" if a.sd3 else "UniGenFlux", batch=B, size=a.size, layers=[model.config.num_layers, getattr(model.config, "num_single_layers", 0)], checkpointing=bool(a.ckpt),
      params_total=n_all, params_trainable=n_train, forward_s=round(fw, 3), backward_s=round(bw, 3), samples_per_s=round(B / (fw + bw), 3),
      peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), kernel_rates=rates)))

if a.shapes:
    import collections
    groups = collections.defaultdict(list)
    for kind, flops, e0, e1 in timer.records:
        groups[(kind, round(flops / 1e9))].append(e0.elapsed_time(e1))
    tot = sum(sum(v) for v in groups.values())
    print(f"{'kind':9s} {'GFLOP/launch':>13s} {'launches':>8s} {'avg us':>9s} {'TFLOP/s':>9s} {'share':>7s}")
    for (kind, gf), v in sorted(groups.items(), key=lambda kv: -sum(kv[1]))[:40]:
        avg = sum(v) / len(v)
        print(f"{kind:9s} {gf:13d} {len(v):8d} {avg * 1e3:9.1f} {gf / max(avg, 1e-9):9.1f} {sum(v) / tot:7.1%}")
