"""Optimizer step over the real trainable tensor list of the full-depth model (reference train.py:652-662: clip_grad_norm_ + AdamW.step()):
743 tensors / 6.89 B elements of UniGenFlux + canny, or with --sd3 1203 tensors / 3.0 B elements of UniGenSD3 + depth. The shapes come from
a model built on the meta device; params (bf16) and grads (bf16, random) are allocated directly. Three routes, alternated in one process:
  (a) fused:  unigen_amd.optim.AdamW(max_grad_norm=1.0).step()          (norm partials, their sum, the update: three launches)
  (b) split:  unigen_amd.optim.clip_grad_norm_(params, 1.0) + AdamW.step()
  (c) torch:  fp32 master params, grads cast to fp32 (_foreach_copy_), torch.nn.utils.clip_grad_norm_(foreach=True),
              torch.optim.AdamW(fused=True).step(), torch._foreach_copy_ back to the bf16 params
Median ms over --steps after --warmup, and counted bytes / s from the bytes the route must move per element (BYTES below).
--lowp measures the optimizer's low-precision state instead: the default step (fp32 masters and moments) and the three arrangements of
AdamW(master_weights=, state_dtype=) - no master + bf16 moments, no master + fp32 moments, master + bf16 moments - alternated in one process on
the same params and grads (about 231 GiB of state in all for UniGenFlux), with and without the fused clip.
usage: python tools/optim_bench.py [--sd3] [--lowp] [--steps 10] [--warmup 3]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

# bytes per element each route has to move (bf16 param / grad = 2, fp32 master / moment / grad copy = 4)
BYTES = dict(
    fused=2 + 2 + 8 + 8 + 8 + 2,                    # grad read by the norm and by the update; master, m, v read + written; bf16 param written
    split=2 + 4 + 2 + 8 + 8 + 8 + 2,                # + the scaling pass reads and writes the grad
    torch=(2 + 4) + 4 + 8 + (4 + 8 + 8 + 8) + (4 + 2),   # grad cast; norm; scale r/w; fused AdamW (grad, master, m, v); copy back
)


def trainable_shapes(sd3: bool):
    dev, BF = torch.device("meta"), torch.bfloat16
    if sd3:
        from unigen_amd.sd3 import UniGenSD3
        m = UniGenSD3.from_config({}, device=dev, dtype=BF)
        m.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=False))
    else:
        from unigen_amd.flux import UniGenFlux
        m = UniGenFlux.from_config({}, device=dev, dtype=BF)
        m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(
            use_rope=True, use_shared_expert=True, use_consis_module=False, use_single_trans_blocks=True, single_control_dev=2,
            single_block_control_method="overall_add", top_num=1, expert_num_each_condition=3))
    m.init_trainable_param()
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


# --lowp: (master_weights, state_dtype) -> bytes per element of the update launch: grad 2 read; then read + written master 4 / bf16 param 2,
# moments 4 or 2 each; a kept master also writes the bf16 param (2). The fused norm reads the grad once more (+ 2).
LOWP = {
    "default": (True, torch.float32, 2 + 8 + 2 + 8 + 8),
    "nomaster_bf16": (False, torch.bfloat16, 2 + 4 + 4 + 4),
    "nomaster_f32": (False, torch.float32, 2 + 4 + 8 + 8),
    "master_bf16": (True, torch.bfloat16, 2 + 8 + 2 + 4 + 4),
}


def lowp_main(a, AdamW, params, shapes, n):
    """The default step (the yardstick: ug_adamw_step, unchanged) and the three low-precision arrangements (ug_adamw_step_lowp), alternated in one
    process on the same params and grads, each with the fused clip (three launches) and without (the update launch alone)."""
    opts = {k: AdamW(params, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, master_weights=m, state_dtype=sd, seed=1) for k, (m, sd, _) in LOWP.items()}
    times = {(k, clip): [] for k in opts for clip in (True, False)}
    for it in range(a.warmup + a.steps):
        for (k, clip), ts in times.items():        # alternated: every arrangement sees the same machine state
            opts[k].max_grad_norm = 1.0 if clip else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            opts[k].step()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ts.append(e0.elapsed_time(e1))
    res = dict(model="UniGenSD3" if a.sd3 else "UniGenFlux", tensors=len(shapes), elements=n, steps=a.steps, peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    for k, o in opts.items():
        state = sum(t.numel() * t.element_size() for st in o.state.values() for t in st.values() if t.is_cuda)
        res[k] = dict(state_bytes_per_elem=round(state / n, 2))
        for clip in (True, False):
            ms, b = statistics.median(times[(k, clip)]), LOWP[k][2] + (2 if clip else 0)
            res[k]["fused_clip" if clip else "update_only"] = dict(ms=round(ms, 2), min_ms=round(min(times[(k, clip)]), 2), bytes_per_elem=b, counted_tb_s=round(n * b / ms / 1e9, 2))
    for k in list(LOWP)[1:]:
        res[k]["vs_default"] = round(res["default"]["fused_clip"]["ms"] / res[k]["fused_clip"]["ms"], 2)
    print("OPTIM_BENCH_LOWP", json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sd3", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lowp", action="store_true", help="the default step and the three low-precision arrangements instead of the three routes")
    a = ap.parse_args()
    from unigen_amd.optim import AdamW, clip_grad_norm_
    shapes = trainable_shapes(a.sd3)
    n = sum(torch.Size(s).numel() for s in shapes)
    dev, BF = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter((0.02 * torch.randn(s, generator=g, device=dev)).to(BF)) for s in shapes]
    grads = [(1e-3 * torch.randn(s, generator=g, device=dev)).to(BF) for s in shapes]
    for p, gr in zip(params, grads):
        p.grad = gr
    if a.lowp:
        return lowp_main(a, AdamW, params, shapes, n)
    ours = AdamW(params, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)

    def fused():
        ours.max_grad_norm = 1.0
        ours.step()

    def split():
        ours.max_grad_norm = None
        clip_grad_norm_(params, 1.0)
        ours.step()

    masters = [p.detach().float() for p in params]
    for m in masters:
        m.grad = torch.empty_like(m)
    try:
        topt, torch_kind = torch.optim.AdamW(masters, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, fused=True), "fused"
    except (RuntimeError, ValueError):
        topt, torch_kind = torch.optim.AdamW(masters, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, foreach=True), "foreach"
    bf_params = [p.data for p in params]
    m_grads = [m.grad for m in masters]

    def torch_route():
        torch._foreach_copy_(m_grads, grads)
        torch.nn.utils.clip_grad_norm_(masters, 1.0, foreach=True)
        topt.step()
        torch._foreach_copy_(bf_params, masters)

    routes = dict(fused=fused, split=split, torch=torch_route)
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.steps):
        for k, fn in routes.items():              # alternated: every route sees the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
    res = dict(model="UniGenSD3" if a.sd3 else "UniGenFlux", tensors=len(shapes), elements=n, steps=a.steps, torch_adamw=torch_kind,
               peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    for k, v in times.items():
        ms = statistics.median(v)
        res[k] = dict(ms=round(ms, 2), bytes_per_elem=BYTES[k], counted_tb_s=round(n * BYTES[k] / ms / 1e9, 2), min_ms=round(min(v), 2))
    res["fused_vs_torch"] = round(res["torch"]["ms"] / res["fused"]["ms"], 2)
    print("OPTIM_BENCH", json.dumps(res))


if __name__ == "__main__":
    main()
