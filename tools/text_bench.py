"""Time the text encoders at their real geometries with random weights: T5-XXL (24 layers, d_model 4096, 64 heads of 64, d_ff 10240, L = 512,
B = 1 and 4) and CLIP-L (12 layers, 768 wide, 12 heads, L = 77, B = 1 and 4). Prints one JSON line per case: ms per encode (HIP events over
`--iters` encodes after `--warmup`) and, from a second pass with per-launch events, the split into GEMM / attention / everything else
(norms, activations, gathers, launch gaps).

    python tools/text_bench.py [--iters 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from unigen_amd import ops  # noqa: E402
from unigen_amd.text import CLIPTextModel, T5EncoderModel  # noqa: E402

T5_XXL = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, relative_attention_num_buckets=32,
              relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
CLIP_L = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=77,
              hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)


def fill(model, seed):
    g = torch.Generator(device=model.device).manual_seed(seed)
    for name, t in model.state_dict().items():
        if t.dim() == 2 and "relative_attention_bias" not in name:
            t.copy_(torch.randn(t.shape, generator=g, device=t.device) * (0.7 / t.shape[1] ** 0.5))
        elif "norm" in name and name.endswith("weight"):
            t.fill_(1.0)
        else:
            t.copy_(torch.randn(t.shape, generator=g, device=t.device) * 0.1)
    model._invalidate()


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, cls, cfg, Lq in (("t5_xxl", T5EncoderModel, T5_XXL, 512), ("clip_l", CLIPTextModel, CLIP_L, 77)):
        model = cls.from_config(cfg, device=dev, dtype=torch.bfloat16)
        fill(model, 1)
        for B in (1, 4):
            ids = torch.randint(3, 1000, (B, Lq), device=dev)
            if name == "clip_l":
                ids[:, -1] = cfg["eos_token_id"]
            ms = timed(lambda: model(ids), a.iters, a.warmup)
            timer = ops.KernelTimer()
            ops.set_timer(timer)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(ids)
            e1.record()
            torch.cuda.synchronize()
            ops.set_timer(None)
            s = timer.summary()
            total = e0.elapsed_time(e1)
            gemm, attn = s.get("gemm", dict(ms=0.0, flops=0.0)), s.get("attn", dict(ms=0.0, flops=0.0))
            print(json.dumps(dict(case=name, B=B, L=Lq, ms_per_encode=round(ms, 3), instrumented_ms=round(total, 3), gemm_ms=round(gemm["ms"], 3),
                                  gemm_tflops=round(gemm["flops"] / max(gemm["ms"], 1e-9) / 1e9, 1), attn_ms=round(attn["ms"], 3),
                                  attn_tflops=round(attn["flops"] / max(attn["ms"], 1e-9) / 1e9, 1), other_ms=round(total - gemm["ms"] - attn["ms"], 3))), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
