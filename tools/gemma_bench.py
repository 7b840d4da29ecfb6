"""The Gemma-2 text encoder on the GPU at gemma-2-2b geometry (26 layers, hidden 2304, 8 query heads over 4 K/V heads of 256, feed-forward 9216, vocabulary
256000), random weights, 1 and 8 prompts of 300 tokens: what a Sana prompt encode costs.

    python tools/gemma_bench.py [--out profiles/gemma_bench.log] [--iters 20] [--layers 26]

Milliseconds per encode: the median of `iters` encodes, each between its own pair of HIP events, after three warm-up encodes. The split: one more
encode with a pair of events round every GEMM and every attention launch (ops.KernelTimer); "rest" is the encode's own time in that run minus the two
sums - norms, RoPE, the gated GELU, the embedding, the mask's host read and the gaps between launches. The event pairs lengthen that run, so its
shares are of its own total, which is printed beside the undisturbed median. The second prompt of each batch is padded from token 211 on."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigen_amd import lib as L  # noqa: E402
from unigen_amd import ops  # noqa: E402
from unigen_amd.gemma import Gemma2Model  # noqa: E402

GEMMA_2_2B = dict(vocab_size=256000, hidden_size=2304, num_hidden_layers=26, num_attention_heads=8, num_key_value_heads=4, head_dim=256, intermediate_size=9216,
                  rms_norm_eps=1e-6, query_pre_attn_scalar=256, attn_logit_softcapping=50.0, sliding_window=4096, hidden_activation="gelu_pytorch_tanh")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gemma_bench.log"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=26)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gemma_bench.py measures on the GPU: no GPU visible")
    dev = torch.device("cuda:0")
    L.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    model = Gemma2Model(dict(GEMMA_2_2B, num_hidden_layers=a.layers), device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(0)
    for t in model.state_dict().values():          # on the device: the embedding alone is 590 M values
        t.copy_(torch.randn(t.shape, generator=g, device=dev) * ((0.7 / t.shape[1] ** 0.5) if t.dim() == 2 else 0.1))
    say(f"# tools/gemma_bench.py on {torch.cuda.get_device_name(0)}; gemma-2-2b geometry, {a.layers} layers, 300 tokens, bf16, random weights; median of {a.iters}")
    say("# prompts   ms per encode   with event pairs: total ms = GEMMs (launches) + attention (launches) + rest;  shares of that total")
    for B in (1, 8):
        ids = torch.randint(0, 256000, (B, 300), generator=g, device=dev, dtype=torch.int32)
        mask = torch.ones(B, 300, dtype=torch.int64, device=dev)
        if B > 1:
            mask[1, 211:] = 0
        for _ in range(3):
            model(ids, attention_mask=mask)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(ids, attention_mask=mask)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = sorted(times)[len(times) // 2]
        timer = ops.KernelTimer(("gemm", "attn"))
        ops.set_timer(timer)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(ids, attention_mask=mask)
        e1.record()
        torch.cuda.synchronize()
        ops.set_timer(None)
        total, s = e0.elapsed_time(e1), timer.summary()
        gm, at = s["gemm"], s["attn"]
        rest = total - gm["ms"] - at["ms"]
        say(f"  {B}        {ms:10.3f}      {total:.3f} = {gm['ms']:.3f} ({gm['launches']}) + {at['ms']:.3f} ({at['launches']}) + {rest:.3f};  "
            f"GEMMs {100 * gm['ms'] / total:.1f} %  attention {100 * at['ms'] / total:.1f} %  rest {100 * rest / total:.1f} %")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
