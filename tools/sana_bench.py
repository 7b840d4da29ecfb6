"""Sana on the GPU: the two kernels of csrc/sana.hip alone, then one block and a 20-layer model forward at Sana-1.6B geometry.

    python tools/sana_bench.py [--out profiles/sana_bench.log] [--iters 50] [--layers 20]

Kernels: microseconds per call (HIP events around `iters` back-to-back calls after a warm-up) and the bytes the algorithm has to move over that time -
linear attention: q, k, v read and o written once (8 B N H 32 bytes in bf16; the fp32 partial states are extra traffic and are reported on their own
line); GLU convolution: x [B N 2C] read once and out [B N Cp] written once. For comparison the same run measures the rate two elementwise kernels of
this library reach on tensors of the convolution's input size (ug_add_bf16: two DISTINCT inputs read and one output written, 6 bytes per element;
ug_gelu_tanh: a read and a write, 4 bytes per element). Rates are bytes over time, not a share of any peak, and none of them is an HBM rate: every
loop runs back to back on buffers of 24 - 550 MB, so the smaller shapes are served partly from the 256 MB last-level cache.
Block and model: milliseconds per forward and the per-kernel-class split from HIP events around every launch of the timed classes (ops.KernelTimer);
"other" is the rest (AdaLN modulate, adds, RMSNorm, small linears, layout changes, launch gaps)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigen_amd import lib as L  # noqa: E402
from unigen_amd import ops  # noqa: E402
from unigen_amd.sana import SanaTransformer2DModel  # noqa: E402

BF = torch.bfloat16
WIDTHS = {"0.6B": dict(heads=36, C=2880), "1.6B": dict(heads=70, C=5600)}
SANA_1600M = dict(in_channels=32, out_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                  cross_attention_head_dim=112, cross_attention_dim=2240, caption_channels=2304, mlp_ratio=2.5, attention_bias=False, sample_size=32,
                  patch_size=1, norm_eps=1e-6, interpolation_scale=None)


def timed(fn, iters, warmup=5):
    """-> microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sana_bench.log"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layers", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sana_bench.py measures on the GPU: no GPU visible")
    dev = torch.device("cuda:0")
    L.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/sana_bench.py on {torch.cuda.get_device_name(0)}; iters {a.iters}; bf16; back-to-back loops: buffers below 256 MB are partly cache-resident")
    say("# kernel                     width  B     N      us/call   counted MB   GB/s")
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (1, 4):
        for N in (1024, 4096):
            side = int(N ** 0.5)
            for name, w in WIDTHS.items():
                H, C = w["heads"], w["C"]
                D, Cp = H * 32, (C + 63) // 64 * 64
                qkv = torch.randn(B * N, 3 * D, generator=g, device=dev).to(BF)
                o = torch.empty(B * N, D, dtype=BF, device=dev)
                ws = torch.empty(ops.linear_attn_workspace_bytes(B, H, N), dtype=torch.uint8, device=dev)
                s3 = (3 * D, N * 3 * D)
                us = timed(lambda: ops.linear_attn(qkv, qkv[:, D:], qkv[:, 2 * D:], o, batches=B, heads=H, N=N, q_strides=s3, k_strides=s3, v_strides=s3,
                                                   o_strides=(D, N * D), workspace=ws), a.iters)
                mb = 8 * B * N * D / 1e6
                say(f"ug_linear_attn               {name}  {B}  {N:5d}  {us:10.1f}  {mb:10.1f}  {mb / us * 1e3:7.0f}    (+ {2 * ws.numel() / 1e6:.1f} MB of fp32 partials written and read)")
                x = torch.randn(B * N, 2 * C, generator=g, device=dev).to(BF)
                w9 = (torch.randn(9, 2 * C, generator=g, device=dev) / 3).to(BF)
                b = (0.1 * torch.randn(2 * C, generator=g, device=dev)).to(BF)
                out = torch.empty(B * N, Cp, dtype=BF, device=dev)
                us = timed(lambda: ops.glu_dwconv3x3(x, w9, b, out, B=B, H=side, W=side, C=C), a.iters)
                mb = 2 * B * N * (2 * C + Cp) / 1e6
                say(f"ug_glu_dwconv3x3             {name}  {B}  {N:5d}  {us:10.1f}  {mb:10.1f}  {mb / us * 1e3:7.0f}")
                y, x2 = torch.empty_like(x), torch.randn(B * N, 2 * C, generator=g, device=dev).to(BF)
                us = timed(lambda: ops.add(x, x2, y), a.iters)
                say(f"  ug_add_bf16 (size of x)   {name}  {B}  {N:5d}  {us:10.1f}  {6 * x.numel() / 1e6:10.1f}  {6 * x.numel() / 1e6 / us * 1e3:7.0f}")
                us = timed(lambda: L.call("ug_gelu_tanh", x.data_ptr(), y.data_ptr(), x.numel(), ops._stream()), a.iters)
                say(f"  ug_gelu_tanh (size of x)  {name}  {B}  {N:5d}  {us:10.1f}  {4 * x.numel() / 1e6:10.1f}  {4 * x.numel() / 1e6 / us * 1e3:7.0f}")
                del qkv, o, ws, x, x2, out, y

    say()
    say("# Sana-1.6B geometry: dim 2240, 70 heads of 32, 20 cross heads of 112 in 128-wide slots, C = 5600 (Cp 5632), 300 text tokens, random weights")
    KINDS = ("gemm", "attn", "linear_attn", "glu_dwconv")
    cfg = dict(SANA_1600M, num_layers=a.layers)
    model = SanaTransformer2DModel(cfg, device=dev, dtype=BF).init_synthetic_(0)
    blk = model.blocks[0]
    for B, side in ((1, 32), (1, 64), (4, 32)):
        N, D = side * side, 2240
        h = torch.randn(B, N, D, generator=g, device=dev).to(BF)
        enc = torch.randn(B, 300, D, generator=g, device=dev).to(BF)
        t6 = (0.1 * torch.randn(B, 6 * D, generator=g, device=dev)).to(BF)
        x = torch.randn(B, 32, side, side, generator=g, device=dev).to(BF)
        cap = torch.randn(B, 300, 2304, generator=g, device=dev).to(BF)
        ts = torch.full((B,), 500.0, device=dev)
        for what, fn, it in (("block", lambda: blk(h, None, enc, None, t6, side, side), max(5, a.iters // 2)),
                             (f"model ({a.layers} layers)", lambda: model(x, cap, ts), max(3, a.iters // 10))):
            us = timed(fn, it, warmup=2)
            timer = ops.KernelTimer(KINDS)
            ops.set_timer(timer)
            fn()
            torch.cuda.synchronize()
            ops.set_timer(None)
            s = timer.summary()
            split = "  ".join(f"{k} {s[k]['ms']:.3f} ms / {s[k]['launches']}" for k in KINDS if k in s)
            say(f"{what:18s} B {B}  N {N:5d}  {us / 1e3:9.3f} ms per forward;  one forward with event pairs (kernel class: ms / launches): {split}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
