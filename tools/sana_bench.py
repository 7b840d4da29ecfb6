"""Sana on the GPU: the two kernels of csrc/sana.hip alone, then one block and a 20-layer model forward at Sana-1.6B geometry.

    python tools/sana_bench.py [--out profiles/sana_bench.log] [--iters 50] [--layers 20]
    python tools/sana_bench.py --train [--out profiles/sana_train_bench.log] [--iters 20] [--layers 20]

Kernels: microseconds per call (HIP events around `iters` back-to-back calls after a warm-up) and the bytes the algorithm has to move over that time -
linear attention: q, k, v read and o written once (8 B N H 32 bytes in bf16; the fp32 partial states are extra traffic and are reported on their own
line); GLU convolution: x [B N 2C] read once and out [B N Cp] written once. For comparison the same run measures the rate two elementwise kernels of
this library reach on tensors of the convolution's input size (ug_add_bf16: two DISTINCT inputs read and one output written, 6 bytes per element;
ug_gelu_tanh: a read and a write, 4 bytes per element). Rates are bytes over time, not a share of any peak, and none of them is an HBM rate: every
loop runs back to back on buffers of 24 - 550 MB, so the smaller shapes are served partly from the 256 MB last-level cache.
Block and model: milliseconds per forward and the per-kernel-class split from HIP events around every launch of the timed classes (ops.KernelTimer);
"other" is the rest (AdaLN modulate, adds, RMSNorm, small linears, layout changes, launch gaps).

--train: the two backward kernels of csrc/sana_bwd.hip alone at Sana-1.6B width, 64 x 64 tokens, B = 1 and 4, each beside a torch-eager composite of
the same formulas (fp32 on the GPU from the same bf16 operands), the two interleaved in one process (rounds of a few calls each, the median round
reported); then forward + backward of the model after set_trainable(True) - every parameter takes a gradient, no checkpointing - with HIP events round
the forward and round the backward, beside the inference forward of the same model."""
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


def eager_state(k, v, B, H, N):
    """S [B, H, d, j] and z [B, H, j] in fp32: what the kernel is handed as `state`; computed outside the timed region"""
    f = lambda t: t.view(B, N, H, 32).transpose(1, 2).float()
    kk = f(k).clamp_min(0)
    return torch.einsum("bhnd,bhnj->bhdj", f(v), kk), kk.sum(-2)


def eager_linear_attn_bwd(q, k, v, do, S, z, B, H, N):
    """the formulas of ug_linear_attn_bwd as torch ops in fp32 from the same inputs as the kernel - q, k, v, do [B N, H 32] bf16 and the forward's
    state S, z - -> dq, dk, dv bf16. The widening of the operands to fp32 [B, H, N, 32] is part of the timed work: eager has no other way to them."""
    f = lambda t: t.view(B, N, H, 32).transpose(1, 2).float()
    q, k, v, do = f(q), f(k), f(v), f(do)
    qq, kk = q.clamp_min(0), k.clamp_min(0)
    den = torch.einsum("bhj,bhnj->bhn", z, qq) + 1e-15
    o = torch.einsum("bhdj,bhnj->bhnd", S, qq) / den[..., None]
    g = do / den[..., None]
    c = -(do * o).sum(-1) / den
    dq = (torch.einsum("bhnd,bhdj->bhnj", g, S) + c[..., None] * z[..., None, :]) * (q > 0)
    dS, dz = torch.einsum("bhnd,bhnj->bhdj", g, qq), torch.einsum("bhn,bhnj->bhj", c, qq)
    dk = (torch.einsum("bhnd,bhdj->bhnj", v, dS) + dz[..., None, :]) * (k > 0)
    dv = torch.einsum("bhdj,bhnj->bhnd", dS, kk)
    return dq.to(BF), dk.to(BF), dv.to(BF)


def eager_glu_bwd(x, w9, b, do, B, side, C):
    """the formulas of ug_glu_dwconv3x3_bwd as torch elementwise ops over shifted windows (bf16 tensors between the ops, as the kernel rounds; the
    weight-gradient sums in fp32): x [B N, 2C], w9 [9, 2C], b [2C], do [B N, C]"""
    F = torch.nn.functional
    pad = lambda t: F.pad(t, (0, 0, 1, 1, 1, 1))                       # [B, H, W, K]: zeros round the image
    win = lambda t, ky, kx: t[:, ky:ky + side, kx:kx + side]
    dsilu = lambda t: torch.sigmoid(t) * (1 + t * (1 - torch.sigmoid(t)))
    xi = x.view(B, side, side, 2 * C)
    ap = pad(F.silu(xi))
    y = b + sum(win(ap, ky, kx) * w9[3 * ky + kx] for ky in range(3) for kx in range(3))
    yv, yg, d = y[..., :C], y[..., C:], do.view(B, side, side, C)
    dy = torch.cat([d * F.silu(yg), d * yv * dsilu(yg)], -1)
    dyp = pad(dy)
    da = sum(win(dyp, 2 - ky, 2 - kx) * w9[3 * ky + kx] for ky in range(3) for kx in range(3))
    dx = da * dsilu(xi)
    dyf = dy.float()
    dw = torch.stack([(dyf * win(ap, ky, kx)).sum((0, 1, 2)) for ky in range(3) for kx in range(3)])
    return dx, dw, dyf.sum((0, 1, 2))


def interleaved(fns, iters, rounds=5):
    """{name: median over the rounds of microseconds per call}, the candidates taking turns round by round"""
    got = {n: [] for n in fns}
    for n, fn in fns.items():
        fn()
    for _ in range(rounds):
        for n, fn in fns.items():
            got[n].append(timed(fn, iters, warmup=1))
    return {n: sorted(v)[len(v) // 2] for n, v in got.items()}


def train_bench(a, dev, say):
    g = torch.Generator(device=dev).manual_seed(0)
    H, C, side = WIDTHS["1.6B"]["heads"], WIDTHS["1.6B"]["C"], 64
    D, N = H * 32, side * side
    say("# kernel alone vs the torch-eager composite of the same formulas, interleaved; Sana-1.6B width, 64 x 64 tokens")
    say("# kernel                  B   HIP us    eager us   eager / HIP")
    for B in (1, 4):
        M = B * N
        qkv, do = torch.randn(M, 3 * D, generator=g, device=dev).to(BF), torch.randn(M, D, generator=g, device=dev).to(BF)
        o, dqkv = torch.empty(M, D, dtype=BF, device=dev), torch.empty(M, 3 * D, dtype=BF, device=dev)
        ws = torch.empty(ops.linear_attn_workspace_bytes(B, H, N), dtype=torch.uint8, device=dev)
        wsb = torch.empty(ops.linear_attn_bwd_workspace_bytes(B, H, N), dtype=torch.uint8, device=dev)
        s3, s1 = (3 * D, N * 3 * D), (D, N * D)
        kw = dict(batches=B, heads=H, N=N, q_strides=s3, k_strides=s3, v_strides=s3)
        ops.linear_attn(qkv, qkv[:, D:], qkv[:, 2 * D:], o, o_strides=s1, workspace=ws, **kw)
        state = ws[:B * H * 1056 * 4].view(torch.float32).clone()
        eS, ez = eager_state(qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, N)
        r = interleaved({"hip": lambda: ops.linear_attn_bwd(qkv, qkv[:, D:], qkv[:, 2 * D:], do, state, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], do_strides=s1,
                                                            dq_strides=s3, dk_strides=s3, dv_strides=s3, workspace=wsb, **kw),
                         "fwd": lambda: ops.linear_attn(qkv, qkv[:, D:], qkv[:, 2 * D:], o, o_strides=s1, workspace=ws, **kw),
                         "eager": lambda: eager_linear_attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], do, eS, ez, B, H, N)}, a.iters)
        say(f"ug_linear_attn_bwd        {B}  {r['hip']:8.1f}  {r['eager']:10.1f}  {r['eager'] / r['hip']:8.2f}    (forward kernel {r['fwd']:.1f} us: backward / forward {r['hip'] / r['fwd']:.2f})")
        del qkv, do, o, dqkv
        x, dout = torch.randn(M, 2 * C, generator=g, device=dev).to(BF), torch.randn(M, C, generator=g, device=dev).to(BF)
        w9, b = (torch.randn(9, 2 * C, generator=g, device=dev) / 3).to(BF), (0.1 * torch.randn(2 * C, generator=g, device=dev)).to(BF)
        out, dx = torch.empty(M, C, dtype=BF, device=dev), torch.empty(M, 2 * C, dtype=BF, device=dev)
        dw9, db = torch.empty(9, 2 * C, dtype=torch.float32, device=dev), torch.empty(2 * C, dtype=torch.float32, device=dev)
        wsg = torch.empty(ops.glu_dwconv3x3_bwd_workspace_bytes(B, side, side, C), dtype=torch.uint8, device=dev)
        gk = dict(B=B, H=side, W=side, C=C)
        r = interleaved({"hip": lambda: ops.glu_dwconv3x3_bwd(x, w9, b, dout, dx, dw9=dw9, dbias=db, workspace=wsg, **gk),
                         "frozen": lambda: ops.glu_dwconv3x3_bwd(x, w9, b, dout, dx, workspace=wsg, **gk),
                         "fwd": lambda: ops.glu_dwconv3x3(x, w9, b, out, **gk),
                         "eager": lambda: eager_glu_bwd(x, w9, b, dout, B, side, C)}, max(2, a.iters // 4))
        say(f"ug_glu_dwconv3x3_bwd      {B}  {r['hip']:8.1f}  {r['eager']:10.1f}  {r['eager'] / r['hip']:8.2f}    (without dw9 / dbias {r['frozen']:.1f} us; forward kernel "
            f"{r['fwd']:.1f} us: backward / forward {r['hip'] / r['fwd']:.2f})")
        del x, dout, out, dx, wsg
    say()
    say(f"# model, Sana-1.6B geometry, {a.layers} layers, 64 x 64 tokens, 300 text tokens, random weights; set_trainable(True), no checkpointing")
    say("# median of three timed iterations after two warm-up ones; no optimizer step between them")
    say("# B   inference forward ms   training forward ms   backward ms   backward / forward   step (fwd + bwd) ms")
    from unigen_amd import autograd as A
    model = SanaTransformer2DModel(dict(SANA_1600M, num_layers=a.layers), device=dev, dtype=BF).init_synthetic_(0)
    for B in (1, 4):
        x = torch.randn(B, 32, side, side, generator=g, device=dev).to(BF)
        cap = torch.randn(B, 300, 2304, generator=g, device=dev).to(BF)
        wl = torch.randn(B, 32, side, side, generator=g, device=dev)
        ts = torch.full((B,), 500.0, device=dev)
        with torch.no_grad():
            inf_us = timed(lambda: model(x, cap, ts), 3, warmup=2)
        model.set_trainable(True)
        fw, bw = [], []
        for it in range(2 + 3):
            for t in model.trainable_parameters().values():
                t.grad = None
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            loss = (model(x, cap, ts).float() * wl).mean()
            ev[1].record()
            loss.backward()
            ev[2].record()
            torch.cuda.synchronize()
            A.clear_activation_cache()
            if it >= 2:
                fw.append(ev[0].elapsed_time(ev[1]))
                bw.append(ev[1].elapsed_time(ev[2]))
        f, b_ = sorted(fw)[1], sorted(bw)[1]
        say(f"  {B}   {inf_us / 1e3:18.2f}   {f:19.2f}   {b_:11.2f}   {b_ / f:18.2f}   {f + b_:19.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time the backward kernels and forward + backward of the model instead")
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--layers", type=int, default=20)
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "sana_train_bench.log" if a.train else "sana_bench.log")
    a.iters = a.iters or (20 if a.train else 50)
    if not torch.cuda.is_available():
        raise SystemExit("tools/sana_bench.py measures on the GPU: no GPU visible")
    dev = torch.device("cuda:0")
    L.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.train:
        say(f"# tools/sana_bench.py --train on {torch.cuda.get_device_name(0)}; iters {a.iters}; bf16")
        train_bench(a, dev, say)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)
        return

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
