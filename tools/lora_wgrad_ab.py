"""Interleaved A/B, in ONE process, of the two routes to an adapter gradient C[R, J] = P[M, R]^T Q[M, J] (dA_cat = dT^T X, dB_bd^T = T^T dY):
  old   ops.transpose of both operands (zero-padded to a multiple of 64 rows) + ops.gemm - what autograd._wgrad runs for a weight gradient;
        the transposes are part of the route and are timed with it
  new   ug_lora_wgrad_bf16 (csrc/lora_bwd.hip): both operands row-major, read once
at the activation shapes of the full-size model, R = 64. Checks both against a float64 product first. Also prints the new kernel's rate over the
bytes it has to move (P + Q + C once) so that it can be set beside the streaming rate of tools/bwd_elementwise_bench.py.

    python tools/lora_wgrad_ab.py [--quick]
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unigen_amd import ops

dev = torch.device("cuda:0")
BF = torch.bfloat16
R = 64
SHAPES = [(M, K, N) for M in (8192, 18432) for K, N in ((3072, 9216), (3072, 21504), (15360, 3072))]
if "--quick" in sys.argv:
    SHAPES = SHAPES[:1]
g = torch.Generator(device=dev).manual_seed(0)


def old_route(p, q):
    Mp = (p.shape[0] + 63) // 64 * 64
    pt, qt = ops.transpose(p, Mp), ops.transpose(q, Mp)              # [R, Mp], [J, Mp]
    out = torch.empty(p.shape[1], q.shape[1], device=dev, dtype=BF)
    return ops.gemm(pt, qt, None, out, M=p.shape[1])


def new_route(p, q):
    return ops.lora_wgrad(p, q)


def timed(fn, p, q, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn(p, q)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


print(f"{'product':10s} {'M':>6s} {'J':>6s}   old us  new us  speedup   new GB/s   rel err old / new (vs float64)", flush=True)
for M, K, N in SHAPES:
    for label, J in (("dA_cat", K), ("dB_bd^T", N)):
        p = (torch.randn(M, R, generator=g, device=dev) * 0.5).to(BF)
        q = torch.randn(M, J, generator=g, device=dev).to(BF)
        truth = p.double().t() @ q.double()
        rel = lambda c: float((c.double() - truth).norm() / truth.norm())
        c_old, c_new = old_route(p, q), new_route(p, q)
        torch.cuda.synchronize()
        e_old, e_new = rel(c_old), rel(c_new)
        del truth
        for fn in (old_route, new_route):
            fn(p, q); fn(p, q)
        torch.cuda.synchronize()
        t = {"old": [], "new": []}
        for _ in range(9):
            t["old"].append(timed(old_route, p, q))
            t["new"].append(timed(new_route, p, q))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        byts = 2.0 * (M * R + M * J + R * J)
        print(f"{label:10s} {M:6d} {J:6d}  {med['old'] * 1e3:7.1f} {med['new'] * 1e3:7.1f}  {med['old'] / med['new']:6.2f}x  {byts / med['new'] / 1e6:8.0f}   "
              f"{e_old:.2e} / {e_new:.2e}   (best old {min(t['old']) * 1e3:.1f}, new {min(t['new']) * 1e3:.1f} us)", flush=True)
        assert e_new <= 2.0 ** -8, e_new
