"""Interleaved A/B, in ONE process, of the two routes to the adapters' skinny "down" product T[M, R] = X[M, K] A[R, K]^T (the training forward's
T = x A_cat^T; the backward's dT = dY B_bd with A = B_bd^T and K = N):
  old   ops.gemm at N = R (ug_gemm_bf16, one tile column of its 128^2 kernel)
  new   ug_lora_down_bf16 (tools/probe/csrc/lora_down.hip: probe library only, `python -m unigen_amd.build --probe`)
at the activation shapes of the full-size model, R = 64. To keep the operands out of the 256 MB last-level cache between repetitions the timed
loop rotates over enough operand copies to exceed 512 MB. Checks both against a float64 product first.

    python tools/lora_down_ab.py [--quick]
"""
import ctypes as C, os, sys
os.environ.setdefault("UG_LIB_PATH", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probe", "libunigen_hip_probe.so"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unigen_amd import ops, lib as L

dev, BF, R = torch.device("cuda:0"), torch.bfloat16, 64
SHAPES = [(M, K) for M in (8192, 18432) for K in (3072, 9216, 15360, 21504)]
if "--quick" in sys.argv:
    SHAPES = SHAPES[:1]
g = torch.Generator(device=dev).manual_seed(0)
old = lambda x, a: ops.gemm(x, a, None, torch.empty(x.shape[0], R, device=dev, dtype=BF), M=x.shape[0])
_down = L.load().ug_lora_down_bf16
_down.restype, _down.argtypes = C.c_int32, [C.c_void_p, C.c_int64] * 3 + [C.c_int64] * 3 + [C.c_void_p]


def new(x, a):
    out = torch.empty(x.shape[0], a.shape[0], device=dev, dtype=BF)
    L.check(_down(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), out.data_ptr(), out.stride(0), x.shape[0], a.shape[0], x.shape[1],
                  torch.cuda.current_stream().cuda_stream), "ug_lora_down_bf16")
    return out


def timed(fn, xs, a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for x in xs:
        fn(x, a)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / len(xs)


print(f"{'M':>6s} {'K':>6s} copies   old us  new us  speedup   new GB/s   rel err old / new (vs float64)", flush=True)
for M, K in SHAPES:
    n = max(2, -(-(512 << 20) // (2 * M * K)))
    xs = [torch.randn(M, K, generator=g, device=dev).to(BF) for _ in range(n)]
    a = (torch.randn(R, K, generator=g, device=dev) * K ** -0.5).to(BF)
    truth = xs[0].double() @ a.double().t()
    rel = lambda c: float((c.double() - truth).norm() / truth.norm())
    e_old, e_new = rel(old(xs[0], a)), rel(new(xs[0], a))
    del truth
    for fn in (old, new):
        timed(fn, xs, a)
    t = {"old": [], "new": []}
    for _ in range(7):
        t["old"].append(timed(old, xs, a))
        t["new"].append(timed(new, xs, a))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    byts = 2.0 * (M * K + R * K + M * R)
    print(f"{M:6d} {K:6d} {n:6d}  {med['old'] * 1e3:7.1f} {med['new'] * 1e3:7.1f}  {med['old'] / med['new']:6.2f}x  {byts / med['new'] / 1e6:8.0f}   "
          f"{e_old:.2e} / {e_new:.2e}   (best old {min(t['old']) * 1e3:.1f}, new {min(t['new']) * 1e3:.1f} us)", flush=True)
    assert e_new <= 2.0 ** -8, e_new
    del xs
