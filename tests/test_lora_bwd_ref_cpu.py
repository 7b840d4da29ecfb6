"""The float64 references of tests/lora_bwd_ref.py against torch.autograd of the oracle's LoRA Linear (R.lora_linear) in float64, to 1e-12, as
tests/test_bwd_ref_cpu.py does for its siblings - and the plausible slips of an adapter backward shown to exceed the GPU bounds of
tests/test_lora_train_gpu.py (gradient parity: rel-L2 1e-3 over all adapter gradients, 5e-3 on the worst parameter) at least 10 x. No GPU."""
import pytest
import torch

from oracle import unigen_ref as R
from tests import lora_bwd_ref as ref

F64 = torch.float64
SPECS = [(8, 16.0), (4, 4.0), (16, 8.0)]          # (rank, alpha) of tests/test_lora_gpu.py::SPECS: alpha != r on two of them


def _case(M, K, N, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(dtype)
    x, w, dy = rn(M, K), rn(N, K, std=0.05), rn(M, N)
    A = [rn(r, K, std=K ** -0.5) for r, _ in SPECS]
    B = [rn(N, r, std=0.3) for r, _ in SPECS]
    return x, w, A, B, [a / r for r, a in SPECS], dy


@pytest.mark.parametrize("M,K,N", [(64, 64, 64), (333, 128, 192), (77, 256, 64)])
def test_reference_matches_float64_autograd(M, K, N):
    x, w, A, B, s, dy = _case(M, K, N, seed=M)
    x64 = x.to(F64).requires_grad_(True)
    A64, B64 = [a.to(F64).requires_grad_(True) for a in A], [b.to(F64).requires_grad_(True) for b in B]
    y = R.lora_linear(x64, w.to(F64), None, list(zip(A64, B64, s)))
    y.backward(dy.to(F64))
    got = ref.lora_linear_bwd(x, w, A, B, s, dy)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(got["dx"], x64.grad) <= 1e-12
    for i in range(len(SPECS)):
        assert rel(got["dA"][i], A64[i].grad) <= 1e-12 and rel(got["dB"][i], B64[i].grad) <= 1e-12
    # the rounding-point variant is a bf16-sized perturbation of the exact result, not something else
    assert rel(got["dx_r"], got["dx"]) <= 2.0 ** -7
    for i in range(len(SPECS)):
        assert rel(got["dA_r"][i], got["dA"][i]) <= 2.0 ** -6 and rel(got["dB_r"][i], got["dB"][i]) <= 2.0 ** -6


def test_wgrad_reference_is_the_transposed_product():
    g = torch.Generator().manual_seed(0)
    p, q = torch.randn(333, 64, generator=g).bfloat16(), torch.randn(333, 128, generator=g).bfloat16()
    c, c_r = ref.lora_wgrad(p, q, 0.5)
    want = 0.5 * torch.einsum("mr,mj->rj", p.to(F64), q.to(F64))
    assert float((c - want).norm() / want.norm()) <= 1e-12
    assert ref.err(c_r, c)[0] <= 2.0 ** -9


@pytest.mark.parametrize("slip", ["scale_twice", "scale_never", "wrong_block", "drop_second", "pad_leak"])
def test_plausible_slips_exceed_the_gpu_bounds(slip):
    """Each mistake moves the concatenated adapter gradients >= 10 x the 1e-3 rel-L2 bound and some parameter >= 10 x the 5e-3 worst-parameter
    bound. ("wrong_block" needs two adapters of one shape: ranks (8, 8) here. "pad_leak": with ranks (8, 4, 16) the third adapter receives four of
    the second's / the padding's rank columns.)"""
    x, w, A, B, s, dy = _case(333, 128, 192, seed=9)
    if slip == "wrong_block":
        A, B, s = A[:1] + [A[0].flip(0)], B[:1] + [B[0].flip(1) * 0.5], [2.0, 0.5]
    good, bad = ref.lora_linear_bwd(x, w, A, B, s, dy), ref.lora_linear_bwd(x, w, A, B, s, dy, slip=slip)
    cat = lambda d: torch.cat([t.flatten() for t in d["dA"] + d["dB"]])
    rel = lambda a, b: float((a - b).norm() / b.norm())
    worst = max(rel(b, g_) for g_, b in zip(good["dA"] + good["dB"], bad["dA"] + bad["dB"]))
    assert rel(cat(bad), cat(good)) >= 10 * 1e-3 and worst >= 10 * 5e-3, (slip, rel(cat(bad), cat(good)), worst)
