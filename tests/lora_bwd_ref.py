"""CPU float64 references of the LoRA adapters' backward (csrc/lora_bwd.hip, autograd.Projection with adapter operands), in the manner of tests/bwd_ref.py: operands as
the kernels see them (bf16 or fp32 values widened to float64), the exact result, and a rounding-point variant (`*_r`) that rounds to bf16 where
the HIP path rounds - T and dT as matrix operands, s * B, every output. tests/test_lora_bwd_ref_cpu.py holds these to torch.autograd in float64."""
import torch

from tests.bwd_ref import F64, bf16, err  # noqa: F401  (re-exported for the tests)


def lora_wgrad(p, q, alpha=1.0):
    """ug_lora_wgrad: C [R, J] = alpha * p [M, R]^T q [M, J]. -> (exact, bf16 of the exact: the output is the kernel's only rounding point)."""
    c = alpha * (p.to(F64).t() @ q.to(F64))
    return c, bf16(c)


def lora_linear_bwd(x, w, A_list, B_list, scalings, dy, slip=None):
    """y = x w^T + sum_a s_a (x A_a^T) B_a^T with dy = d loss / d y:   dx = dy w + sum_a s_a (dy B_a) A_a,   dA_a = s_a (dy B_a)^T x,
    dB_a = s_a dy^T (x A_a^T).  Returns {"dx", "dA": [...], "dB": [...]} exact in float64 and {"dx_r", "dA_r", "dB_r"} with the HIP path's rounding
    points: B'_a = bf16(s_a B_a), T_a = bf16(x A_a^T), dT_a = bf16(dy B'_a), dx_r = bf16(dy w + sum dT_a A_a), dA_a_r = bf16(dT_a^T x),
    dB_a_r = bf16(s_a bf16(T_a^T dy)^T).
    `slip`: one of the mistakes tests/test_lora_bwd_ref_cpu.py shows the GPU bounds would catch (applied to the exact variant only):
    "scale_twice", "scale_never", "wrong_block" (dT of adapter a taken from adapter a+1's B), "drop_second" (dA of the second adapter missing),
    "pad_leak" (the fused operands stack the adapters along the rank and zero-pad to 64; the slip hands every adapter its rows of the fused
    dA_cat / columns of dB_bd from offsets counted as if each rank were padded to 8 on its own, so padded or foreign rank columns leak in)."""
    x, w, dy = x.to(F64), w.to(F64), dy.to(F64)
    out = {"dx": dy @ w, "dA": [], "dB": []}
    acc_r = dy @ w
    out.update(dA_r=[], dB_r=[])
    n = len(A_list)
    for i, (A, B, s) in enumerate(zip(A_list, B_list, scalings)):
        A, B = A.to(F64), B.to(F64)
        s_eff = {"scale_twice": s * s, "scale_never": 1.0}.get(slip, s)
        B_used = B_list[(i + 1) % n].to(F64) if slip == "wrong_block" and B_list[(i + 1) % n].shape == B.shape else B
        dT = s_eff * (dy @ B_used)
        out["dx"] = out["dx"] + dT @ A
        dA = dT.t() @ x
        if slip == "drop_second" and i == 1:
            dA = torch.zeros_like(dA)
        out["dA"].append(dA)
        out["dB"].append(s_eff * (dy.t() @ (x @ A.t())))
        Bs = bf16(s * B)
        T_r, dT_r = bf16(x @ A.t()), bf16(dy @ Bs)
        acc_r = acc_r + dT_r @ A
        out["dA_r"].append(bf16(dT_r.t() @ x))
        out["dB_r"].append(bf16(s * bf16(T_r.t() @ dy).t()))
    out["dx_r"] = bf16(acc_r)
    if slip == "pad_leak":
        pad = torch.nn.functional.pad
        ranks = [A.shape[0] for A in A_list]
        Rp = (sum(-(-r // 8) * 8 for r in ranks) + 63) // 64 * 64
        dA_cat = pad(torch.cat(out["dA"], 0), (0, 0, 0, Rp - sum(ranks)))           # the correct fused gradients ...
        dB_bd = pad(torch.cat(out["dB"], 1), (0, Rp - sum(ranks)))
        c0 = 0
        for i, r in enumerate(ranks):                                                # ... sliced at the wrong offsets
            out["dA"][i], out["dB"][i] = dA_cat[c0:c0 + r].clone(), dB_bd[:, c0:c0 + r].clone()
            c0 += -(-r // 8) * 8
    return out
