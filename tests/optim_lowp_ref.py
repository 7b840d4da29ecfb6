"""Host restatement (numpy) of the low-precision AdamW step of csrc/optim.hip: Philox4x32-10, the stochastic rounding rule and the whole step -
adamw1 in np.float32, operation by operation (the library is built with -ffp-contract=off and IEEE sqrt / division, so the fp32 values before
the rounding are reproducible here bit for bit), then the draws. The layout of the counter and of the draws is include/unigen_hip.h's.
Shared by tests/test_optim_lowp_ref_cpu.py (the reference against known answers and its own statistics) and tests/test_optim_lowp_gpu.py."""
import numpy as np

U32 = np.uint32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's Philox4x32-10 on arrays (or scalars) of counters; the key is one pair of ints. -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(U32) for c in (c0, c1, c2, c3))


def draws(seed: int, param_index: int, step: int, elements, word: int) -> np.ndarray:
    """the 16-bit draws (uint32 in [0, 65536)) of the elements with these indices inside their tensor"""
    e = np.asarray(elements, dtype=np.int64)
    j = (e >> 1).astype(np.uint64)
    w = philox4x32_10(j & MASK, j >> np.uint64(32), param_index, step, seed & 0xFFFFFFFF, seed >> 32)[word]
    return (w >> (16 * (e & 1)).astype(U32)) & U32(0xFFFF)


def sr_round(x, r) -> np.ndarray:
    """fp32 -> bf16 bits (uint16) with the draws r"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(U32)
    r = np.asarray(r, dtype=U32)
    special = (u & U32(0x7F800000)) == U32(0x7F800000)
    nan = special & ((u & U32(0x007FFFFF)) != 0)
    finite = (u.astype(np.uint64) + r.astype(np.uint64)) >> np.uint64(16)            # u + r < 2^32 for every finite u
    return np.where(nan, (u >> U32(16)) | U32(0x0040), np.where(special, u >> U32(16), finite.astype(U32))).astype(np.uint16)


def rne(x) -> np.ndarray:
    """fp32 -> bf16 bits, round to nearest even, NaN stays NaN (the library's f2bf)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(U32)
    nan = ((u & U32(0x7F800000)) == U32(0x7F800000)) & ((u & U32(0x007FFFFF)) != 0)
    rounded = (u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> U32(16)) & U32(1)).astype(np.uint64)) >> np.uint64(16)
    return np.where(nan, (u >> U32(16)) | U32(0x0040), rounded.astype(U32)).astype(np.uint16)


def widen(bits) -> np.ndarray:
    """bf16 bits -> fp32"""
    return (np.asarray(bits, dtype=np.uint16).astype(U32) << U32(16)).view(np.float32)


def hyper(lr, betas, eps, weight_decay, step: int) -> dict:
    """unigen_amd.optim._fill_group: Python floats, each rounded to fp32 once"""
    f, (b1, b2) = np.float32, betas
    return dict(decay=f(1 - lr * weight_decay), lerp_w=f(1 - b1), beta2=f(b2), one_minus_beta2=f(1 - b2), eps=f(eps), step_size=f(lr / (1 - b1 ** step)),
                inv_bc2_sqrt=f(1.0 / float(f((1 - b2 ** step) ** 0.5))))


def adamw1(p, m, v, g, h):
    """csrc/optim.hip adamw1 on np.float32 arrays: every operation rounds to fp32 once, none is contracted"""
    f = np.float32
    assert all(a.dtype == np.float32 for a in (p, m, v, g))
    p = p * h["decay"]
    d = g - m
    m = m + h["lerp_w"] * d if h["lerp_w"] < f(0.5) else g - d * (f(1.0) - h["lerp_w"])
    v = v * h["beta2"] + (h["one_minus_beta2"] * g) * g
    denom = np.sqrt(v) * h["inv_bc2_sqrt"] + h["eps"]
    p = p - h["step_size"] * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


class Tensor:
    """one parameter's state on the host. kind: 'f32' (fp32 param in place), 'master' (bf16 param, fp32 master and moments: the default),
    (False, 'bf16'), (False, 'f32'), (True, 'bf16'): the three low-precision arrangements as (master_weights, state dtype)."""

    def __init__(self, kind, p, param_index: int, seed: int = 0, step: int = 0):
        self.kind, self.index, self.seed, self.step = kind, param_index, seed, step
        if kind == "f32":
            self.p = np.array(p, dtype=np.float32).ravel()
        else:
            self.p = np.array(p, dtype=np.uint16).ravel()                  # bf16 bits
        n = self.p.size
        self.master = widen(self.p).copy() if kind in ("master", (True, "bf16")) else None
        sbf = kind in ((False, "bf16"), (True, "bf16"))
        self.m = np.zeros(n, dtype=np.uint16 if sbf else np.float32)
        self.v = np.zeros(n, dtype=np.uint16 if sbf else np.float32)

    def update(self, g, lr, betas, eps, weight_decay, coef=None):
        """g: fp32 (a bf16 grad widened); coef: the fused clip coefficient (np.float32) or None"""
        self.step += 1
        h = hyper(lr, betas, eps, weight_decay, self.step)
        g = np.ascontiguousarray(g, dtype=np.float32).ravel()
        if coef is not None:
            g = g * np.float32(coef)
        sbf = self.m.dtype == np.uint16
        p32 = self.p if self.kind == "f32" else self.master if self.master is not None else widen(self.p)
        p, m, v = adamw1(p32, widen(self.m) if sbf else self.m, widen(self.v) if sbf else self.v, g, h)
        e = np.arange(p.size, dtype=np.int64)
        d = lambda word: draws(self.seed, self.index, self.step, e, word)
        if self.kind == "f32":
            self.p = p
        elif self.master is not None:
            self.master, self.p = p, rne(p)
        else:
            self.p = sr_round(p, d(0))
        self.m, self.v = (sr_round(m, d(1)), sr_round(v, d(2))) if sbf else (m, v)
