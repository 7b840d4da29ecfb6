"""float64 references, case tables and the judging functions of the step / glue / optimizer kernel sweep (tests/test_fuzz_step_gpu.py), written
from the definitions in include/unigen_hip.h and the formulas of the calls they replace - not from the kernels. No GPU is needed to import or run
this module; tests/test_step_kernel_ref_cpu.py pins every reference to torch and the oracle and shows that the judging functions reject the
plausible slips of each kernel.

Three kinds of reference:
  - ops made of +, -, x on bf16 / fp32 values (euler_step, cfg_combine, add, add_rowbcast, gate_residual, grad_scale): every step is taken in
    fp64 and rounded to the working type where the header says so. One +, - or x of two fp32 values rounded through fp64 equals the directly
    rounded result (53 >= 2 * 24 + 2), and rounding to bf16 through fp32 likewise (24 >= 2 * 8 + 2), so with a library built with
    -ffp-contract=off these references predict the kernels BIT FOR BIT, bf16 and fp32 twin alike;
  - data movement (gather_rows, pack / unpack_latents, transpose): the index formula, equality;
  - transcendental or summed ops (timestep_embed, gelu_tanh, small_linear_f32, AdamW): fp64 truth, torch's own fp32 evaluation of the same
    formula, and a per-element (per-row for the linear) bound = a margin over torch's measured error (constants below, re-measured by the CPU test).
"""
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -7.625                       # exact in bf16; every output buffer is filled with it before a call
GUARD = 64                          # sentinel elements before and after every output (a multiple of 8: 16-byte alignment survives)
EPS32 = 2.0 ** -24                  # half an fp32 ulp at 1 (unit round-off)
OK, BAD_SHAPE, BAD_ALIGN, UNSUPPORTED = 0, -1, -2, -3
CHUNK = 65536                       # UG_OPTIM_CHUNK

# ---- measured figures (docs/PARITY_TOLERANCES.md, "Step / glue / optimizer kernel sweep"). `*_TORCH`: the worst error of torch's own fp32 evaluation
# against fp64 truth on the committed cases, rounded up; the kernel's bound is the stated margin over it. test_step_kernel_ref_cpu.py re-measures each
# one and fails when torch exceeds the recorded figure or falls below half of it.
TS_C_TORCH, TS_MARGIN = 9.5, 4.0            # timestep_embed: |err| <= c * 2^-24 * max(|t f|, 1)
GELU_C_TORCH, GELU_MARGIN = 2.0, 4.0        # gelu_tanh:      |err| <= c * 2^-24 * |x|
LINEAR_ROW_TORCH, LINEAR_MARGIN = 4.5e-7, 4.0   # small_linear_f32: per-row |err|_2 / |truth|_2
ADAMW_K_TORCH, ADAMW_MARGIN = 6.5, 2.0      # AdamW: |err| <= k * 2^-23 * max(|value|, |update|) per element of p, m, v


def rnd(x64: torch.Tensor, dt) -> torch.Tensor:
    """fp64 -> the working type (through fp32: innocuous, see the module docstring) -> fp64"""
    return x64.to(F32).to(dt).to(F64)


def mags(g: torch.Generator, shape, lo=-3.0, hi=3.0) -> torch.Tensor:
    """fp32 values of either sign whose magnitudes are spread log-uniformly over [10^lo, 10^hi]"""
    e = lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)
    s = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).to(F64)
    return (s * 10.0 ** e).to(F32)


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=F32))


# ----------------------------------------------------------------------------------------------------------------------------------
# bit-exact arithmetic
# ----------------------------------------------------------------------------------------------------------------------------------
def euler_step(x, v, dt_step: float, slip=None):
    """x = rnd(float(x) + rnd(rnd(dt) * v)), dt an fp32 number (ug_euler_step; the fp32 twin rounds to fp32 only)"""
    dt = x.dtype
    d = torch.tensor(f32(dt_step), dtype=F64)
    dtr = d if slip == "dt_unrounded" else rnd(d, dt)
    p = dtr * v.to(F64)
    if slip != "product_unrounded":
        p = rnd(p, dt)
    return rnd(x.to(F64) + p, dt).to(dt)


def cfg_combine(u, t, gs: float, slip=None):
    """out = rnd(u + rnd(gs * rnd(t - u))), gs an fp32 number (ug_cfg_combine)"""
    dt = u.dtype
    d = t.to(F64) - u.to(F64)
    if slip != "difference_unrounded":
        d = rnd(d, dt)
    p = f32(gs) * d
    if slip != "product_unrounded":
        p = rnd(p, dt)
    return rnd(u.to(F64) + p, dt).to(dt)


def add(a, b):
    return rnd(a.to(F64) + b.to(F64), a.dtype).to(a.dtype)


def add_rowbcast(x, table, rpb: int, slip=None):
    """x[r] = rnd(float(x[r]) + table[r % rpb]), table fp32 (ug_add_rowbcast_f32)"""
    r = torch.arange(x.shape[0])
    rows = r.clamp_max(table.shape[0] - 1) if slip == "row_not_wrapped" else r % rpb
    return rnd(x.to(F64) + table.to(F64)[rows], x.dtype).to(x.dtype)


def gate_residual(x, a, gate, rps: int, slip=None):
    """y[r] = (x ? x[r] : 0) + rnd(gate[r / rps] * a[r]) (ug_gate_residual)"""
    dt = a.dtype
    r = torch.arange(a.shape[0])
    rows = (r % gate.shape[0]) if slip == "sample_is_remainder" else r // rps
    p = gate.to(F64)[rows] * a.to(F64)
    if slip != "product_unrounded":
        p = rnd(p, dt)
    return (p if x is None else rnd(x.to(F64) + p, dt)).to(dt)


def grad_scale(g, coef32: float):
    """g = rnd(g * coef), coef an fp32 number (ug_grad_scale)"""
    return rnd(g.to(F64) * f32(coef32), g.dtype).to(g.dtype)


# ----------------------------------------------------------------------------------------------------------------------------------
# data movement
# ----------------------------------------------------------------------------------------------------------------------------------
def gather_rows(src, idx, slip=None):
    """out[i] = src[idx[i]], zeros where idx[i] < 0 (ug_gather_rows)"""
    out = src[idx.clamp_min(0).long()].clone()
    if slip != "negative_reads_row_0":
        out[idx < 0] = 0
    return out


def pack_index(B, C, H, W, slip=None):
    """flat index into latents [B][C][H][W] of every element of packed [B][(H/2)(W/2)][4C]: column c*4 + dy*2 + dx of token (i, j) is pixel
    (2i + dy, 2j + dx) of channel c (ug_pack_latents)"""
    b, i, j, c, dy, dx = torch.meshgrid(torch.arange(B), torch.arange(H // 2), torch.arange(W // 2), torch.arange(C), torch.arange(2), torch.arange(2),
                                        indexing="ij")
    if slip == "dy_dx_swapped":
        dy, dx = dx, dy
    return ((((b * C + c) * H + 2 * i + dy) * W) + 2 * j + dx).reshape(B, (H // 2) * (W // 2), 4 * C)


def pack_latents(lat, slip=None):
    B, C, H, W = lat.shape
    return lat.reshape(-1)[pack_index(B, C, H, W, slip)]


def unpack_latents(packed, H, W, slip=None):
    B, _, c4 = packed.shape
    out = torch.empty(B * (c4 // 4) * H * W, dtype=packed.dtype)
    out[pack_index(B, c4 // 4, H, W, slip).reshape(-1)] = packed.reshape(-1)
    return out.reshape(B, c4 // 4, H, W)


def transpose(src, rows_pad: int, fill=0.0):
    """dst[b][c][r] = src[b][r][c], dst[b][c][rows .. rows_pad) = 0 (ug_transpose); src [batch, rows, cols]"""
    batch, rows, cols = src.shape
    out = torch.full((batch, cols, rows_pad), fill, dtype=src.dtype)
    out[:, :, :rows] = src.transpose(1, 2)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# timestep embedding, GELU, small linear
# ----------------------------------------------------------------------------------------------------------------------------------
def timestep_embed64(t32, dim: int):
    """-> (truth fp64 [B, dim] = [cos | sin] of a = t * exp(-ln(1e4) k / half), |a| tiled to [B, dim])"""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)
    a = t32.to(F64)[:, None] * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], 1), torch.cat([a, a], 1).abs()


def timestep_embed_torch32(t32, dim: int):
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half)
    a = t32[:, None] * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], 1)


def bf16_half_ulp(truth64):
    """half a bf16 ulp at the magnitude of each value (the rounding of a bf16 output)"""
    e = torch.floor(torch.log2(truth64.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 8)


def timestep_bound(a_abs, truth64, dt, c=None):
    c = TS_MARGIN * TS_C_TORCH if c is None else c
    b = c * EPS32 * a_abs.clamp_min(1.0)
    return b + bf16_half_ulp(truth64) if dt == BF else b


def gelu64(x):
    """tanh GELU 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), in its equal form x / (1 + exp(-2u)) that keeps the negative tail"""
    x = x.to(F64)
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x / (1.0 + torch.exp(-2.0 * u))


def gelu_torch32(x32):
    return torch.nn.functional.gelu(x32, approximate="tanh")


def gelu_bound(x, truth64, dt, c=None):
    """torch's fp32 tanh form computes the factor 0.5 (1 + tanh u) in [0, 1] with an ABSOLUTE error of a few 2^-24, so the error of x * factor scales
    with |x|, not with the (possibly tiny) result: the bound is c 2^-24 |x| (+ half a bf16 ulp of the truth for a bf16 output)."""
    c = GELU_MARGIN * GELU_C_TORCH if c is None else c
    b = c * EPS32 * x.to(F64).abs()
    return b + bf16_half_ulp(truth64) if dt == BF else b


def small_linear64(x, W, b, res, silu: bool):
    x = x.to(F64)
    if silu:
        x = x / (1.0 + torch.exp(-x))
    y = x @ W.to(F64).t()
    if b is not None:
        y = y + b.to(F64)
    return y if res is None else y + res.to(F64)


def small_linear_torch32(x, W, b, res, silu: bool):
    y = torch.nn.functional.linear(torch.nn.functional.silu(x) if silu else x, W, b)
    return y if res is None else y + res


def row_rel(got64, truth64):
    return (got64 - truth64).norm(dim=-1) / truth64.norm(dim=-1).clamp_min(1e-300)


# ----------------------------------------------------------------------------------------------------------------------------------
# AdamW and clipping
# ----------------------------------------------------------------------------------------------------------------------------------
class AdamWRef64:
    """fp64 restatement of torch.optim.AdamW's recurrence (decoupled weight decay). lr, wd, betas, eps: one value, or a list with one per tensor.
    After a step, scale_p / scale_m / scale_v hold max(|value|, |update|) per element (the scale of adamw_bound)."""

    def __init__(self, params):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.t = 0
        self.scale_p, self.scale_m, self.scale_v = [], [], []

    def step(self, grads, lr, wd, betas=(0.9, 0.999), eps=1e-8, slip=None):
        self.t += 1
        tb = max(self.t - 1, 1) if slip == "bias_correction_of_previous_step" else self.t
        self.scale_p, self.scale_m, self.scale_v = [], [], []
        for i in range(len(self.p)):
            g = grads[i].double()
            lr_i, wd_i = (lr[i], wd[i]) if isinstance(lr, list) else (lr, wd)
            b1, b2 = betas[i] if isinstance(betas, list) else betas
            eps_i = eps[i] if isinstance(eps, list) else eps
            self.p[i] *= 1 - lr_i * wd_i
            dm = (1 - b1) * (g - self.m[i])
            if slip == "lerp_swapped":                # lerp(grad, exp_avg, w) for lerp(exp_avg, grad, w)
                dm = (g - self.m[i]) - dm
            self.m[i] += dm
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            denom = self.v[i].sqrt() / (1 - b2 ** tb) ** 0.5 + eps_i
            step_size = lr_i / (1 - b1 ** tb)
            self.p[i] -= step_size * self.m[i] / denom
            sm = torch.maximum(self.m[i].abs(), dm.abs())
            self.scale_m.append(sm)
            self.scale_v.append(torch.maximum(self.v[i], (1 - b2) * g * g))
            self.scale_p.append(torch.maximum(self.p[i].abs(), step_size * sm / denom))


def adamw_bound(scale64, k=None):
    """k fp32 epsilons of max(|value|, |update|): the update term keeps the bound meaningful where the new value cancels"""
    k = ADAMW_MARGIN * ADAMW_K_TORCH if k is None else k
    return k * 2.0 ** -23 * scale64


def adamw_hparams(lr, wd, betas, eps, t):
    """struct ug_adamw_group as the header defines it: each value computed in fp64 and rounded to fp32 once; inv_bc2_sqrt = 1 / fp32(sqrt(1 - beta2^t))
    taken in fp32"""
    b1, b2 = betas
    bc2 = torch.tensor((1 - b2 ** t) ** 0.5, dtype=F32)
    return dict(decay=1 - lr * wd, lerp_w=1 - b1, beta2=b2, one_minus_beta2=1 - b2, eps=eps, step_size=lr / (1 - b1 ** t), inv_bc2_sqrt=float(1.0 / bc2))


def clip_coef64(total_norm: float, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)"""
    return min(1.0, max_norm / (total_norm + 1e-6))


def clip_coef32(norm32: torch.Tensor, max_norm: float) -> torch.Tensor:
    """the same in torch's fp32 tensor arithmetic (Tensor.__rdiv__: reciprocal, then the product), given the fp32 norm"""
    return torch.clamp((norm32.to(F32) + 1e-6).reciprocal() * max_norm, max=1.0)


def body_start(offsets, esizes, n: int) -> int:
    """first element h in [0, 8) at which every stream (element offset into a 16-byte aligned buffer, element size) is 16-byte aligned, or n: the
    header promises vector accesses on the aligned body of a chunk and scalar head / tail. A chunk start (a multiple of 65536 elements) keeps
    every stream's alignment, so h is the same in every chunk of a tensor."""
    for h in range(8):
        if all(((o + h) * e) % 16 == 0 for o, e in zip(offsets, esizes)):
            return min(h, n)
    return n


def regions(n: int, h: int) -> torch.Tensor:
    """int8 [n]: 0 head, 1 body, 2 tail of each chunk of a tensor whose chunks start their vector body at element h"""
    out = torch.empty(n, dtype=torch.int8)
    for c0 in range(0, n, CHUNK):
        m = min(CHUNK, n - c0)
        hh = min(h, m)
        body_end = hh + (m - hh) // 8 * 8
        r = out[c0:c0 + m]
        r[:hh], r[hh:body_end], r[body_end:] = 0, 1, 2
    return out


REGION_NAMES = ("head", "body", "tail")

# ----------------------------------------------------------------------------------------------------------------------------------
# judging: what the GPU sweep asserts. `image`: the whole output buffer, sentinels included; `inside`: bool mask of the elements the op owns.
# ----------------------------------------------------------------------------------------------------------------------------------
def guarded(shape_rows: int, D: int, ld: int, dt, fill=SENT):
    """-> (flat buffer of sentinels, its [rows, D] view with leading dimension ld, bool mask of the view's elements)"""
    n = shape_rows * ld
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dt)
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[GUARD:GUARD + n].view(shape_rows, ld)[:, :D] = True
    return buf, buf[GUARD:GUARD + n].view(shape_rows, ld)[:, :D], mask


def judge_guards(name, image, inside):
    out = image[~inside]
    bad = int((out != SENT).sum())
    assert bad == 0, (f"{name}: {bad} element(s) outside the output were written", torch.nonzero((image != SENT) & ~inside)[:4].flatten().tolist())


def judge_exact(name, image, want_image, inside):
    """bit equality of the op's elements and untouched sentinels everywhere else"""
    judge_guards(name, image, inside)
    a, b = image[inside], want_image[inside]
    same = a == b                                     # torch.equal's comparison, kept per element so that a failure can name its first elements
    bad = int((~same).sum())
    first = torch.nonzero(~same)[:4].flatten().tolist()
    assert bad == 0, (f"{name}: {bad} of {a.numel()} elements differ from the reference", first, a[~same][:4].tolist(), b[~same][:4].tolist())


def judge_bounded(name, image, truth64, bound64, inside, region=None):
    """|got - truth| <= bound per element (truth, bound: the shape of image[inside]); -> the worst |err| / bound, per region when given"""
    judge_guards(name, image, inside)
    got = image[inside].to(F64)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    ratio = (got - truth64.reshape(-1)).abs() / bound64.reshape(-1).clamp_min(1e-300)
    ratio = torch.where((got == truth64.reshape(-1)), torch.zeros_like(ratio), ratio)
    worst = {}
    if region is None:
        worst["all"] = float(ratio.max()) if ratio.numel() else 0.0
    else:
        for k, nm in enumerate(REGION_NAMES):
            sel = ratio[region.reshape(-1) == k]
            worst[nm] = float(sel.max()) if sel.numel() else 0.0
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (f"{name}: error over the bound (|err| / bound by region)", bad, torch.nonzero(ratio > 1.0)[:4].flatten().tolist())
    return worst


def judge_rows(name, got64, truth64, bound: float):
    e = row_rel(got64, truth64)
    worst = float(e.max())
    assert worst <= bound, (f"{name}: row {int(e.argmax())} has relative error {worst:.3e} > {bound:.3e}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# case tables (the test ids and the CPU test see the same cases)
# ----------------------------------------------------------------------------------------------------------------------------------
GRID_ELEMS = 2048 * 256 * 8          # elements one pass of the euler / cfg / add / rowbcast launch covers (grid capped at 2048 blocks of 256 x 8)
FLAT_N = [8, 16, 4088, 4096, 4104, 257 * 4096 + 8, GRID_ELEMS + 4104]
EULER_DT = [-0.25, 0.9741077 - 0.9873806, -0.0132729, -0.0357, 0.0]          # FLUX-schnell's step; SD3's shifted 28-step schedule; no step
CFG_GS = [0.0, 1.0, 3.5, 7.0, -1.0]
GELU_N = FLAT_N[:6] + [7, 4099, 65537]                    # n % 8 != 0: the element-wise kernel
FLAT_REFUSED = [dict(n=12, off=0, code=BAD_ALIGN), dict(n=4100, off=0, code=BAD_ALIGN), dict(n=16, off=1, code=BAD_ALIGN), dict(n=4096, off=4, code=BAD_ALIGN)]


def flat_cases(kind):
    """kind: euler | cfg | gelu -> list of dict(id, n, seed, off (element offset of the bases: gelu only), param)"""
    out = []
    ns = GELU_N if kind == "gelu" else FLAT_N
    for i, n in enumerate(ns):
        c = dict(n=n, seed=i, off=0)
        if kind == "euler":
            c["dt"] = EULER_DT[i % len(EULER_DT)]
        if kind == "cfg":
            c["gs"] = CFG_GS[i % len(CFG_GS)]
        out.append(c)
    if kind == "euler":
        out += [dict(n=4104, seed=20 + j, off=0, dt=d) for j, d in enumerate(EULER_DT)]
    if kind == "cfg":
        out += [dict(n=4104, seed=20 + j, off=0, gs=s) for j, s in enumerate(CFG_GS)]
    if kind == "gelu":
        out += [dict(n=4096, seed=30, off=1), dict(n=4099, seed=31, off=1)]            # a base one element off 16 bytes: the element-wise kernel
    for c in out:
        c["id"] = f"n{c['n']}" + (f"-off{c['off']}" if c["off"] else "") + (f"-dt{c['dt']:.4g}" if "dt" in c else "") + (f"-gs{c['gs']:g}" if "gs" in c else "")
    return out


def flat_data(c, dt, big=False):
    """two operands with magnitudes over 1e-3 .. 1e3 (gelu: part of them up to +-30, where exp / rcp saturate)"""
    g = torch.Generator().manual_seed(1000 + c["seed"])
    a, b = mags(g, (c["n"],)).to(dt), mags(g, (c["n"],)).to(dt)
    if big:
        k = c["n"] // 2
        a[:k] = (60.0 * torch.rand(k, generator=g) - 30.0).to(dt)
    return a, b


def flat_check(n: int, off: int, esize: int) -> int:
    """ug_euler_step / ug_cfg_combine: n a multiple of 8 and 16-byte aligned bases, or UG_ERR_BAD_ALIGN"""
    return OK if n % 8 == 0 and (off * esize) % 16 == 0 else BAD_ALIGN


ROWS, DS, LD_EXTRA = [1, 7, 333, 4099], [8, 64, 200, 1536, 3072], [0, 8, 64]
ROW_SHAPES = [(1, 8), (7, 64), (333, 200), (4099, 1536), (333, 3072), (7, 1536), (1, 3072), (4099, 8), (333, 64), (7, 200), (4099, 64), (1, 200), (333, 8)]


def _rpb_choices(rows):
    div = {1: 1, 7: 1, 333: 37, 4099: 1}[rows]
    return [1, rows, div, {1: 3, 7: 3, 333: 100, 4099: 1000}[rows]]            # 1, all rows, a proper divisor (1 where rows is prime), a non-divisor


def row_cases(kind):
    """kind: add | rowbcast | gather | gate -> list of dict(id, rows, D, ld_* (each D, D + 8 or D + 64, drawn independently), ...)"""
    out = []
    shapes = ROW_SHAPES + ([(4099, 3072)] if kind == "gather" else [])            # gather's launch covers 4096 x 256 x 8 elements: this one takes two passes
    for i, (rows, D) in enumerate(shapes):
        g = torch.Generator().manual_seed(7000 + i + 100 * len(kind))
        ld = lambda: D + LD_EXTRA[int(torch.randint(0, 3, (1,), generator=g))]
        c = dict(rows=rows, D=D, seed=i, ld_a=ld(), ld_b=ld(), ld_o=ld(), ld_x=ld())
        if i == 2:
            c.update(ld_a=D + 8, ld_b=D + 64, ld_o=D)            # all three different at least once
        if kind == "rowbcast":
            c["rpb"] = _rpb_choices(rows)[i % 4]
        if kind == "gate":
            c["rps"] = _rpb_choices(rows)[(i + 2) % 4]
            c["x"] = ("none", "given", "alias")[i % 3]
        if kind == "gather":
            c["src_rows"] = max(1, rows // 3 + 2)
            c["idx"] = ("mixed", "all_negative", "duplicates", "last_row")[i % 4]
        c["id"] = f"{rows}x{D}-" + "-".join(f"{k}{v}" for k, v in c.items() if k in ("ld_a", "ld_b", "ld_o", "ld_x", "rpb", "rps", "x", "idx"))
        out.append(c)
    return out


def gather_idx(c, g):
    n, s = c["rows"], c["src_rows"]
    if c["idx"] == "all_negative":
        return torch.full((n,), -1, dtype=torch.int32) - torch.randint(0, 3, (n,), generator=g).to(torch.int32)
    if c["idx"] == "duplicates":
        return torch.full((n,), s // 2, dtype=torch.int32)
    if c["idx"] == "last_row":
        return torch.full((n,), s - 1, dtype=torch.int32)
    idx = torch.randint(-2, s, (n,), generator=g).to(torch.int32)
    idx[-1] = s - 1
    return idx


def row_check(D, lds, offs=(), esize=2) -> int:
    """the 16-byte row ops: D and every leading dimension a multiple of 8, bases 16-byte aligned, or UG_ERR_BAD_ALIGN"""
    return OK if D % 8 == 0 and all(l % 8 == 0 for l in lds) and all((o * esize) % 16 == 0 for o in offs) else BAD_ALIGN


ROW_REFUSED = [dict(rows=3, D=12, ld=16, off=0), dict(rows=3, D=16, ld=20, off=0), dict(rows=3, D=16, ld=16, off=4), dict(rows=3, D=16, ld=16, off=1)]

PACK_CASES = [(1, 1, 2, 2), (2, 16, 128, 128), (3, 16, 6, 10), (2, 1, 8, 4), (1, 4, 2, 2), (5, 3, 34, 2), (4, 16, 128, 136), (1, 16, 2, 64)]
PACK_REFUSED = [(1, 4, 3, 4), (1, 4, 4, 5), (2, 1, 1, 2)]


def pack_check(B, C, H, W) -> int:
    return OK if min(B, C, H, W) > 0 and H % 2 == 0 and W % 2 == 0 else BAD_SHAPE


# (batch, rows, cols, rows_pad, ld_src extra, ld_dst extra, batch-stride extra (elements beyond one matrix, source and destination))
TRANSPOSE_CASES = [
    (1, 300, 192, 304, 0, 0, 0), (1, 64, 64, 64, 0, 0, 0), (3, 1000, 72, 1024, 0, 0, 0), (1, 257, 130, 260, 0, 0, 0), (2, 130, 256, 136, 64, 0, 0),
    (1, 4608, 3072, 4608, 0, 0, 0), (1, 77, 8, 80, 8, 0, 0),                                                  # the seven shapes of test_backward_gpu.py
    (1, 200, 8, 200, 0, 0, 0), (2, 199, 72, 200, 0, 8, 72), (1, 193, 130, 200, 0, 0, 0), (3, 192, 72, 200, 8, 16, 1000), (1, 65, 8, 128, 0, 0, 0),
    (2, 1, 130, 64, 3, 5, 7), (1, 120, 72, 127, 0, 0, 0), (2, 57, 8, 64, 0, 8, 8), (1, 1025, 136, 1088, 0, 0, 0),
]


def transpose_check(rows, cols, rows_pad, ld_src, ld_dst) -> int:
    return OK if rows > 0 and cols > 0 and rows_pad >= rows and ld_src >= cols and ld_dst >= rows_pad else BAD_SHAPE


TS_T = [0.0, 1e-3, 1.0, 250.5, 999.0, 1000.0]
TS_CASES = [dict(B=B, dim=dim, slack=s, id=f"B{B}-dim{dim}-ld+{s}") for B, dim, s in
            [(1, 2, 0), (5, 64, 0), (64, 256, 0), (1, 320, 8), (5, 1024, 3), (64, 2, 1), (5, 256, 64), (64, 320, 0), (1, 1024, 0), (64, 64, 5)]]


# The guidance embedders feed the same kernel with `guidance.to(bf16) * 1000` (in bf16): 1000, 3504, 7008, 29952 for scales 1, 3.5, 7, 30 - arguments up
# to 30 x the largest timestep. dim = 256 (the embedders' width), B in {1, 5}. torch's own fp32 constant on these cases is 9.06 (re-measured by
# tests/test_step_kernel_ref_cpu.py), within TS_C_TORCH: the bound of TS_CASES holds here unchanged, scaled by the larger |t f|.
TS_GUIDANCE = [1.0, 3.5, 7.0, 30.0]
TS_GUIDANCE_CASES = [dict(B=B, dim=256, slack=s, guidance=True, id=f"guidance-B{B}-dim256-ld+{s}") for B, s in [(1, 0), (5, 0), (5, 8)]]


def ts_guidance_times(B: int):
    """float(bf16(g) * 1000 in bf16) for g in TS_GUIDANCE, cycled to B entries and starting at the largest for B = 1"""
    t = (torch.tensor(TS_GUIDANCE, dtype=BF) * 1000).to(F32)
    return t.flip(0).repeat(-(-B // len(TS_GUIDANCE)))[:B].contiguous()


def ts_times(c):
    if c.get("guidance"):
        return ts_guidance_times(c["B"])
    g = torch.Generator().manual_seed(c["B"] * 7 + c["dim"])
    t = torch.tensor((TS_T * 11)[:c["B"]], dtype=F32)
    if c["B"] > len(TS_T):
        t[len(TS_T):] = 1000.0 * torch.rand(c["B"] - len(TS_T), generator=g)
    return t


# (M, N, K, ldx extra, ldw extra, ldo extra, bias, residual, silu)
LINEAR_CASES = [(1, 7, 8, 0, 0, 0, True, False, False), (5, 130, 100, 4, 0, 3, True, True, True), (16, 256, 1536, 0, 8, 0, True, False, True),
                (64, 33, 3072, 0, 0, 7, False, True, False), (2, 1536, 256, 0, 0, 0, True, False, True), (3, 4, 259, 1, 1, 1, False, False, True),
                (64, 9, 64, 0, 0, 0, True, True, True), (1, 1, 3072, 0, 0, 0, True, False, False)]


def linear_data(c):
    M, N, K, ex, ew, eo, bias, res, silu = c
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    x = torch.randn(M, K + ex, generator=g)[:, :K]
    W = (torch.randn(N, K + ew, generator=g) * K ** -0.5)[:, :K]
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    R = torch.randn(M, N, generator=g) if res else None
    return x, W, b, R


# ---- optimizer ----------------------------------------------------------------------------------------------------------------------
OPT_NUMEL = [0, 1, 7, 8, 9, 65535, 65536, 65537, 2 * 65536 + 13]
OPT_FORMS = [(True, True), (True, False), (False, True), (False, False)]           # (GBF: bf16 grads, MASTER: bf16 param + fp32 master)
OPT_GROUPS = [dict(lr=1e-3, wd=0.05, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-3, wd=0.0, betas=(0.3, 0.95), eps=1e-6)]      # lerp_w 0.1 and 0.7
OPT_MODES = ["aligned", "h1", "h3", "h4", "h7", "random", "odd_param"]
OPT_CLIP = ["fused", "unfused", "none"]
OPT_MAX_NORM = 1.0
STREAMS = ("grad", "param", "master", "exp_avg", "exp_avg_sq")


def opt_esizes(gbf, master):
    """element size of each stream the AdamW kernel walks: grad, fp32 master-or-param, exp_avg, exp_avg_sq, and the bf16 param of a master form"""
    return [2 if gbf else 4, 4, 4, 4] + ([2] if master else [])


def optim_case(mode: str):
    """-> list of tensors dict(n, gbf, master, group, off = element offset of each stream into its own 16-byte aligned buffer, h = body_start of the
    AdamW pass, h_grad = body_start of the gradient-only passes). Modes: every offset 0; offsets that meet at a common aligned element h = 1, 3, 4, 7;
    offsets drawn independently from 0..8 (mostly no common element: scalar chunks); a param one element off with everything else aligned
    (no common aligned element exists: the whole chunk goes scalar)."""
    g = torch.Generator().manual_seed(OPT_MODES.index(mode))
    out = []
    for fi, (gbf, master) in enumerate(OPT_FORMS):
        for ni, n in enumerate(OPT_NUMEL):
            unit = dict(grad=8 if gbf else 4, param=8 if master else 4, master=4, exp_avg=4, exp_avg_sq=4)
            if mode == "aligned":
                off = {s: 0 for s in STREAMS}
            elif mode[0] == "h":
                h = int(mode[1:])
                off = {s: (-h) % unit[s] + unit[s] * int(torch.randint(0, 2, (1,), generator=g)) for s in STREAMS}
                off = {s: o if o <= 8 else o - unit[s] for s, o in off.items()}
            elif mode == "random":
                off = {s: int(torch.randint(0, 9, (1,), generator=g)) for s in STREAMS}
            else:
                off = {s: 0 for s in STREAMS}
                off["param"] = 1
            walked = [off["grad"], off["master"] if master else off["param"], off["exp_avg"], off["exp_avg_sq"]] + ([off["param"]] if master else [])
            out.append(dict(n=n, gbf=gbf, master=master, group=(fi + ni) % 2, off=off, h=body_start(walked, opt_esizes(gbf, master), min(n, CHUNK)),
                            h_grad=body_start([off["grad"]], [2 if gbf else 4], min(n, CHUNK))))
    return out


def optim_data(case, seed, steps=2):
    """-> (p0: fp32 start values (bf16-representable for a master form: the master starts as float(param)), grads[step][tensor] in the grad dtype)"""
    g = torch.Generator().manual_seed(9000 + seed)
    p0, grads = [], [[] for _ in range(steps)]
    for t in case:
        p = torch.randn(t["n"], generator=g) * 0.5
        p0.append(p.to(BF).to(F32) if t["master"] else p)
        for s in range(steps):
            grads[s].append((torch.randn(t["n"], generator=g) * 0.05).to(BF if t["gbf"] else F32))
    return p0, grads


def optim_hyper(case):
    gr = [OPT_GROUPS[t["group"]] for t in case]
    return [x["lr"] for x in gr], [x["wd"] for x in gr], [x["betas"] for x in gr], [x["eps"] for x in gr]
