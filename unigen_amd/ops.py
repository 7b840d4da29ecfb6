"""Thin torch-tensor front end over the C ABI (unigen_amd/lib.py).

torch is used only for device memory and the current HIP stream; every computation below runs in libunigen_hip.so.
All tensors must be bf16 CUDA(HIP) tensors with a contiguous last dimension unless stated otherwise.

fp32 verification mode: when the activation tensors are torch.float32 the SAME call goes to the entry point's `_f32` twin
(include/unigen_hip.h, last section) - fp32 storage, no intermediate rounding - so a model whose parameters are fp32 runs the
identical host orchestration in exact arithmetic. Mixed dtypes in one call are an error.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import lib as L

bf16 = torch.bfloat16


class KernelTimer:
    """Optional per-launch timing for bench.py: HIP events recorded on the launch stream around each call of the named
    kernel classes, with the algorithmic FLOPs of the launch. Off unless installed with `set_timer`."""

    def __init__(self, kinds=("gemm", "attn")):
        self.kinds = set(kinds)
        self.records = []   # (kind, flops, start_event, end_event)
        self.tags = []      # per record: the launch's shape, e.g. (M, N, K, groups) of a GEMM (tools/shape_rates.py)

    def begin(self, kind):
        if kind not in self.kinds:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def end(self, kind, flops, ev0, tag=None):
        if ev0 is None:
            return
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream())
        self.records.append((kind, flops, ev0, ev1))
        self.tags.append(tag)

    def summary(self):
        """-> {kind: dict(launches, flops, ms)} (call after a device synchronize)."""
        out = {}
        for kind, flops, e0, e1 in self.records:
            d = out.setdefault(kind, dict(launches=0, flops=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += e0.elapsed_time(e1)
        return out


_timer: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]) -> None:
    global _timer
    _timer = t


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


f32 = torch.float32


def _chk(t: torch.Tensor, name: str, dtype=bf16) -> None:
    if not t.is_cuda:
        raise L.UniGenHipError(f"{name}: expected a GPU tensor (unigen_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")


def _act(t: torch.Tensor, name: str):
    """Activation dtype of a call, taken from its first tensor: bf16 (product path) or fp32 (verification twins)."""
    if t.dtype not in (bf16, f32):
        raise TypeError(f"{name}: expected torch.bfloat16 (or torch.float32 for the verification path), got {t.dtype}")
    return t.dtype


def _fn(base: str, dt):
    """The C-ABI function for activation dtype `dt`: `base` itself for bf16, its `_f32` twin otherwise."""
    return getattr(L.load(), base if dt == bf16 else L.F32_TWIN_OF[base])


def _call(base: str, dt, *args) -> None:
    """Call `base` (bf16) or its `_f32` twin (any other dtype); a failure raises under the name of the symbol that was called."""
    name = base if dt == bf16 else L.F32_TWIN_OF[base]
    rc = getattr(L.load(), name)(*args)         # not through L.call: one Python frame per launch matters to the launch-bound batch-1 forwards
    if rc:
        L.check(rc, name)


class RowMap:
    """Logical row m -> physical row (m // rows_per_batch) * batch_stride + m % rows_per_batch (0 = identity)."""

    __slots__ = ("rpb", "bstride")

    def __init__(self, rows_per_batch: int = 0, batch_stride: int = 0):
        self.rpb, self.bstride = rows_per_batch, batch_stride


IDENT = RowMap()


class QkRope:
    """Operands of the UG_EPI_QKV_ROPE epilogue: RMSNorm weights of the q / k heads [128], the (cos, sin) pair table [positions, 64, 2]
    fp32, and the position of output row m = pos0 + m % rows_per_batch. Columns [0, until_n) of the projection are q | k heads."""

    __slots__ = ("wq", "wk", "cs", "rpb", "pos0", "until_n", "eps", "dh")

    def __init__(self, wq, wk, cs, rows_per_batch: int, pos0: int, until_n: int, eps: float = 1e-6, dh: int = 128):
        self.wq, self.wk, self.cs, self.rpb, self.pos0, self.until_n, self.eps, self.dh = wq, wk, cs, rows_per_batch, pos0, until_n, eps, dh


def qk_rope_fusable(M: int, N: int, until_n: int, dh: int, dtype: torch.dtype, *, c_rpb: int = 0, rope_rpb: int = 0) -> bool:
    """Whether ug_gemm_bf16 can take q/k RMSNorm + RoPE in its epilogue for this projection: bf16, heads of 64 or 128, whole 256^2 tiles, and
    at least one full round of them (below that the dispatcher prefers the 128^2 kernel, which has no such epilogue). c_rpb / rope_rpb are the
    rows per batch of the launch's C row map and of its positions (0, the default: identity map, position = row): the epilogue needs the
    former a multiple of 256 (one scalar row map per tile) and the latter 0 or >= 256 (at most one position wrap per 16-row group) -
    gemm_check refuses anything else.
    UG_GEMM_FUSE_QKROPE=0 keeps the stand-alone ug_qk_rmsnorm_rope pass (A/B measurements)."""
    if os.environ.get("UG_GEMM_FUSE_QKROPE", "1") == "0":
        return False
    return (dtype == torch.bfloat16 and dh in (64, 128) and M % 256 == 0 and N % 256 == 0 and until_n % 256 == 0 and (M // 256) * (N // 256) >= 256
            and c_rpb % 256 == 0 and (rope_rpb == 0 or rope_rpb >= 256))


_gemm_ws: dict = {}


def _gemm_workspace(device, stream: int) -> torch.Tensor:
    """Caller-owned scratch for the GEMM's split-K tail: one per (device, stream), allocated once - launches on one stream are ordered, two
    streams must not share arrival tickets or slabs (include/unigen_hip.h: "One workspace per stream")."""
    key = (device, stream)
    ws = _gemm_ws.get(key)
    if ws is None:
        ws = torch.zeros(int(L.load().ug_gemm_workspace_bytes()), dtype=torch.uint8, device=device)   # tickets start at zero
        _gemm_ws[key] = ws
    return ws


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, M: int,
         epilogue: int = L.EPI_BIAS, lda: Optional[int] = None, ldc: Optional[int] = None, a_map: RowMap = IDENT,
         c_map: RowMap = IDENT, residual: Optional[torch.Tensor] = None, ldr: Optional[int] = None,
         r_map: RowMap = IDENT, gate: Optional[torch.Tensor] = None, gate_ld: int = 0, rows_per_sample: int = 0,
         alpha: float = 1.0, groups: int = 1, a_gstride: int = 0, w_gstride: int = 0, bias_gstride: int = 0,
         c_gstride: int = 0, r_gstride: int = 0, gate_gstride: int = 0, lora_t: Optional[torch.Tensor] = None,
         lora_b: Optional[torch.Tensor] = None, gelu_from_n: int = 0, c_shift_from_n: int = 0, c_shift: int = 0,
         qk_rope: Optional[QkRope] = None) -> torch.Tensor:
    """out[m, :N] = epilogue(a[m, :K] @ w[:N, :K]^T + bias). `a`/`out`/`residual` are base tensors whose data_ptr is row 0
    (slices of a bigger buffer are fine); leading dims default to the tensors' row strides. `qk_rope` selects UG_EPI_QKV_ROPE
    (with gelu_from_n > 0 the columns from there on still get GELU)."""
    dt = _act(a, "a")
    if qk_rope is not None:
        if dt != torch.bfloat16:
            raise ValueError("the fused q/k RMSNorm + RoPE epilogue is bf16 only")
        epilogue = L.EPI_QKV_ROPE
    _chk(w, "w", dt)
    _chk(out, "out", torch.float32 if epilogue == L.EPI_F32 else dt)
    if bias is not None:
        _chk(bias, "bias", dt)
    N, K = (w.shape[-2], w.shape[-1])
    d = L.GemmDesc()
    d.A, d.lda, d.a_rpb, d.a_bstride = a.data_ptr(), (lda if lda is not None else a.stride(-2)), a_map.rpb, a_map.bstride
    d.W, d.ldw = w.data_ptr(), w.stride(-2)
    d.bias = _p(bias)
    d.C, d.ldc, d.c_rpb, d.c_bstride = out.data_ptr(), (ldc if ldc is not None else out.stride(-2)), c_map.rpb, c_map.bstride
    if residual is not None:
        _chk(residual, "residual", dt)
        d.R, d.ldr, d.r_rpb, d.r_bstride = residual.data_ptr(), (ldr if ldr is not None else residual.stride(-2)), r_map.rpb, r_map.bstride
    if gate is not None:
        _chk(gate, "gate", dt)
        d.gate, d.gate_ld, d.rows_per_sample = gate.data_ptr(), gate_ld, rows_per_sample
    d.alpha, d.epilogue = alpha, epilogue
    d.M, d.N, d.K = M, N, K
    d.groups, d.a_gstride, d.w_gstride, d.bias_gstride, d.c_gstride = groups, a_gstride, w_gstride, bias_gstride, c_gstride
    d.r_gstride, d.gate_gstride = r_gstride, gate_gstride
    d.gelu_from_n, d.c_shift_from_n, d.c_shift = gelu_from_n, c_shift_from_n, c_shift
    if qk_rope is not None:
        q = qk_rope
        _chk(q.wq, "qk_rope.wq", dt); _chk(q.wk, "qk_rope.wk", dt)
        if q.wq.numel() != q.dh or q.wk.numel() != q.dh:
            raise ValueError(f"qk_rope: weights must be [{q.dh}]")
        if q.cs is not None:
            _chk(q.cs, "qk_rope.cs", torch.float32)
            if q.cs.dim() != 3 or tuple(q.cs.shape[1:]) != (q.dh // 2, 2) or not q.cs.is_contiguous():
                raise ValueError(f"qk_rope: the pair table must be [positions, {q.dh // 2}, 2] contiguous")
            if q.cs.shape[0] < q.pos0 + (q.rpb if q.rpb else M):
                raise ValueError(f"qk_rope: the pair table has {q.cs.shape[0]} positions, rows reach {q.pos0 + (q.rpb if q.rpb else M)}")
        elif q.dh != 64:
            raise ValueError("qk_rope: the (cos, sin) table may only be omitted at head width 64")
        d.qk_wq, d.qk_wk, d.rope_cs = q.wq.data_ptr(), q.wk.data_ptr(), _p(q.cs)
        d.rope_rpb, d.rope_pos0, d.qk_until_n, d.qk_eps, d.qk_dh = q.rpb, q.pos0, q.until_n, q.eps, q.dh
    stream = _stream()
    ws = _gemm_workspace(a.device, stream)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if lora_t is not None:
        _chk(lora_t, "lora_t", dt); _chk(lora_b, "lora_b", dt)
        d.lora_T, d.ldt, d.lora_B, d.ldb, d.lora_r = lora_t.data_ptr(), lora_t.stride(-2), lora_b.data_ptr(), lora_b.stride(-2), lora_b.shape[-1]
    ev = _timer.begin("gemm") if _timer is not None else None
    _call("ug_gemm_bf16", dt, C.byref(d), stream)
    if ev is not None:
        _timer.end("gemm", 2.0 * M * N * (K + (d.lora_r or 0)) * max(groups, 1), ev, tag=(M, N, K, max(groups, 1), epilogue))
    return out


def small_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, silu_in: bool = False,
                 residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = residual[m] + bf16(act(x[m]) @ w^T + bias), M = x.shape[0] (chunks of <= 16 rows per launch)."""
    dt = _act(x, "x")
    _chk(w, "w", dt); _chk(out, "out", dt)
    if bias is not None:
        _chk(bias, "bias", dt)
    if residual is not None:
        _chk(residual, "residual", dt)
    M, K = x.shape
    N = w.shape[0]
    step = 16 if dt == bf16 else 64     # the bf16 kernel keeps up to 16 rows of x in LDS; more rows re-stream the weights
    for m0 in range(0, M, step):
        mm = min(step, M - m0)
        r = residual[m0:] if residual is not None else None
        _call("ug_small_linear_bf16", dt, x[m0:].data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), _p(bias), _p(r),
              residual.stride(0) if residual is not None else 0, out[m0:].data_ptr(), out.stride(0), mm, N, K, 1 if silu_in else 0, _stream())
    return out


def adaln_modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out: torch.Tensor, *, rows: int, D: int,
                   rows_per_sample: int, mod_ld: int, ldx: Optional[int] = None, x_map: RowMap = IDENT, eps: float = 1e-6) -> torch.Tensor:
    dt = _act(x, "x")
    _chk(shift, "shift", dt); _chk(scale, "scale", dt); _chk(out, "out", dt)
    _call("ug_adaln_modulate", dt, x.data_ptr(), ldx if ldx is not None else x.stride(-2), x_map.rpb, x_map.bstride, shift.data_ptr(), scale.data_ptr(), mod_ld,
          rows_per_sample, out.data_ptr(), out.stride(-2), rows, D, eps, _stream())
    return out


def qk_rmsnorm_rope(buf: torch.Tensor, *, batches: int, rows_per_batch: int, ld: int, q_off: int, k_off: int, heads: int, dh: int,
                    batch_stride_rows: Optional[int] = None, pos_offset: int = 0, wq_a=None, wk_a=None, wq_b=None, wk_b=None,
                    split: int = 0, cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """buf.data_ptr() is row 0 of batch 0 of the processed row range."""
    dt = _act(buf, "buf")
    for wt in (wq_a, wk_a, wq_b, wk_b):
        if wt is not None:
            _chk(wt, "qk-norm weight", dt)
    if batch_stride_rows is None:
        batch_stride_rows = rows_per_batch
    if cos is not None:
        _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
        assert cos.shape[0] >= pos_offset + rows_per_batch and cos.shape[1] == dh and cos.is_contiguous() and sin.is_contiguous(), \
            (cos.shape, pos_offset, rows_per_batch, dh)
    _call("ug_qk_rmsnorm_rope", dt, buf.data_ptr(), ld, batches, rows_per_batch, batch_stride_rows, pos_offset, q_off, k_off, heads, dh, _p(wq_a), _p(wk_a),
          _p(wq_b), _p(wk_b), split, _p(cos), _p(sin), eps, _stream())
    return buf


def flash_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, batches: int, heads: int, dh: int,
               Lq: int, Lkv: int, q_strides, k_strides, v_strides, o_strides, scale: Optional[float] = None,
               lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q/k/v/out are base tensors (data_ptr = element [batch 0, row 0, head 0, 0]); *_strides = (row_stride, batch_stride).
    lse (bf16 path only): fp32 [batches, heads, >= Lq], receives the rows' base-2 log-sum-exp for flash_attn_bwd.
    dh = 512 (the AutoencoderKL mid-block head) runs ug_flash_attn_fwd_wide: forward only, so it takes no lse."""
    dt = _act(q, "q")
    _chk(k, "k", dt); _chk(v, "v", dt); _chk(out, "out", dt)
    if scale is None:
        scale = dh ** -0.5
    if dh == 512 and lse is not None:
        raise L.UniGenHipError("flash_attn: lse= is not available at dh = 512 (ug_flash_attn_fwd_wide is forward only: there is no backward at this head width)")
    ev = _timer.begin("attn") if _timer is not None else None
    if dh == 512:
        _call("ug_flash_attn_fwd_wide", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0],
              v_strides[1], out.data_ptr(), o_strides[0], o_strides[1], batches, heads, Lq, Lkv, dh, scale, _stream())
    elif lse is not None:
        _chk(lse, "lse", torch.float32)
        assert dt == bf16 and lse.is_contiguous() and lse.shape[0] == batches and lse.shape[1] == heads and lse.shape[2] >= Lq
        L.call("ug_flash_attn_fwd_lse", q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0],
               v_strides[1], out.data_ptr(), o_strides[0], o_strides[1], batches, heads, Lq, Lkv, dh, scale, lse.data_ptr(), lse.shape[2], _stream())
    else:
        _call("ug_flash_attn_fwd", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0],
              v_strides[1], out.data_ptr(), o_strides[0], o_strides[1], batches, heads, Lq, Lkv, dh, scale, _stream())
    if ev is not None:
        _timer.end("attn", 4.0 * batches * heads * Lq * Lkv * dh, ev, tag=(batches, heads, Lq, Lkv, dh))
    return out


def timestep_embed(t: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _chk(t, "t", torch.float32)
    dt = _act(out, "out")
    _call("ug_timestep_embed", dt, t.data_ptr(), out.data_ptr(), out.stride(0), t.shape[0], out.shape[1], _stream())
    return out


def euler_step(x: torch.Tensor, v: torch.Tensor, dt: float) -> torch.Tensor:
    adt = _act(x, "x")
    _chk(v, "v", adt)
    assert x.is_contiguous() and v.is_contiguous() and x.numel() == v.numel()
    _call("ug_euler_step", adt, x.data_ptr(), v.data_ptr(), dt, x.numel(), _stream())
    return x


def cfg_combine(uncond: torch.Tensor, text: torch.Tensor, guidance_scale: float, out: torch.Tensor) -> torch.Tensor:
    dt = _act(uncond, "uncond")
    _chk(text, "text", dt); _chk(out, "out", dt)
    assert uncond.is_contiguous() and text.is_contiguous() and out.is_contiguous() and uncond.numel() == text.numel() == out.numel()
    _call("ug_cfg_combine", dt, uncond.data_ptr(), text.data_ptr(), guidance_scale, out.data_ptr(), out.numel(), _stream())
    return out


def dpm_step(pred_uncond: torch.Tensor, pred_text: Optional[torch.Tensor], guidance_scale: float, sample: torch.Tensor, x0_prev: torch.Tensor,
             model_in: Optional[torch.Tensor], *, order: int, sigma: float, a: float, b: float, rinv: float = 0.0) -> torch.Tensor:
    """ug_dpm_step: guidance, x0 = sample - sigma p, the DPM-Solver++ update of `order` and the history, on fp32 `sample` / `x0_prev` in place;
    `model_in` ([copies x sample.numel()] elements of the predictions' dtype, or None) receives the new sample once per copy."""
    dt = _act(pred_uncond, "pred_uncond")
    _chk(sample, "sample", f32); _chk(x0_prev, "x0_prev", f32)
    n = sample.numel()
    assert pred_uncond.is_cuda and pred_uncond.is_contiguous() and sample.is_contiguous() and x0_prev.is_contiguous() and pred_uncond.numel() == x0_prev.numel() == n
    if pred_text is not None:
        _chk(pred_text, "pred_text", dt)
        assert pred_text.is_contiguous() and pred_text.numel() == n
    copies = 0
    if model_in is not None:
        _chk(model_in, "model_in", dt)
        assert model_in.is_contiguous() and n > 0 and model_in.numel() % n == 0
        copies = model_in.numel() // n
    _call("ug_dpm_step", dt, pred_uncond.data_ptr(), _p(pred_text), guidance_scale, sample.data_ptr(), x0_prev.data_ptr(), _p(model_in), copies, order,
          sigma, a, b, rinv, n, _stream())
    return sample


def add(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    dt = _act(a, "a")
    _chk(b, "b", dt); _chk(out, "out", dt)
    D = a.shape[-1]
    rows = a.numel() // D
    a2, b2, o2 = a.reshape(rows, D), b.reshape(rows, D), out.view(rows, D)
    _call("ug_add_bf16", dt, a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), o2.data_ptr(), o2.stride(0), rows, D, _stream())
    return out


def add_rowbcast_f32(x: torch.Tensor, table: torch.Tensor, rows_per_batch: int) -> torch.Tensor:
    """x[r] = bf16(x[r] + table[r % rows_per_batch]) in place; x [rows, D] bf16, table [rows_per_batch, D] fp32."""
    dt = _act(x, "x")
    _chk(table, "table", torch.float32)
    rows, D = x.shape
    assert table.shape == (rows_per_batch, D)
    _call("ug_add_rowbcast_f32", dt, x.data_ptr(), x.stride(0), table.data_ptr(), table.stride(0), rows, rows_per_batch, D, _stream())
    return x


def gather_rows(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[i] = src[idx[i]] (zeros where idx[i] < 0); src [R, W], idx int32 [n], out [n, W]."""
    dt = _act(src, "src")
    _chk(idx, "idx", torch.int32); _chk(out, "out", dt)
    n, W = out.shape
    assert idx.numel() == n and src.shape[1] == W and idx.is_contiguous()
    _call("ug_gather_rows", dt, src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), n, W, _stream())
    return out


def moe_gate_top1(x: torch.Tensor, c: torch.Tensor, wg: torch.Tensor, gates: torch.Tensor, idx: torch.Tensor) -> None:
    dt = _act(x, "x")
    _chk(c, "c", dt); _chk(wg, "wg", dt); _chk(gates, "gates", torch.float32); _chk(idx, "idx", torch.int32)
    S, D = x.shape
    E = wg.shape[0]
    assert x.stride(0) == c.stride(0) and wg.is_contiguous() and gates.is_contiguous()
    _call("ug_moe_gate_top1", dt, x.data_ptr(), c.data_ptr(), x.stride(0), wg.data_ptr(), S, D, E, gates.data_ptr(), idx.data_ptr(), _stream())


def moe_gate_bwd(gates: torch.Tensor, dgates: torch.Tensor, x: torch.Tensor, c: torch.Tensor, wg: torch.Tensor):
    """Backward of moe_gate_top1: gates, d gates [S, E] fp32; x, c [S, D]; wg [E, D] -> (d(x + c) [S, D], d wg [E, D] in wg's dtype)."""
    dt = _act(x, "x")
    _chk(c, "c", dt); _chk(wg, "wg", dt); _chk(gates, "gates", torch.float32); _chk(dgates, "dgates", torch.float32)
    S, D = x.shape
    E = wg.shape[0]
    assert x.stride(0) == c.stride(0) and wg.is_contiguous() and gates.is_contiguous() and dgates.is_contiguous() and gates.shape == dgates.shape == (S, E)
    dx = torch.empty(S, D, device=x.device, dtype=dt)
    part = torch.empty(int(L.load().ug_moe_gate_bwd_slices(S)), E, D, device=x.device, dtype=torch.float32)
    _call("ug_moe_gate_bwd", dt, gates.data_ptr(), dgates.data_ptr(), x.data_ptr(), c.data_ptr(), x.stride(0), wg.data_ptr(), S, D, E, dx.data_ptr(), D,
          part.data_ptr(), _stream())
    return dx, part.sum(0).to(dt)          # the kernel's per-slice fp32 partials, added in a fixed order


def moe_capacity_rts(gates, idx, uniform, capacity: int, slot, token_of_slot, exp_counts, l_aux) -> None:
    _chk(gates, "gates", torch.float32); _chk(idx, "idx", torch.int32); _chk(uniform, "uniform", torch.float32)
    _chk(slot, "slot", torch.int32); _chk(token_of_slot, "token_of_slot", torch.int32)
    _chk(exp_counts, "exp_counts", torch.int64); _chk(l_aux, "l_aux", torch.float32)
    S, E = gates.shape
    assert uniform.shape == (S, E) and uniform.is_contiguous() and token_of_slot.numel() == E * capacity
    L.call("ug_moe_capacity_rts", gates.data_ptr(), idx.data_ptr(), uniform.data_ptr(), S, E, capacity, slot.data_ptr(), token_of_slot.data_ptr(),
           exp_counts.data_ptr(), l_aux.data_ptr(), _stream())


def moe_gate_top2(x: torch.Tensor, c: torch.Tensor, wg: torch.Tensor, noise: Optional[torch.Tensor], gates: torch.Tensor, idx: torch.Tensor) -> None:
    """top2gating's gate: gates [S, E] fp32, idx int32 [2, S] (first choice = argmax, second = argmax of logits + noise over the others)."""
    dt = _act(x, "x")
    _chk(c, "c", dt); _chk(wg, "wg", dt); _chk(gates, "gates", torch.float32); _chk(idx, "idx", torch.int32)
    S, D = x.shape
    E = wg.shape[0]
    assert x.stride(0) == c.stride(0) and wg.is_contiguous() and gates.is_contiguous() and idx.is_contiguous() and idx.shape == (2, S)
    if noise is not None:
        _chk(noise, "noise", torch.float32); assert noise.shape == (S, E) and noise.is_contiguous()
    _call("ug_moe_gate_top2", dt, x.data_ptr(), c.data_ptr(), x.stride(0), wg.data_ptr(), S, D, E, _p(noise), gates.data_ptr(), idx.data_ptr(), _stream())


def moe_capacity_top2(gates, idx, capacity: int, slot, token_of_slot, weights, exp_counts, l_aux) -> None:
    _chk(gates, "gates", torch.float32); _chk(idx, "idx", torch.int32); _chk(slot, "slot", torch.int32); _chk(token_of_slot, "token_of_slot", torch.int32)
    _chk(weights, "weights", torch.float32); _chk(exp_counts, "exp_counts", torch.int64); _chk(l_aux, "l_aux", torch.float32)
    S, E = gates.shape
    assert idx.shape == slot.shape == weights.shape == (2, S) and idx.is_contiguous() and slot.is_contiguous() and weights.is_contiguous()
    assert token_of_slot.numel() == E * capacity and token_of_slot.is_contiguous() and gates.is_contiguous()
    L.call("ug_moe_capacity_top2", gates.data_ptr(), idx.data_ptr(), S, E, capacity, slot.data_ptr(), token_of_slot.data_ptr(), weights.data_ptr(),
           exp_counts.data_ptr(), l_aux.data_ptr(), _stream())


def moe_gate_topk(x: torch.Tensor, c: torch.Tensor, wg: torch.Tensor, K: int, gates: torch.Tensor, logits: torch.Tensor, idx: torch.Tensor) -> None:
    """topkgating's gate (k > 2): gates, logits [S, E] fp32, idx int32 [K, S] (the token's K choices by descending logit)."""
    dt = _act(x, "x")
    _chk(c, "c", dt); _chk(wg, "wg", dt); _chk(gates, "gates", torch.float32); _chk(logits, "logits", torch.float32); _chk(idx, "idx", torch.int32)
    S, D = x.shape
    E = wg.shape[0]
    assert c.shape == x.shape and wg.shape[1] == D and gates.shape == (S, E) and logits.shape == (S, E) and idx.shape == (K, S) and idx.is_contiguous()
    assert x.stride(0) == c.stride(0) and gates.is_contiguous() and logits.is_contiguous()
    _call("ug_moe_gate_topk", dt, x.data_ptr(), c.data_ptr(), x.stride(0), wg.data_ptr(), S, D, E, K, gates.data_ptr(), logits.data_ptr(), idx.data_ptr(),
          _stream())


def moe_capacity_topk(gates, logits, idx, capacity: int, slot, token_of_slot, weights, exp_counts, l_aux) -> None:
    """topkgating's capacity rule + combine weights + l_aux (include/unigen_hip.h): idx / slot / weights [K, S]."""
    S, E = gates.shape
    K = idx.shape[0]
    for t, dt in ((gates, torch.float32), (logits, torch.float32), (idx, torch.int32), (slot, torch.int32), (token_of_slot, torch.int32), (weights, torch.float32),
                  (exp_counts, torch.int64), (l_aux, torch.float32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    assert logits.shape == (S, E) and idx.shape == (K, S) and slot.shape == (K, S) and weights.shape == (K, S) and token_of_slot.shape == (E, capacity)
    L.call("ug_moe_capacity_topk", gates.data_ptr(), logits.data_ptr(), idx.data_ptr(), S, E, K, capacity, slot.data_ptr(), token_of_slot.data_ptr(),
           weights.data_ptr(), exp_counts.data_ptr(), l_aux.data_ptr(), _stream())


def moe_combine_topk(yh, yc, weights, idx, slot, out, *, E: int, capacity: int, xs=None, cs=None, s_map: RowMap = IDENT, accumulate: bool = False) -> torch.Tensor:
    """weights fp32 / idx / slot [K, S'] (S' >= S: column slices of longer arrays keep their row stride); otherwise as moe_combine."""
    dt = _act(yh, "yh")
    _chk(yc, "yc", dt); _chk(out, "out", dt); _chk(weights, "weights", torch.float32); _chk(idx, "idx", torch.int32); _chk(slot, "slot", torch.int32)
    S, D = out.shape[-2], out.shape[-1]
    K = weights.shape[0]
    ks = weights.stride(0) if K > 1 else max(S, 1)
    assert weights.shape == idx.shape == slot.shape == (K, S) and weights.stride(1) == idx.stride(1) == slot.stride(1) == 1
    assert K == 1 or (idx.stride(0) == ks and slot.stride(0) == ks)
    if xs is not None:
        _chk(xs, "xs", dt); _chk(cs, "cs", dt); assert xs.stride(-2) == cs.stride(-2)
    _call("ug_moe_combine_topk", dt, yh.data_ptr(), yc.data_ptr(), weights.data_ptr(), idx.data_ptr(), slot.data_ptr(), K, ks, E, capacity, _p(xs), _p(cs),
          xs.stride(-2) if xs is not None else 0, s_map.rpb, s_map.bstride, out.data_ptr(), out.stride(-2), S, D, 1 if accumulate else 0, _stream())
    return out


def moe_dispatch_modulate(x, add_, mod, token_of_slot, out, *, E: int, capacity: int, tokens_per_sample: int,
                          mod_estride: int = 0, mod_bstride: int = 0) -> torch.Tensor:
    """mod: the expert-modulation vectors, row of (expert e, sample b) at element offset e * mod_estride + b * mod_bstride."""
    dt = _act(x, "x")
    _chk(out, "out", dt); _chk(token_of_slot, "token_of_slot", torch.int32)
    D = x.shape[-1]
    assert out.is_contiguous() and out.numel() == E * capacity * D
    if mod is not None:
        _chk(mod, "mod", dt)
    if add_ is not None:
        _chk(add_, "add", dt); assert add_.is_contiguous()
    _call("ug_moe_dispatch_modulate", dt, x.data_ptr(), x.stride(-2), _p(add_), _p(mod), mod_estride, mod_bstride, token_of_slot.data_ptr(), E, capacity,
          tokens_per_sample, D, out.data_ptr(), _stream())
    return out


def moe_combine(yh, yc, gates, idx, slot, out, *, E: int, capacity: int, xs=None, cs=None, s_map: RowMap = IDENT, accumulate: bool = False) -> torch.Tensor:
    """xs / cs: base tensors of the shared experts' image / condition streams; token s is row s_map(s) of them."""
    dt = _act(yh, "yh")
    _chk(yc, "yc", dt); _chk(out, "out", dt)
    S, D = out.shape[-2], out.shape[-1]
    if xs is not None:
        _chk(xs, "xs", dt); _chk(cs, "cs", dt); assert xs.stride(-2) == cs.stride(-2)
    _call("ug_moe_combine", dt, yh.data_ptr(), yc.data_ptr(), gates.data_ptr(), idx.data_ptr(), slot.data_ptr(), E, capacity, _p(xs), _p(cs),
          xs.stride(-2) if xs is not None else 0, s_map.rpb, s_map.bstride, out.data_ptr(), out.stride(-2), S, D, 1 if accumulate else 0, _stream())
    return out


def pack_latents(latents: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FluxPipeline._pack_latents: [B, C, H, W] -> [B, (H/2)(W/2), 4C] (src/UniGenPipeline.py:641)."""
    dt = _act(latents, "latents")
    B, Cc, H, W = latents.shape
    latents = latents.contiguous()
    if out is None:
        out = torch.empty(B, (H // 2) * (W // 2), Cc * 4, device=latents.device, dtype=dt)
    _chk(out, "out", dt); assert out.is_contiguous() and out.numel() == latents.numel()
    _call("ug_pack_latents", dt, latents.data_ptr(), out.data_ptr(), B, Cc, H, W, _stream())
    return out


def unpack_latents(packed: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FluxPipeline._unpack_latents: [B, (H/2)(W/2), 4C] -> [B, C, H, W] (H, W = latent height / width; src/UniGenPipeline.py:796)."""
    dt = _act(packed, "packed")
    B, n, ch = packed.shape
    assert n == (H // 2) * (W // 2) and ch % 4 == 0, (packed.shape, H, W)
    packed = packed.contiguous()
    if out is None:
        out = torch.empty(B, ch // 4, H, W, device=packed.device, dtype=dt)
    _chk(out, "out", dt); assert out.is_contiguous()
    _call("ug_unpack_latents", dt, packed.data_ptr(), out.data_ptr(), B, ch // 4, H, W, _stream())
    return out


def probe_mfma_peak(device, shape: int = 1, seconds: float = 0.4) -> float:
    """Measured dense bf16 MFMA rate (TFLOP/s) of a bare register-operand MFMA loop on every CU (ug_probe_mfma_bf16), timed with HIP
    events on the current stream over ~`seconds` of back-to-back launches so the chip settles at the clock it holds under matrix load.
    shape 0 = 32x32x16, 1 = 16x16x32 (the shape the GEMM uses)."""
    props = torch.cuda.get_device_properties(device)
    blocks = props.multi_processor_count
    scratch = torch.empty(blocks * 256, dtype=torch.float32, device=device)
    fl = C.c_double(0.0)
    iters = 100_000
    launch = lambda: L.call("ug_probe_mfma_bf16", shape, blocks, iters, scratch.data_ptr(), C.byref(fl), _stream())
    launch()
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); launch(); e1.record(); e1.synchronize()
    n = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    for _ in range(n):          # settle the clock
        launch()
    e0.record()
    for _ in range(n):
        launch()
    e1.record(); e1.synchronize()
    return fl.value * n / (e0.elapsed_time(e1) * 1e-3) / 1e12


# ---------------------------------------------------------------------------------------------------------------------
# AutoencoderKL ops (unigen_amd/vae.py): NHWC activations as 2-D tensors [B * H * W, C]
# ---------------------------------------------------------------------------------------------------------------------
_zero_pages: dict = {}


def _zero_page(device) -> torch.Tensor:
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(4096, dtype=torch.uint8, device=device)      # >= 2 * (Cin + 64) bytes for Cin <= 1984: the 256^2 convolution path
        _zero_pages[device] = z
    return z


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, B: int, H: int, W: int, Ho: int, Wo: int, KH: int, KW: int,
                stride: int = 1, pad_t: int = 1, pad_l: int = 1, up: int = 0, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[B*Ho*Wo, Cout] = residual + conv(x[B*H*W, Cin]; w[Cout, KH, KW, Cin]) + bias (ug_conv2d_nhwc: implicit GEMM, see include/unigen_hip.h)."""
    dt = _act(x, "x")
    _chk(w, "w", dt); _chk(out, "out", dt)
    Cin, Cout = x.shape[-1], out.shape[-1]
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and w.numel() == Cout * KH * KW * Cin, (x.shape, w.shape, out.shape)
    assert x.numel() == B * H * W * Cin and out.numel() == B * Ho * Wo * Cout
    d = L.ConvDesc()
    d.x, d.B, d.H, d.W, d.Cin = x.data_ptr(), B, H, W, Cin
    d.w, d.bias = w.data_ptr(), _p(bias)
    if bias is not None:
        _chk(bias, "bias", dt)
    if residual is not None:
        _chk(residual, "residual", dt); assert residual.is_contiguous() and residual.numel() == out.numel()
        d.R = residual.data_ptr()
    d.out, d.Ho, d.Wo, d.Cout = out.data_ptr(), Ho, Wo, Cout
    d.KH, d.KW, d.stride, d.pad_t, d.pad_l, d.up = KH, KW, stride, pad_t, pad_l, up
    zp = _zero_page(x.device)
    d.zero_page, d.zero_page_bytes = zp.data_ptr(), zp.numel()
    _call("ug_conv2d_nhwc", dt, C.byref(d), _stream())
    return out


_gn_ws: dict = {}


def groupnorm_nhwc(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, *, B: int, HW: int, groups: int, eps: float = 1e-6,
                   silu: bool = False) -> torch.Tensor:
    dt = _act(x, "x")
    _chk(gamma, "gamma", dt); _chk(beta, "beta", dt); _chk(out, "out", dt)
    Cc = x.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == B * HW * Cc
    need = int(L.load().ug_groupnorm_workspace_bytes(B, HW, groups))
    key = (x.device, _stream())
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _gn_ws[key] = ws
    _call("ug_groupnorm_nhwc", dt, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), B, HW, Cc, groups, eps,
          1 if silu else 0, _stream())
    return out


def softmax_rows(scores: torch.Tensor, probs: torch.Tensor, scale: float) -> torch.Tensor:
    """probs[r] = softmax(scale * scores[r]); scores fp32 [rows, cols], probs bf16 (or fp32: verification) [rows, cols]."""
    _chk(scores, "scores", torch.float32)
    dt = _act(probs, "probs")
    rows, cols = scores.shape
    _call("ug_softmax_rows", dt, scores.data_ptr(), scores.stride(0), probs.data_ptr(), probs.stride(0), rows, cols, scale, _stream())
    return probs


def nchw_to_nhwc(x: torch.Tensor, Cp: int, div: float = 0.0, add: float = 0.0) -> torch.Tensor:
    """[B, C, H, W] -> [B*H*W, Cp] (channels >= C zero); div != 0: v -> (v / div) + add on the way (latents / scaling_factor + shift_factor)."""
    dt = _act(x, "x")
    B, Cc, H, W = x.shape
    x = x.contiguous()
    out = torch.empty(B * H * W, Cp, device=x.device, dtype=dt)
    _call("ug_nchw_to_nhwc", dt, x.data_ptr(), out.data_ptr(), B, Cc, H * W, Cp, div, add, _stream())
    return out


def nhwc_to_nchw(x: torch.Tensor, B: int, Cc: int, H: int, W: int) -> torch.Tensor:
    """[B*H*W, Cp] -> [B, C, H, W] (first C channels)."""
    dt = _act(x, "x")
    assert x.is_contiguous() and x.shape[0] == B * H * W and x.shape[1] >= Cc
    out = torch.empty(B, Cc, H, W, device=x.device, dtype=dt)
    _call("ug_nhwc_to_nchw", dt, x.data_ptr(), out.data_ptr(), B, Cc, H * W, x.shape[1], _stream())
    return out


def vae_sample(moments: torch.Tensor, noise: torch.Tensor, *, B: int, latent: int, H: int, W: int, shift: float = 0.0, scale: float = 1.0) -> torch.Tensor:
    """z [B, L, H, W] = ((mean + exp(0.5 clamp(logvar)) * noise) - shift) * scale from NHWC moments [B*H*W, Cp >= 2L] and NCHW noise."""
    dt = _act(moments, "moments")
    _chk(noise, "noise", dt)
    assert moments.is_contiguous() and noise.is_contiguous() and noise.numel() == B * latent * H * W
    z = torch.empty(B, latent, H, W, device=moments.device, dtype=dt)
    _call("ug_vae_sample", dt, moments.data_ptr(), moments.shape[1], noise.data_ptr(), z.data_ptr(), B, latent, H * W, shift, scale, _stream())
    return z


def _chk_view(t: torch.Tensor, name: str, dt) -> None:
    """a strided [B, C, H, W] view handed over with its element strides: any layout, but on the device, of the call's dtype, and no stride negative"""
    if not t.is_cuda:
        raise L.UniGenHipError(f"{name}: expected a GPU tensor (unigen_amd has no CPU path)")
    if t.dtype != dt:
        raise TypeError(f"{name}: expected {dt}, got {t.dtype}")
    if t.dim() != 4 or min(t.stride()) < 0:
        raise ValueError(f"{name}: expected a [B, C, H, W] view with non-negative strides, got shape {tuple(t.shape)} strides {t.stride()}")


def _vae_tile(t: Optional[torch.Tensor], dt, B: int, Cc: int) -> L.VaeTile:
    v = L.VaeTile()
    if t is not None:
        _chk_view(t, "tile", dt)
        assert t.dim() == 4 and t.shape[0] == B and t.shape[1] == Cc, (t.shape, B, Cc)
        v.p, v.H, v.W = t.data_ptr(), t.shape[2], t.shape[3]
        v.sb, v.sc, v.sy, v.sx = t.stride()
    return v


def vae_tile_blend(tile: torch.Tensor, upper: Optional[torch.Tensor], left: Optional[torch.Tensor], upper_left: Optional[torch.Tensor], out: torch.Tensor,
                   extent: int) -> torch.Tensor:
    """One tile of AutoencoderKL.tiled_decode / tiled_encode into its canvas region (ug_vae_tile_blend: blend_v, blend_h, crop and cat in one pass).
    Every tensor is a logical [B, C, H, W] VIEW of any strides (NHWC rows: `rows.view(B, H, W, Cp).permute(0, 3, 1, 2)[:, :C]`); `out` is the view of
    the canvas region [B, C, h, w] that receives rows [0, h) x columns [0, w) of the blended tile. Neighbours are the RAW tiles, or None."""
    dt = _act(tile, "tile")
    _chk_view(out, "out", dt)
    B, Cc, h, w = out.shape
    d = L.VaeBlendDesc()
    d.T, d.U, d.Lf, d.UL = (_vae_tile(t, dt, B, Cc) for t in (tile, upper, left, upper_left))
    d.out = out.data_ptr()
    d.ob, d.oc, d.oy, d.ox = out.stride()
    d.B, d.C, d.h, d.w, d.E = B, Cc, h, w, int(extent)
    _call("ug_vae_tile_blend", dt, C.byref(d), _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# backward-pass entry points (include/unigen_hip.h "Backward pass of the control-module training step")
# ---------------------------------------------------------------------------------------------------------------------
def transpose(src: torch.Tensor, rows_pad: Optional[int] = None) -> torch.Tensor:
    """src [..., rows, cols] (any row stride, uniform batch stride) -> [..., cols, rows_pad] contiguous, zero beyond `rows`."""
    dt = _act(src, "src")
    rows, cols = src.shape[-2], src.shape[-1]
    rows_pad = rows if rows_pad is None else rows_pad
    lead = src.shape[:-2]
    batch = 1
    for d in lead:
        batch *= d
    if len(lead) > 1:
        raise ValueError("transpose: at most one batch dimension")
    bstride = src.stride(0) if lead else 0
    out = torch.empty(*lead, cols, rows_pad, device=src.device, dtype=dt)
    _call("ug_transpose", dt, src.data_ptr(), src.stride(-2), bstride, out.data_ptr(), rows_pad, cols * rows_pad, batch, rows, cols, rows_pad, _stream())
    return out


def colsum(a: torch.Tensor, b: Optional[torch.Tensor] = None, *, rows_per_group: Optional[int] = None, alpha: float = 1.0) -> torch.Tensor:
    """a (and b) [rows, cols] -> [rows / rows_per_group, cols]: per-group column sums of a (* b), fp32 accumulation."""
    dt = _act(a, "a")
    rows, cols = a.shape
    g = rows if rows_per_group is None else rows_per_group
    if b is not None:
        _chk(b, "b", dt)
    out = torch.empty(rows // g, cols, device=a.device, dtype=dt)
    ws = torch.empty(int(L.load().ug_colsum_workspace_bytes(rows, cols, g)), device=a.device, dtype=torch.uint8)
    _call("ug_colsum", dt, a.data_ptr(), a.stride(0), _p(b), b.stride(0) if b is not None else 0, out.data_ptr(), cols, rows, cols, g, alpha, ws.data_ptr(),
          ws.numel(), _stream())
    return out


def lora_wgrad(p: torch.Tensor, q: torch.Tensor, out: Optional[torch.Tensor] = None, *, alpha: float = 1.0) -> torch.Tensor:
    """p [M, R]^T q [M, J] -> [R, J] (ug_lora_wgrad_bf16 / _f32): the adapter gradients dA_cat = dT^T X and dB_bd^T = T^T dY straight from the row-major
    operands (any row stride that is a multiple of 8). R = 64 ... 256 in steps of 64, J a multiple of 64, any M. `out`: a [R, J] tensor or column
    block (its row stride is the leading dimension)."""
    dt = _act(p, "p")
    _chk(p, "p", dt); _chk(q, "q", dt)
    (M, R), J = p.shape, q.shape[1]
    if q.shape[0] != M or p.dim() != 2 or q.dim() != 2:
        raise ValueError(f"lora_wgrad: p {tuple(p.shape)} and q {tuple(q.shape)} must share their rows")
    if out is None:
        out = torch.empty(R, J, device=p.device, dtype=dt)
    _chk(out, "out", dt)
    if tuple(out.shape) != (R, J):
        raise ValueError(f"lora_wgrad: out must be [{R}, {J}], got {tuple(out.shape)}")
    ws = torch.empty(int(L.load().ug_lora_wgrad_workspace_bytes(M, R, J)), device=p.device, dtype=torch.uint8)
    _call("ug_lora_wgrad_bf16", dt, p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), out.data_ptr(), out.stride(0), M, R, J, alpha, ws.data_ptr(),
          ws.numel(), _stream())
    return out


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    dt = _act(x, "x")
    x = x.contiguous()
    out = torch.empty_like(x)
    _call("ug_gelu_tanh", dt, x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def gelu_tanh_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    dt = _act(x, "x")
    x, dy = x.contiguous(), dy.contiguous()
    _chk(dy, "dy", dt)
    out = torch.empty_like(x)
    _call("ug_gelu_tanh_bwd", dt, x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def adaln_modulate_bwd(x: torch.Tensor, dy: torch.Tensor, scale: torch.Tensor, *, rows_per_sample: int, eps: float = 1e-6):
    """x, dy [rows, D]; scale [samples, D] (row stride = its stride(0)) -> (dx [rows, D], d shift [samples, D], d scale [samples, D])."""
    dt = _act(x, "x")
    _chk(dy, "dy", dt); _chk(scale, "scale", dt)
    rows, D = x.shape
    samples = rows // rows_per_sample
    dx = torch.empty(rows, D, device=x.device, dtype=dt)
    part = torch.empty(samples, int(L.load().ug_adaln_modulate_bwd_partials(rows, rows_per_sample)), 2, D, device=x.device, dtype=torch.float32)
    _call("ug_adaln_modulate_bwd", dt, x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), scale.data_ptr(), scale.stride(0), rows_per_sample,
          dx.data_ptr(), D, part.data_ptr(), rows, D, eps, _stream())
    sums = part.sum(1).to(dt) if part.shape[1] > 1 else part[:, 0].to(dt)         # the kernel's per-sample partials, added in a fixed order
    return dx, sums[:, 0], sums[:, 1]


def qk_rmsnorm_rope_bwd(x: torch.Tensor, dy: torch.Tensor, w: Optional[torch.Tensor], cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], *,
                        rows_per_batch: int, pos_offset: int, heads: int, dh: int, eps: float = 1e-6):
    """x, dy [rows, heads * dh] (any row stride) -> (dx [rows, heads * dh], d weight [dh] in x's dtype or None)."""
    dt = _act(x, "x")
    _chk(dy, "dy", dt)
    rows = x.shape[0]
    dx = torch.empty(rows, heads * dh, device=x.device, dtype=dt)
    dwx = torch.empty(int(L.load().ug_qk_rmsnorm_rope_bwd_partials(rows, heads)), dh, device=x.device, dtype=torch.float32) if w is not None else None
    if cos is not None:
        _chk(cos, "cos", torch.float32); _chk(sin, "sin", torch.float32)
        assert cos.shape[0] >= pos_offset + rows_per_batch and cos.shape[1] == dh and cos.is_contiguous() and sin.is_contiguous()
    _call("ug_qk_rmsnorm_rope_bwd", dt, x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), dx.data_ptr(), heads * dh, _p(dwx), _p(w), _p(cos), _p(sin),
          rows, rows_per_batch, pos_offset, heads, dh, eps, _stream())
    return dx, (dwx.sum(0).to(dt) if dwx is not None else None)       # <= 2048 fp32 partial rows of the kernel, added in a fixed order


def row_lse(S: torch.Tensor, scale: float, valid_cols: Optional[int] = None) -> torch.Tensor:
    _chk(S, "S", torch.float32)
    rows, cols = S.shape
    out = torch.empty(rows, device=S.device, dtype=torch.float32)
    L.call("ug_row_lse", S.data_ptr(), S.stride(0), out.data_ptr(), rows, valid_cols or cols, scale, _stream())
    return out


def attn_prob(S: torch.Tensor, lse: torch.Tensor, scale: float, dtype, valid_cols: Optional[int] = None) -> torch.Tensor:
    rows, cols = S.shape
    P = torch.empty(rows, cols, device=S.device, dtype=dtype)
    _call("ug_attn_prob", dtype, S.data_ptr(), S.stride(0), lse.data_ptr(), P.data_ptr(), cols, rows, cols, valid_cols or cols, scale, _stream())
    return P


def attn_dscore(P: torch.Tensor, dP: torch.Tensor, delta: torch.Tensor, scale: float) -> torch.Tensor:
    dt = _act(P, "P")
    rows, cols = P.shape
    dS = torch.empty_like(P)
    _call("ug_attn_dscore", dt, P.data_ptr(), P.stride(0), dP.data_ptr(), dP.stride(0), delta.data_ptr(), dS.data_ptr(), cols, rows, cols, scale, _stream())
    return dS


def rowdot(a: torch.Tensor, b: torch.Tensor, groups: int) -> torch.Tensor:
    """a, b [rows, groups * cols] -> [groups, rows] fp32: per-group row dot products."""
    dt = _act(a, "a")
    _chk(b, "b", dt)
    rows = a.shape[0]
    cols = a.shape[1] // groups
    out = torch.empty(groups, rows, device=a.device, dtype=torch.float32)
    _call("ug_rowdot", dt, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), rows, groups, cols, _stream())
    return out


def flash_attn_bwd(q, k, v, o, do, *, heads: int, lse: Optional[torch.Tensor] = None, scale: Optional[float] = None):
    """q, o, do [B, Lq, H * dh], k, v [B, Lkv, H * dh] (any row / batch strides, bf16) -> (dq, dk, dv) contiguous.
    lse: what flash_attn(..., lse=) wrote, fp32 [B, H, Lq rounded up to 64] with zero padding (None: recomputed).
    scale: the softmax scale of the forward (None: dh ** -0.5)."""
    _chk(q, "q"); _chk(k, "k"); _chk(v, "v"); _chk(o, "o"); _chk(do, "do")
    B, Lq, HD = q.shape
    Lkv, dh = k.shape[1], HD // heads
    dq, dk, dv = torch.empty(B, Lq, HD, device=q.device, dtype=bf16), torch.empty(B, Lkv, HD, device=q.device, dtype=bf16), torch.empty(B, Lkv, HD, device=q.device, dtype=bf16)
    lib = L.load()
    ws = torch.empty(int(lib.ug_flash_attn_bwd_workspace_bytes(B, heads, Lq)), device=q.device, dtype=torch.uint8)
    st = lambda t: (t.data_ptr(), t.stride(1), t.stride(0))
    ev = _timer.begin("attn_bwd") if _timer is not None else None
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, heads, (Lq + 63) // 64 * 64), lse.shape
    L.call("ug_flash_attn_bwd", *st(q), *st(k), *st(v), *st(o), *st(do), *st(dq), *st(dk), *st(dv), B, heads, Lq, Lkv, dh, dh ** -0.5 if scale is None else float(scale), _p(lse),
           ws.data_ptr(),
           ws.numel(), _stream())
    if ev is not None:
        _timer.end("attn_bwd", 10.0 * B * heads * Lq * Lkv * dh, ev)
    return dq, dk, dv


def gate_residual(x: Optional[torch.Tensor], a: torch.Tensor, gate: torch.Tensor, rows_per_sample: int) -> torch.Tensor:
    """a (and x) [rows, D]; gate [samples, D] -> x + gate[row // rows_per_sample] * a (x None: the product alone)."""
    dt = _act(a, "a")
    _chk(gate, "gate", dt)
    if x is not None:
        _chk(x, "x", dt)
    rows, D = a.shape
    y = torch.empty(rows, D, device=a.device, dtype=dt)
    _call("ug_gate_residual", dt, _p(x), x.stride(0) if x is not None else 0, a.data_ptr(), a.stride(0), gate.data_ptr(), gate.stride(0), rows_per_sample,
          y.data_ptr(), D, rows, D, _stream())
    return y


FLOW_SCHEMES = {"none": L.UG_FLOW_NONE, "sigma_sqrt": L.UG_FLOW_SIGMA_SQRT, "cosmap": L.UG_FLOW_COSMAP, "logit_normal": L.UG_FLOW_LOGIT_NORMAL,
                "mode": L.UG_FLOW_MODE}


def _chk_f32_vec(t: torch.Tensor, name: str, n: int) -> None:
    _chk(t, name, f32)
    if t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: expected {n} contiguous fp32 values, got {tuple(t.shape)}")


def flow_noise(x: torch.Tensor, noise: torch.Tensor, u: torch.Tensor, sigma_table: torch.Tensor, *, scheme: str = "none", pack: bool = True):
    """x, noise [B, C, H, W]; u [B] fp32 draws in [0, 1); sigma_table [T] fp32 -> noisy, target (x's dtype; [B, (H/2)(W/2), 4C] when `pack`, else
    x's shape), sigma, timestep, weight ([B] fp32): train.py:598-613 and the loss weighting of :644 in one launch (ug_flow_noise / _f32)."""
    dt = _act(x, "x")
    if x.dim() != 4 or noise.shape != x.shape:
        raise ValueError(f"flow_noise: x and noise must share a [B, C, H, W] shape, got {tuple(x.shape)} and {tuple(noise.shape)}")
    if scheme not in FLOW_SCHEMES:
        raise ValueError(f"flow_noise: unknown weighting scheme {scheme!r} (one of {sorted(FLOW_SCHEMES)})")
    _chk(noise, "noise", dt)
    B, Cc, H, W = x.shape
    _chk_f32_vec(u, "u", B)
    _chk(sigma_table, "sigma_table", f32)
    if sigma_table.dim() != 1 or not sigma_table.is_contiguous():
        raise ValueError("flow_noise: sigma_table must be a contiguous 1-d tensor")
    x, noise = x.contiguous(), noise.contiguous()
    shape = (B, (H // 2) * (W // 2), Cc * 4) if pack else (B, Cc, H, W)
    noisy, target = torch.empty(shape, device=x.device, dtype=dt), torch.empty(shape, device=x.device, dtype=dt)
    svw = torch.empty(3, B, device=x.device, dtype=f32)
    _call("ug_flow_noise", dt, x.data_ptr(), noise.data_ptr(), u.data_ptr(), sigma_table.data_ptr(), sigma_table.numel(), FLOW_SCHEMES[scheme],
          1 if pack else 0, B, Cc, H, W, noisy.data_ptr(), target.data_ptr(), svw[0].data_ptr(), svw[1].data_ptr(), svw[2].data_ptr(), _stream())
    return noisy, target, svw[0], svw[1], svw[2]


def _flow_pair(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, who: str):
    dt = _act(pred, "pred")
    _chk(target, "target", dt)
    if pred.dim() < 2 or pred.shape != target.shape:
        raise ValueError(f"{who}: pred and target must share a [B, ...] shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    B = pred.shape[0]
    _chk_f32_vec(weight, "weight", B)
    return dt, B, pred.numel() // B, pred.contiguous(), target.contiguous()


def flow_loss(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    """pred, target [B, ...]; weight [B] fp32 -> (loss_per_sample [B], loss []) fp32: mean over a sample of weight * (pred - target)^2 and the mean of
    those over the batch (train.py:648-652), fp32 accumulation, bit-identical run to run. `workspace`: >= ug_flow_loss_workspace_bytes(B, n) bytes."""
    dt, B, n, pred, target = _flow_pair(pred, target, weight, "flow_loss")
    nbytes = int(L.load().ug_flow_loss_workspace_bytes(B, n))
    if workspace is None:
        workspace = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    per_sample, loss = torch.empty(B, device=pred.device, dtype=f32), torch.empty((), device=pred.device, dtype=f32)
    _call("ug_flow_loss", dt, pred.data_ptr(), target.data_ptr(), weight.data_ptr(), B, n, per_sample.data_ptr(), loss.data_ptr(), workspace.data_ptr(),
          workspace.numel() * workspace.element_size(), _stream())
    return per_sample, loss


def flow_loss_bwd(pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """d loss / d pred of flow_loss, scaled by the device fp32 scalar `gout` (read by the kernel: no host copy), in pred's dtype and shape."""
    dt, B, n, pred, target = _flow_pair(pred, target, weight, "flow_loss_bwd")
    _chk_f32_vec(gout, "gout", 1)
    grad = torch.empty_like(pred)
    _call("ug_flow_loss_bwd", dt, pred.data_ptr(), target.data_ptr(), weight.data_ptr(), gout.data_ptr(), B, n, grad.data_ptr(), _stream())
    return grad


# ---- text encoders (csrc/text.hip) ----------------------------------------------------------------------------------------------------
def flash_attn_bias(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, batches: int, heads: int, dh: int, Lq: int, Lkv: int,
                    q_strides, k_strides, v_strides, o_strides, scale: float, rel_table: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """flash_attn with an additive relative-position bias (rel_table fp32 [heads, 2 * rel_len - 1], indexed by k - q) and / or a causal mask."""
    dt = _act(q, "q")
    _chk(k, "k", dt); _chk(v, "v", dt); _chk(out, "out", dt)
    rel_len = 0
    if rel_table is not None:
        _chk(rel_table, "rel_table", torch.float32)
        if rel_table.dim() != 2 or rel_table.shape[0] != heads or rel_table.shape[1] % 2 != 1 or not rel_table.is_contiguous():
            raise ValueError(f"rel_table: expected a contiguous [heads = {heads}, 2 * rel_len - 1] table, got {tuple(rel_table.shape)}")
        rel_len = (rel_table.shape[1] + 1) // 2
    ev = _timer.begin("attn") if _timer is not None else None
    _call("ug_flash_attn_fwd_bias", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0],
          v_strides[1], out.data_ptr(), o_strides[0], o_strides[1], batches, heads, Lq, Lkv, dh, scale, _p(rel_table), rel_len, 1 if causal else 0, _stream())
    if ev is not None:
        _timer.end("attn", 4.0 * batches * heads * Lq * Lkv * dh * (0.5 if causal else 1.0), ev, tag=(batches, heads, Lq, Lkv, dh))
    return out


def t5_rel_table(weight: torch.Tensor, L_: int, *, num_buckets: int, max_distance: int) -> torch.Tensor:
    """fp32 [heads, 2L - 1]: T5's relative-position bias as a function of k - q, from relative_attention_bias.weight [num_buckets, heads]."""
    dt = _act(weight, "weight")
    if weight.dim() != 2 or weight.shape[0] != num_buckets or not weight.is_contiguous():
        raise ValueError(f"weight: expected a contiguous [num_buckets = {num_buckets}, heads] tensor, got {tuple(weight.shape)}")
    heads = weight.shape[1]
    table = torch.empty(heads, 2 * L_ - 1, dtype=torch.float32, device=weight.device)
    _call("ug_t5_rel_table", dt, weight.data_ptr(), num_buckets, max_distance, heads, L_, table.data_ptr(), _stream())
    return table


def rmsnorm_rows(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T5LayerNorm over the last dimension of x [rows, D]."""
    dt = _act(x, "x")
    _chk(w, "w", dt)
    rows, D = x.shape
    out = torch.empty(rows, D, dtype=dt, device=x.device) if out is None else out
    _chk(out, "out", dt)
    assert w.numel() == D and out.shape == x.shape
    _call("ug_rmsnorm_rows", dt, x.data_ptr(), x.stride(0), w.data_ptr(), out.data_ptr(), out.stride(0), rows, D, eps, _stream())
    return out


def layernorm_rows(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.LayerNorm (weight and bias) over the last dimension of x [rows, D]."""
    dt = _act(x, "x")
    _chk(w, "w", dt); _chk(b, "b", dt)
    rows, D = x.shape
    out = torch.empty(rows, D, dtype=dt, device=x.device) if out is None else out
    _chk(out, "out", dt)
    assert w.numel() == D and b.numel() == D and out.shape == x.shape
    _call("ug_layernorm_rows", dt, x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), out.data_ptr(), out.stride(0), rows, D, eps, _stream())
    return out


def gated_gelu(ab: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = gelu_new(ab[m, n]) * ab[m, F + n]; ab [M, 2F]."""
    dt = _act(ab, "ab")
    M, F2 = ab.shape
    out = torch.empty(M, F2 // 2, dtype=dt, device=ab.device) if out is None else out
    _chk(out, "out", dt)
    assert F2 % 2 == 0 and out.shape == (M, F2 // 2)
    _call("ug_gated_gelu", dt, ab.data_ptr(), ab.stride(0), out.data_ptr(), out.stride(0), M, F2 // 2, _stream())
    return out


def quick_gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x * sigmoid(1.702 x), contiguous; out may be x itself."""
    dt = _act(x, "x")
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", dt)
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel()
    _call("ug_quick_gelu", dt, x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def gelu_erf(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """0.5 x (1 + erf(x / sqrt 2)), contiguous; out may be x itself."""
    dt = _act(x, "x")
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", dt)
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel()
    _call("ug_gelu_erf", dt, x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


# ---- image front end (csrc/image.hip): uint8 NHWC [B, H, W, C] tensors, byte strides per sample and per row -------------------------------------------
u8 = torch.uint8


def _img(x: torch.Tensor, name: str, channels=(1, 3)):
    """-> (B, H, W, C, sample stride, row stride) of a uint8 [B, H, W, C] GPU tensor whose pixels are contiguous within a row."""
    if not x.is_cuda:
        raise L.UniGenHipError(f"{name}: expected a GPU tensor (unigen_amd has no CPU path)")
    if x.dtype != u8 or x.dim() != 4:
        raise TypeError(f"{name}: expected a uint8 [B, H, W, C] tensor, got {x.dtype} {tuple(x.shape)}")
    B, H, W, Cc = x.shape
    if Cc not in channels:
        raise ValueError(f"{name}: {Cc} channels (expected one of {channels})")
    if (Cc > 1 and x.stride(3) != 1) or (W > 1 and x.stride(2) != Cc):
        raise ValueError(f"{name}: the pixels of a row must be contiguous (strides {x.stride()})")
    return B, H, W, Cc, x.stride(0), x.stride(1)


def canny_grad(x: torch.Tensor):
    """Stage 1 of Canny -> (dx int16, dy int16, mag int32), each [B, H, W]."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    dx, dy = torch.empty(B, H, W, dtype=torch.int16, device=x.device), torch.empty(B, H, W, dtype=torch.int16, device=x.device)
    mag = torch.empty(B, H, W, dtype=torch.int32, device=x.device)
    L.call("ug_canny_grad", x.data_ptr(), sb, sr, B, H, W, Cc, dx.data_ptr(), dy.data_ptr(), mag.data_ptr(), _stream())
    return dx, dy, mag


def canny_nms(dx: torch.Tensor, dy: torch.Tensor, mag: torch.Tensor, low: int, high: int) -> torch.Tensor:
    """Stage 2 -> map uint8 [B, H, W]: 2 strong, 0 candidate, 1 not an edge."""
    _chk(dx, "dx", torch.int16); _chk(dy, "dy", torch.int16); _chk(mag, "mag", torch.int32)
    assert dx.is_contiguous() and dy.is_contiguous() and mag.is_contiguous() and dx.shape == dy.shape == mag.shape and dx.dim() == 3
    B, H, W = dx.shape
    out = torch.empty(B, H, W, dtype=u8, device=dx.device)
    L.call("ug_canny_nms", dx.data_ptr(), dy.data_ptr(), mag.data_ptr(), B, H, W, low, high, out.data_ptr(), _stream())
    return out


def canny_max_sweeps(H: int, W: int) -> int:
    return int(L.load().ug_canny_max_sweeps(H, W))


def canny_hysteresis(emap: torch.Tensor):
    """Stage 3 on a copy of `emap` -> (edges uint8 [B, H, W] 255 / 0, sweeps). Synchronises the stream once per sweep."""
    _chk(emap, "emap", u8)
    assert emap.dim() == 3
    B, H, W = emap.shape
    work = emap.contiguous().clone()
    out = torch.empty(B, H, W, dtype=u8, device=emap.device)
    flag = torch.zeros(1, dtype=torch.int32, device=emap.device)
    sweeps = C.c_int32(0)
    L.call("ug_canny_hysteresis", work.data_ptr(), B, H, W, out.data_ptr(), H * W, W, flag.data_ptr(), C.byref(sweeps), _stream())
    return out, sweeps.value


def canny_u8(x: torch.Tensor, low: int = 100, high: int = 200):
    """cv2.Canny(x, low, high) per image of a uint8 [B, H, W, C] batch -> (edges uint8 [B, H, W], sweeps of the hysteresis)."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    lib = L.load()
    ws = torch.empty(int(lib.ug_canny_workspace_bytes(B, H, W)), dtype=u8, device=x.device)
    out = torch.empty(B, H, W, dtype=u8, device=x.device)
    sweeps = C.c_int32(0)
    L.call("ug_canny_u8", x.data_ptr(), sb, sr, B, H, W, Cc, low, high, out.data_ptr(), H * W, W, ws.data_ptr(), ws.numel(), C.byref(sweeps), _stream())
    return out, sweeps.value


def img_resize_u8(x: torch.Tensor, height: int, width: int, xtables=None, ytables=None) -> torch.Tensor:
    """PIL's 8-bit resampling with host-built tables (unigen_amd.image.resample_tables, on the device): `xtables` / `ytables` = (bounds int32 [out, 2],
    coef int32 [out, k], k) of the pass that changes the width / the height, None for a pass that is skipped."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    if (xtables is None) != (W == width) or (ytables is None) != (H == height):
        raise ValueError("img_resize_u8: tables are needed for exactly the passes whose size changes")
    for t, n in ((xtables, width), (ytables, height)):
        if t is not None:
            _chk(t[0], "bounds", torch.int32); _chk(t[1], "coef", torch.int32)
            assert t[0].is_contiguous() and t[1].is_contiguous() and tuple(t[0].shape) == (n, 2) and tuple(t[1].shape) == (n, t[2])
    out = torch.empty(B, height, width, Cc, dtype=u8, device=x.device)
    tmp = torch.empty(B, H, width, Cc, dtype=u8, device=x.device) if (xtables is not None and ytables is not None) else None
    xb, xc, xk = (xtables[0].data_ptr(), xtables[1].data_ptr(), xtables[2]) if xtables is not None else (None, None, 0)
    yb, yc, yk = (ytables[0].data_ptr(), ytables[1].data_ptr(), ytables[2]) if ytables is not None else (None, None, 0)
    L.call("ug_img_resize_u8", x.data_ptr(), sb, sr, B, H, W, Cc, out.data_ptr(), height * width * Cc, width * Cc, height, width, xb, xc, xk, yb, yc, yk,
           _p(tmp), _stream())
    return out


def img_rgb_to_l(x: torch.Tensor) -> torch.Tensor:
    """PIL's convert("L"): [B, H, W, 3] -> [B, H, W, 1]."""
    B, H, W, Cc, sb, sr = _img(x, "x", channels=(3,))
    out = torch.empty(B, H, W, 1, dtype=u8, device=x.device)
    L.call("ug_img_rgb_to_l", x.data_ptr(), sb, sr, B, H, W, out.data_ptr(), H * W, W, _stream())
    return out


def _img_dt(dtype) -> int:
    if dtype not in (bf16, f32):
        raise TypeError(f"image tensors are torch.float32 or torch.bfloat16, got {dtype}")
    return L.UG_DT_F32 if dtype == f32 else L.UG_DT_BF16


def img_u8_to_chw(x: torch.Tensor, normalize: bool = True, dtype=f32, replicate: bool = False) -> torch.Tensor:
    """uint8 [B, H, W, C] -> `dtype` [B, C, H, W] as 2 (v / 255) - 1 (or v / 255); `replicate` turns a gray image into three equal channels."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    cout = 3 if (replicate and Cc == 1) else Cc
    out = torch.empty(B, cout, H, W, dtype=dtype, device=x.device)
    L.call("ug_img_u8_to_chw", x.data_ptr(), sb, sr, B, H, W, Cc, out.data_ptr(), _img_dt(dtype), cout, int(bool(normalize)), _stream())
    return out


def img_chw_to_u8(x: torch.Tensor, denormalize: bool = True) -> torch.Tensor:
    """fp32 / bf16 [B, C, H, W] -> uint8 [B, H, W, C] with diffusers' rounding points (denormalize, clamp, * 255, round half to even)."""
    if not x.is_cuda:
        raise L.UniGenHipError("x: expected a GPU tensor (unigen_amd has no CPU path)")
    if x.dim() != 4 or not 1 <= x.shape[1] <= 4:
        raise ValueError(f"x: expected [B, C <= 4, H, W], got {tuple(x.shape)}")
    dt = _img_dt(x.dtype)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty(B, H, W, Cc, dtype=u8, device=x.device)
    L.call("ug_img_chw_to_u8", x.data_ptr(), dt, B, Cc, H, W, out.data_ptr(), H * W * Cc, W * Cc, int(bool(denormalize)), _stream())
    return out


def img_box_blur_u8(x: torch.Tensor, cx, cy, passes: int = 1, fuse: bool = True) -> torch.Tensor:
    """PIL's box blur of a uint8 [B, H, W, C] batch: `passes` passes along rows with the constants cx = (r, ww, fw), then along columns with cy
    (unigen_amd.image.box_blur_constants; those of radius 0 skip the axis). passes = 3 with the box radius of `gaussian_box_radius` is PIL's
    GaussianBlur. `fuse=False` forces one launch per pass."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    lib = L.load()
    ws = torch.empty(int(lib.ug_img_blur_workspace_bytes(B, H, W, Cc)), dtype=u8, device=x.device)
    out = torch.empty(B, H, W, Cc, dtype=u8, device=x.device)
    L.call("ug_img_box_blur_u8", x.data_ptr(), sb, sr, B, H, W, Cc, out.data_ptr(), H * W * Cc, W * Cc, *(int(v) for v in cx), *(int(v) for v in cy),
           int(passes), int(bool(fuse)), ws.data_ptr(), ws.numel(), _stream())
    return out


# ---- depth condition (csrc/depth.hip): the glue of Depth Anything that is neither a GEMM nor a convolution; activations NHWC ----------------------------
def img_u8_to_patches(x: torch.Tensor, patch: int, mean, std, rescale: float = 1 / 255, dtype=bf16, Kp: Optional[int] = None) -> torch.Tensor:
    """uint8 [B, H, W, C] (a strided view is fine) -> the rows [B * (H/P) * (W/P), Kp] of the patch-embedding GEMM in `dtype`, normalised as
    DPTImageProcessor does; Kp defaults to 3 P^2 rounded up to a multiple of 64, the pad columns are zero."""
    B, H, W, Cc, sb, sr = _img(x, "x")
    if dtype not in (bf16, f32):
        raise TypeError(f"dtype: torch.bfloat16 or torch.float32, got {dtype}")
    Kp = (3 * patch * patch + 63) // 64 * 64 if Kp is None else Kp
    if H % patch or W % patch:
        raise ValueError(f"image {H}x{W} is not a multiple of the patch size {patch}")
    out = torch.empty(B * (H // patch) * (W // patch), Kp, dtype=dtype, device=x.device)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _call("ug_img_u8_to_patches", dtype, x.data_ptr(), sb, sr, B, H, W, Cc, patch, float(rescale), m3, s3, out.data_ptr(), Kp, Kp, _stream())
    return out


def relu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x < 0 ? +0 : x (torch.relu's values: NaN propagates, -0 stays -0), contiguous, numel a multiple of 8; out may be x itself."""
    dt = _act(x, "x")
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", dt)
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel()
    _call("ug_relu", dt, x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def deconv_scatter_nhwc(prod: torch.Tensor, bias: torch.Tensor, *, B: int, h: int, w: int, f: int, Cout: int, Cp: int) -> torch.Tensor:
    """Second half of ConvTranspose2d(k = s = f): prod fp32 [B*h*w, f*f*Cout] (the GEMM against the weight laid out [(ky, kx, co)][Cin]) ->
    [B, h*f, w*f, Cp] in bias' dtype = rnd(prod + bias), zeros in the pad channels."""
    _chk(prod, "prod", f32)
    dt = _act(bias, "bias")
    assert prod.dim() == 2 and prod.shape[0] == B * h * w and prod.shape[1] >= f * f * Cout and bias.numel() == Cout and bias.is_contiguous()
    out = torch.empty(B, h * f, w * f, Cp, dtype=dt, device=prod.device)
    _call("ug_deconv_scatter_nhwc", dt, prod.data_ptr(), prod.stride(0), bias.data_ptr(), out.data_ptr(), B, h, w, f, Cout, Cp, _stream())
    return out


def bilinear_nhwc(x: torch.Tensor, Ho: int, Wo: int, align_corners: bool) -> torch.Tensor:
    """F.interpolate(mode="bilinear") of NHWC [B, H, W, C] (C a multiple of 8) to [B, Ho, Wo, C]."""
    dt = _act(x, "x")
    assert x.dim() == 4 and x.is_contiguous(), x.shape
    B, H, W, Cc = x.shape
    out = torch.empty(B, Ho, Wo, Cc, dtype=dt, device=x.device)
    _call("ug_bilinear_nhwc", dt, x.data_ptr(), B, H, W, Cc, out.data_ptr(), Ho, Wo, int(bool(align_corners)), _stream())
    return out


def depth_head_out(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, C_: int, max_depth: float = 1.0, metric: bool = False) -> torch.Tensor:
    """x [B, H, W, Cp] (channels [0, C_) used) -> fp32 [B, H, W] = act(bias + sum_c w[c] relu(x[c])) * max_depth; act is ReLU, or sigmoid if metric."""
    dt = _act(x, "x")
    _chk(w, "w", dt); _chk(bias, "bias", dt)
    assert x.dim() == 4 and x.is_contiguous() and w.is_contiguous() and w.numel() == C_ and bias.numel() == 1 and C_ <= x.shape[-1]
    B, H, W, Cp = x.shape
    out = torch.empty(B, H, W, dtype=f32, device=x.device)
    _call("ug_depth_head_out", dt, x.data_ptr(), B * H * W, C_, Cp, w.data_ptr(), bias.data_ptr(), float(max_depth), int(bool(metric)), out.data_ptr(),
          _stream())
    return out


def bicubic_f32(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """F.interpolate(mode="bicubic", align_corners=False) of fp32 [B, H, W] to [B, Ho, Wo]."""
    _chk(x, "x", f32)
    assert x.dim() == 3 and x.is_contiguous(), x.shape
    B, H, W = x.shape
    out = torch.empty(B, Ho, Wo, dtype=f32, device=x.device)
    L.call("ug_bicubic_f32", x.data_ptr(), B, H, W, out.data_ptr(), Ho, Wo, _stream())
    return out


def minmax_workspace_bytes(B: int, HW: int) -> int:
    return int(L.load().ug_minmax_workspace_bytes(B, HW))


def minmax_to_u8(d: torch.Tensor, channels: int = 1, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [B, H, W] -> uint8 [B, H, W, channels] (1 or 3 equal channels): per image uint8(trunc((d - min) / (max - min) * 255)); a constant image
    gives 0. `workspace`: a uint8 tensor of at least minmax_workspace_bytes(B, H * W), contents irrelevant."""
    _chk(d, "d", f32)
    assert d.dim() == 3 and d.is_contiguous(), d.shape
    B, H, W = d.shape
    ws = torch.empty(minmax_workspace_bytes(B, H * W), dtype=u8, device=d.device) if workspace is None else workspace
    _chk(ws, "workspace", u8)
    out = torch.empty(B, H, W, channels, dtype=u8, device=d.device)
    L.call("ug_minmax_to_u8", d.data_ptr(), B, H * W, out.data_ptr(), channels, ws.data_ptr(), ws.numel(), _stream())
    return out


# ---- Sana transformer block (csrc/sana.hip) ----
def linear_attn_workspace_bytes(batches: int, heads: int, N: int) -> int:
    return int(L.load().ug_linear_attn_workspace_bytes(batches, heads, N))


def linear_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, batches: int, heads: int, N: int, q_strides, k_strides,
                v_strides, o_strides, dh: int = 32, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ReLU linear attention (SanaLinearAttnProcessor2_0). q/k/v/out are base tensors (data_ptr = element [batch 0, row 0, head 0, 0]) and
    *_strides = (row_stride, batch_stride), as for flash_attn. `workspace`: a uint8 tensor of at least linear_attn_workspace_bytes(batches, heads, N),
    contents irrelevant; allocated per call when omitted."""
    dt = _act(q, "q")
    _chk(k, "k", dt); _chk(v, "v", dt); _chk(out, "out", dt)
    ws = torch.empty(linear_attn_workspace_bytes(batches, heads, N), dtype=u8, device=q.device) if workspace is None else workspace
    _chk(ws, "workspace", u8)
    if ws.numel() < linear_attn_workspace_bytes(batches, heads, N):
        raise ValueError(f"linear_attn: the workspace has {ws.numel()} bytes, {linear_attn_workspace_bytes(batches, heads, N)} are needed")
    ev = _timer.begin("linear_attn") if _timer is not None else None
    _call("ug_linear_attn", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0], v_strides[1],
          out.data_ptr(), o_strides[0], o_strides[1], batches, heads, N, dh, ws.data_ptr(), _stream())
    if ev is not None:
        _timer.end("linear_attn", 4.0 * batches * heads * N * dh * (dh + 1), ev, tag=(batches, heads, N))
    return out


def glu_dwconv3x3(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, *, B: int, H: int, W: int, C: int,
                  ldx: Optional[int] = None, ldo: Optional[int] = None) -> torch.Tensor:
    """out[..., c] = y[..., c] * silu(y[..., C + c]), y = dwconv3x3(silu(x)) + bias (the middle of GLUMBConv). x: rows of 2C channels per pixel (NHWC),
    w9 [9, 2C] (conv_depth.weight repacked tap-major), bias [2C]; out: rows of ldo >= C columns, the columns past C written as zeros."""
    dt = _act(x, "x")
    _chk(w9, "w9", dt); _chk(bias, "bias", dt); _chk(out, "out", dt)
    assert w9.is_contiguous() and tuple(w9.shape) == (9, 2 * C) and bias.numel() == 2 * C, (w9.shape, bias.shape, C)
    ev = _timer.begin("glu_dwconv") if _timer is not None else None
    _call("ug_glu_dwconv3x3", dt, x.data_ptr(), ldx if ldx is not None else x.stride(-2), w9.data_ptr(), bias.data_ptr(), out.data_ptr(),
          ldo if ldo is not None else out.stride(-2), B, H, W, C, _stream())
    if ev is not None:
        _timer.end("glu_dwconv", 2.0 * 9 * 2 * C * B * H * W, ev, tag=(B, H, W, C))
    return out


# ---- Sana backward (csrc/sana_bwd.hip) ----
def linear_attn_bwd_workspace_bytes(batches: int, heads: int, N: int) -> int:
    return int(L.load().ug_linear_attn_bwd_workspace_bytes(batches, heads, N))


def linear_attn_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dout: torch.Tensor, state: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor,
                    dv: torch.Tensor, *, batches: int, heads: int, N: int, q_strides, k_strides, v_strides, do_strides, dq_strides, dk_strides, dv_strides,
                    dh: int = 32, workspace: Optional[torch.Tensor] = None):
    """Backward of linear_attn. Base tensors and (row_stride, batch_stride) pairs as in the forward; `state`: the fp32 [batches * heads * 1056] values
    the forward left at the start of its workspace; dq / dk / dv may be the column blocks of one [M, 3 D] buffer. Returns (dq, dk, dv)."""
    dt = _act(q, "q")
    for t, n in ((k, "k"), (v, "v"), (dout, "dout"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        _chk(t, n, dt)
    _chk(state, "state", f32)
    if state.numel() < batches * heads * 1056 or not state.is_contiguous():
        raise ValueError(f"linear_attn_bwd: state has {state.numel()} floats, {batches * heads * 1056} contiguous ones are needed")
    need = linear_attn_bwd_workspace_bytes(batches, heads, N)
    ws = torch.empty(need, dtype=u8, device=q.device) if workspace is None else workspace
    _chk(ws, "workspace", u8)
    if ws.numel() < need:
        raise ValueError(f"linear_attn_bwd: the workspace has {ws.numel()} bytes, {need} are needed")
    ev = _timer.begin("linear_attn_bwd") if _timer is not None else None
    _call("ug_linear_attn_bwd", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0], v_strides[1],
          dout.data_ptr(), do_strides[0], do_strides[1], state.data_ptr(), dq.data_ptr(), dq_strides[0], dq_strides[1], dk.data_ptr(), dk_strides[0],
          dk_strides[1], dv.data_ptr(), dv_strides[0], dv_strides[1], batches, heads, N, dh, ws.data_ptr(), ws.numel(), _stream())
    if ev is not None:
        _timer.end("linear_attn_bwd", 12.0 * batches * heads * N * dh * (dh + 1), ev, tag=(batches, heads, N))
    return dq, dk, dv


def glu_dwconv3x3_bwd_workspace_bytes(B: int, H: int, W: int, C: int, dtype=bf16) -> int:
    return int(L.load().ug_glu_dwconv3x3_bwd_workspace_bytes(B, H, W, C, 2 if dtype == bf16 else 4))


def glu_dwconv3x3_bwd(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, dout: torch.Tensor, dx: torch.Tensor, *, B: int, H: int, W: int, C: int,
                      dw9: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, ldx: Optional[int] = None, lddo: Optional[int] = None,
                      lddx: Optional[int] = None, workspace: Optional[torch.Tensor] = None):
    """Backward of glu_dwconv3x3: x, w9, bias as in the forward, dout rows of lddo >= C columns -> dx rows of 2C (row stride lddx), and, when given,
    dw9 [9, 2C] / dbias [2C] fp32, fully reduced (both or neither). Returns (dx, dw9, dbias)."""
    dt = _act(x, "x")
    _chk(w9, "w9", dt); _chk(bias, "bias", dt); _chk(dout, "dout", dt); _chk(dx, "dx", dt)
    assert w9.is_contiguous() and tuple(w9.shape) == (9, 2 * C) and bias.numel() == 2 * C, (w9.shape, bias.shape, C)
    if (dw9 is None) != (dbias is None):
        raise ValueError("glu_dwconv3x3_bwd: dw9 and dbias are both given or both None")
    if dw9 is not None:
        _chk(dw9, "dw9", f32); _chk(dbias, "dbias", f32)
        assert dw9.is_contiguous() and tuple(dw9.shape) == (9, 2 * C) and dbias.is_contiguous() and dbias.numel() == 2 * C, (dw9.shape, dbias.shape)
    need = glu_dwconv3x3_bwd_workspace_bytes(B, H, W, C, dt)
    ws = torch.empty(need, dtype=u8, device=x.device) if workspace is None else workspace
    _chk(ws, "workspace", u8)
    if ws.numel() < need:
        raise ValueError(f"glu_dwconv3x3_bwd: the workspace has {ws.numel()} bytes, {need} are needed")
    ev = _timer.begin("glu_dwconv_bwd") if _timer is not None else None
    _call("ug_glu_dwconv3x3_bwd", dt, x.data_ptr(), ldx if ldx is not None else x.stride(-2), w9.data_ptr(), bias.data_ptr(), dout.data_ptr(),
          lddo if lddo is not None else dout.stride(-2), dx.data_ptr(), lddx if lddx is not None else dx.stride(-2), _p(dw9), _p(dbias), B, H, W, C,
          ws.data_ptr(), ws.numel(), _stream())
    if ev is not None:
        _timer.end("glu_dwconv_bwd", 2.0 * 9 * 2 * C * B * H * W * (3 if dw9 is not None else 2), ev, tag=(B, H, W, C))
    return dx, dw9, dbias


# ---- Gemma-2 text encoder (csrc/text.hip) ----------------------------------------------------------------------------------------------
def flash_attn_softcap(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, batches: int, heads: int, kv_heads: int, dh: int, L_: int,
                       q_strides, k_strides, v_strides, o_strides, scale: float, softcap: float = 0.0, window: int = 0,
                       kv_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention with grouped K/V heads (query head h reads K/V head h // (heads // kv_heads)), logits capped as softcap * tanh(s / softcap)
    (0: off), keys at or before q - window hidden (0: no window) and keys from kv_len[b] on hidden (kv_len int32 [batches] on the device, or None)."""
    dt = _act(q, "q")
    _chk(k, "k", dt); _chk(v, "v", dt); _chk(out, "out", dt)
    if kv_len is not None:
        _chk(kv_len, "kv_len", torch.int32)
        if kv_len.shape != (batches,) or not kv_len.is_contiguous():
            raise ValueError(f"kv_len: expected a contiguous int32 [batches = {batches}] tensor, got {tuple(kv_len.shape)}")
    ev = _timer.begin("attn") if _timer is not None else None
    _call("ug_flash_attn_fwd_softcap", dt, q.data_ptr(), q_strides[0], q_strides[1], k.data_ptr(), k_strides[0], k_strides[1], v.data_ptr(), v_strides[0],
          v_strides[1], out.data_ptr(), o_strides[0], o_strides[1], batches, heads, kv_heads, L_, dh, scale, softcap, window, _p(kv_len), _stream())
    if ev is not None:
        _timer.end("attn", 2.0 * batches * heads * L_ * L_ * dh, ev, tag=(batches, heads, L_, L_, dh))
    return out


def rope_half(buf: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, rows_per_batch: int, col0: int, nheads: int, dh: int) -> torch.Tensor:
    """Rotate-half RoPE in place on `nheads` consecutive dh-wide heads from column col0 of buf [rows, ld]; cos / sin [>= rows_per_batch, dh // 2] in
    buf's dtype, row r at position r % rows_per_batch."""
    dt = _act(buf, "buf")
    _chk(cos, "cos", dt); _chk(sin, "sin", dt)
    rows = buf.shape[0]
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[0] < rows_per_batch or cos.shape[1] != dh // 2 or not (cos.is_contiguous() and sin.is_contiguous()):
        raise ValueError(f"cos / sin: expected contiguous [>= {rows_per_batch}, {dh // 2}] tables, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    assert buf.dim() == 2 and buf.stride(1) == 1
    _call("ug_rope_half", dt, buf.data_ptr(), buf.stride(0), rows, rows_per_batch, col0, nheads, dh, cos.data_ptr(), sin.data_ptr(), _stream())
    return buf


def gemma_rmsnorm_rows(x: torch.Tensor, w: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gemma2RMSNorm over the last dimension of x [rows, D] (weight 1 + w, one rounding); with `residual` the sum residual + norm(x)."""
    dt = _act(x, "x")
    _chk(w, "w", dt)
    rows, D = x.shape
    out = torch.empty(rows, D, dtype=dt, device=x.device) if out is None else out
    _chk(out, "out", dt)
    assert w.numel() == D and out.shape == x.shape
    if residual is not None:
        _chk(residual, "residual", dt)
        assert residual.shape == x.shape
    _call("ug_gemma_rmsnorm_rows", dt, x.data_ptr(), x.stride(0), w.data_ptr(), _p(residual), residual.stride(0) if residual is not None else 0,
          out.data_ptr(), out.stride(0), rows, D, eps, _stream())
    return out


def gather_rows_scaled(src: torch.Tensor, idx: torch.Tensor, scale: float, out: torch.Tensor) -> torch.Tensor:
    """out[i] = src[idx[i]] * scale (zeros where idx[i] < 0); src [R, W], idx int32 [n], out [n, W]."""
    dt = _act(src, "src")
    _chk(idx, "idx", torch.int32); _chk(out, "out", dt)
    n, W = out.shape
    assert idx.numel() == n and src.shape[1] == W and idx.is_contiguous()
    _call("ug_gather_rows_scaled", dt, src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), n, W, scale, _stream())
    return out


# ---- DC-AE (csrc/dcae.hip; unigen_amd/dcae.py): NHWC activations as 2-D tensors [B * H * W, C] ----
def rmsnorm_bias_rows(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, eps: float, *, residual: Optional[torch.Tensor] = None, relu: bool = False,
                      out: Optional[torch.Tensor] = None, C_: Optional[int] = None) -> torch.Tensor:
    """RMSNorm with weight and bias over the first C_ (default: all) columns of x [rows, ld], one rounding; then + residual, or ReLU. out may be x
    or the residual."""
    dt = _act(x, "x")
    _chk(w, "w", dt); _chk(bias, "bias", dt)
    rows, Cc = x.shape[0], (x.shape[1] if C_ is None else C_)
    out = torch.empty(rows, Cc, dtype=dt, device=x.device) if out is None else out
    _chk(out, "out", dt)
    assert w.numel() == Cc and bias.numel() == Cc and out.shape[0] == rows
    if residual is not None:
        _chk(residual, "residual", dt)
        assert residual.shape[0] == rows
    _call("ug_rmsnorm_bias_rows", dt, x.data_ptr(), x.stride(0), w.data_ptr(), bias.data_ptr(), _p(residual), residual.stride(0) if residual is not None else 0,
          out.data_ptr(), out.stride(0), rows, Cc, eps, 1 if relu else 0, _stream())
    return out


def msconv_proj(x: torch.Tensor, w_dw: torch.Tensor, w_pw: torch.Tensor, out: torch.Tensor, *, B: int, H: int, W: int, G: int, k: int = 5) -> torch.Tensor:
    """One scale of SanaMultiscaleAttentionProjection: depthwise k x k (w_dw [k*k, G*32], tap-major) then the grouped 1x1 (w_pw [G, 32, 32]) over the
    first G * 32 columns of x [B*H*W, ld] into those of out [B*H*W, ld']."""
    dt = _act(x, "x")
    _chk(w_dw, "w_dw", dt); _chk(w_pw, "w_pw", dt); _chk(out, "out", dt)
    assert w_dw.is_contiguous() and tuple(w_dw.shape) == (k * k, G * 32) and w_pw.is_contiguous() and w_pw.numel() == G * 32 * 32, (w_dw.shape, w_pw.shape, G, k)
    assert x.shape[0] == B * H * W and out.shape[0] == B * H * W
    ev = _timer.begin("msconv") if _timer is not None else None
    _call("ug_msconv_proj", dt, x.data_ptr(), x.stride(0), w_dw.data_ptr(), w_pw.data_ptr(), out.data_ptr(), out.stride(0), B, H, W, G, k, _stream())
    if ev is not None:
        _timer.end("msconv", 2.0 * (k * k + 32) * G * 32 * B * H * W, ev, tag=(B, H, W, G, k))
    return out


def dc_shortcut(h: torch.Tensor, out: torch.Tensor, *, up: bool, B: int, H: int, W: int, Cin: int, Cout: int, factor: int, x: Optional[torch.Tensor] = None,
                x_shuffle: bool = False) -> torch.Tensor:
    """The non-parametric DC-AE shortcut of h [B*H*W, ld] (pixel-unshuffle + group mean, or channel repeat + pixel-shuffle), plus x where given;
    x_shuffle: x has h's pixel grid and is rearranged as h is. H, W are h's."""
    dt = _act(h, "h")
    _chk(out, "out", dt)
    if x is not None:
        _chk(x, "x", dt)
    assert h.shape[0] == B * H * W and out.shape[0] == (B * H * W * factor * factor if up else B * (H // factor) * (W // factor)), (h.shape, out.shape)
    assert x is None or x.shape[0] == (h.shape[0] if x_shuffle else out.shape[0])
    _call("ug_dc_shortcut_up" if up else "ug_dc_shortcut_down", dt, h.data_ptr(), h.stride(0), _p(x), x.stride(0) if x is not None else 0, 1 if x_shuffle else 0,
          out.data_ptr(), out.stride(0), B, H, W, Cin, Cout, factor, _stream())
    return out


def silu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(x) on a contiguous tensor, numel a multiple of 8; out may be x itself."""
    dt = _act(x, "x")
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", dt)
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel()
    _call("ug_silu", dt, x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out
