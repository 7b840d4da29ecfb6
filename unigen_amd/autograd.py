"""torch.autograd.Function wrappers of the HIP hot ops: the second caller of the forward (reference train.py:622-662:
`accelerator.backward(loss)` through the same transformer). torch.autograd is the tape (as it is in the reference); every matrix product of the
backward is ug_gemm_bf16 again - dX = dY W through a transposed copy of W, dW = dY^T X through transposed copies of dY and X, and the attention
backward as five grouped GEMMs per sample around the elementwise kernels of csrc/backward.hip. fp32 tensors select the `_f32` verification twins,
as in the forward. There is no CPU path."""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import lib as L
from . import ops

_wt_cache: dict = {}


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def _w_transposed(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> [K, N] (N must be a multiple of 64: it becomes the contraction length). Frozen weights are transposed once."""
    if w.requires_grad:
        return ops.transpose(w.detach())
    # the entry pins the STORAGE (a detached alias, not the Parameter object: `p.data = new_buffer` - engine._pack, nn.Module._apply - would
    # free the old storage under a pinned Parameter and let another weight of the same shape land on its address), so the address cannot be
    # recycled while the entry exists; `_version` catches in-place updates (load_state_dict, optimizer steps on a formerly frozen weight).
    # Re-pointing also calls clear_caches() (engine._pack / _pack_stack), which drops the dead transposed copies.
    key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), w.dtype, w._version)
    hit = _wt_cache.get(key)
    if hit is None:
        if len(_wt_cache) > 4096:
            _wt_cache.clear()
        hit = _wt_cache[key] = (ops.transpose(w.detach()), w.detach())
    return hit[0]


def evict_weight(w: torch.Tensor) -> None:
    """Drop the cached transposes of every frozen weight that lives in w's storage: for a buffer that is rewritten in place (unigen_amd/sana.py
    rebuilds a packed copy into its buffer after an optimizer step). The new version counter would miss the old entries, which would stay and
    pin a dead transpose each."""
    st = w.untyped_storage()
    lo, hi = st.data_ptr(), st.data_ptr() + st.nbytes()
    for k in [k for k in _wt_cache if lo <= k[0] < hi]:
        del _wt_cache[k]


def clear_caches() -> None:
    """Drop EVERY cached transpose (frozen weights and recent activations). Only for when parameters are re-pointed at new storage
    (engine._pack / _pack_stack / _apply call it); a training loop must NOT call this per step - every frozen weight would be re-transposed
    each step - it calls clear_activation_cache()."""
    _wt_cache.clear()
    _xt_cache.clear()


def clear_activation_cache() -> None:
    """Drop the (up to 4) activation transposes of the last backward and the source tensors they pin - hundreds of MB at full size that would
    otherwise outlive the step. Call after `loss.backward()` (tools/train_bench.py, tests/fullsize_train_parity.py do); the frozen-weight
    transposes stay."""
    _xt_cache.clear()


_xt_cache: list = []        # the last few activation transposes of this backward pass: (source tensor, padded length, transposed copy)


def _x_transposed(x: torch.Tensor, Mp: int) -> torch.Tensor:
    """X^T for wgrad. to_q / to_k / to_v (+ proj_mlp), the added projections and the expert linears read the same input: their backward nodes
    run back to back, so a 4-entry cache removes most of the repeated transposes. Entries pin their source (no address reuse while cached)."""
    for src, mp, xt in _xt_cache:
        if src.data_ptr() == x.data_ptr() and src.shape == x.shape and src._version == x._version and mp == Mp and src.stride() == x.stride():
            return xt
    xt = ops.transpose(x, Mp)
    _xt_cache.append((x, Mp, xt))
    if len(_xt_cache) > 4:
        _xt_cache.pop(0)
    return xt


def _dgrad(dy: torch.Tensor, wt: torch.Tensor, acc: Optional[torch.Tensor] = None, lora_t=None, lora_b=None) -> torch.Tensor:
    """dY [M, N] times a transposed weight wt [K, N] -> [M, K] (dX = dY W): into a fresh buffer, optionally with the K-segment lora_t lora_b^T in
    the same accumulator, or added to `acc` in place through the GEMM's residual epilogue (every element is read and written by one lane; the same
    bf16 sums autograd would form with separate add kernels)."""
    M, N = dy.shape
    if N % 64 != 0:
        raise L.UniGenHipError(f"linear backward: out_features={N} must be a multiple of 64 (it is the contraction length of dX = dY W)")
    if acc is None:
        return ops.gemm(dy, wt, None, torch.empty(M, wt.shape[0], device=dy.device, dtype=dy.dtype), M=M, lora_t=lora_t, lora_b=lora_b)
    return ops.gemm(dy, wt, None, acc, M=M, epilogue=L.EPI_RES_SCALE, residual=acc, alpha=1.0)


def _wgrad(dy: torch.Tensor, xs) -> torch.Tensor:
    """dW = dY^T [x_0 | x_1 | ...] -> [N, sum K_j], one GEMM per column block, through transposed copies of dY and the x_j (also what the fp32
    verification path runs). A transposed-operand kernel (dY^T X straight from the row-major operands, tools/probe: csrc/gemm_tn.hip) measured
    6 % SLOWER per step than this (0.884 vs 0.832 s backward at B = 2): probe library only."""
    M, N = dy.shape
    Mp = _pad64(M)
    dyt = ops.transpose(dy, Mp)                                            # [N, Mp]; the x_j become [K_j, Mp]
    dw = torch.empty(N, sum(x.shape[1] for x in xs), device=dy.device, dtype=dy.dtype)
    c0 = 0
    for x in xs:                                                           # ldc = dw's row stride, K_j columns from column c0
        ops.gemm(dyt, _x_transposed(x, Mp), None, dw[:, c0:] if c0 else dw, M=N)
        c0 += x.shape[1]
    return dw


def _bgrad(dy: torch.Tensor) -> torch.Tensor:
    return ops.colsum(dy).view(dy.shape[1])


def _rows(x: torch.Tensor) -> torch.Tensor:
    return x.reshape(-1, x.shape[-1]).contiguous()


def _adjacent(ts) -> bool:
    """The tensors are consecutive row blocks of one contiguous buffer (the packed QKV / QKV+MLP weights of engine._pack)."""
    for a, b in zip(ts[:-1], ts[1:]):
        if a is None or b is None or not a.is_contiguous() or not b.is_contiguous() or a.dtype != b.dtype:
            return False
        if b.data_ptr() != a.data_ptr() + a.numel() * a.element_size() or a.shape[1:] != b.shape[1:]:
            return False
        if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():      # neighbours by the allocator's choice, not views of one buffer
            return False
    return ts[0] is not None and ts[0].is_contiguous()


class Projection(torch.autograd.Function):
    """n >= 1 Linear layers that read the SAME rows x (one projection; to_q | to_k | to_v [| proj_mlp] of an attention block), optionally with live
    LoRA adapters:  y_i = x w_i^T + b_i [+ T B_bd[rows of i]^T,  T = bf16(x A_cat^T)]. ONE ug_gemm_bf16 over the packed weights when the parameters
    sit back to back in memory (engine._pack re-points them so), n GEMMs into the column blocks of one buffer otherwise. Returns the n column
    blocks as views. `a_cat` [Rp, K] / `b_bd` [sum N_i, Rp] are the fused operands of lora.fuse_adapters_autograd (differentiable: torch.autograd
    carries their gradients on to every adapter's own lora_A / lora_B), or None; `has` [n]: whether projection i carries a live adapter (its rows
    of b_bd are non-zero). With adapters the forward is the inference engine's (HipModule._lora_gemm: T, then the K-segment launch): the same two
    launches, the same rounding points.
    Backward: dx = sum_i dy_i w_i [+ dT A_cat] accumulates through the GEMM's residual epilogue (dy_1 W_1, then R + dy_2 W_2, ...), the adapter
    term as the K-segment of the first launch; d w_i = dy_i^T x with ONE transposed copy of x. dT = sum_i dy_i B_bd[rows of i] (the projections'
    rank columns are disjoint, so accumulating adds exact zeros); dA_cat = dT^T x and dB_bd[rows of i] = (T^T dy_i)^T through ug_lora_wgrad - no
    transposed copy of x or dy unless a base weight itself is trainable."""

    @staticmethod
    def forward(ctx, x, n, has, a_cat, b_bd, *wb):
        ws, bs = wb[:n], wb[n:]
        M, K = x.shape
        Ns = [w.shape[0] for w in ws]
        has_b = [b is not None for b in bs]
        t = None
        if a_cat is not None:
            t = ops.gemm(x, a_cat, None, torch.empty(M, a_cat.shape[0], device=x.device, dtype=x.dtype), M=M)
        out = torch.empty(M, sum(Ns), device=x.device, dtype=x.dtype)
        if n > 1 and _adjacent(ws) and (all(has_b) and _adjacent([b.view(-1, 1) for b in bs]) or not any(has_b)):
            wp = torch.as_strided(ws[0], (sum(Ns), K), (K, 1))
            bp = torch.as_strided(bs[0], (sum(Ns),), (1,)) if has_b[0] else None
            ops.gemm(x, wp, bp, out, M=M, lora_t=t, lora_b=b_bd)
        else:                                                    # (one projection: its launch is the packed launch)
            c0 = 0
            for w, b, N, h in zip(ws, bs, Ns, has):              # ldc = the buffer's row stride, N columns from column c0
                ops.gemm(x, w, b, out[:, c0:] if c0 else out, M=M, lora_t=t if h else None, lora_b=b_bd[c0:c0 + N] if h else None)
                c0 += N
        ctx.save_for_backward(x, t, a_cat, b_bd, *ws)
        ctx.Ns, ctx.has, ctx.has_b = Ns, has, has_b
        return (out,) if n == 1 else out.split(Ns, 1)

    @staticmethod
    def backward(ctx, *dys):
        saved = ctx.saved_tensors            # ONE access: under torch.utils.checkpoint a second unpack of the same tensors is an error
        x, t, a_cat, b_bd, ws = saved[0], saved[1], saved[2], saved[3], saved[4:]
        n, need = len(ws), ctx.needs_input_grad                  # inputs: x, n, has, a_cat, b_bd, n weights, n biases
        dys = [None if dy is None else dy.contiguous() for dy in dys]
        d_t, live = None, [i for i in range(n) if ctx.has[i] and dys[i] is not None]
        if live:
            rows = [slice(sum(ctx.Ns[:i]), sum(ctx.Ns[:i + 1])) for i in range(n)]
            if need[0] or need[3]:
                for i in live:
                    d_t = _dgrad(dys[i], ops.transpose(b_bd[rows[i]].detach()), d_t)                 # B_bd block transposed: [Rp, N_i]
        dx = da = db = None
        dws, dbs = [None] * n, [None] * n
        for i, dy in enumerate(dys):
            if dy is None:
                continue
            if need[0] and dx is None and d_t is not None:        # dy_i w_i + dT A_cat in one accumulator (lora_b [K, Rp] = A_cat^T)
                dx = _dgrad(dy, _w_transposed(ws[i]), lora_t=d_t, lora_b=ops.transpose(a_cat.detach()))
            elif need[0]:
                dx = _dgrad(dy, _w_transposed(ws[i]), dx)
            if need[5 + i]:
                dws[i] = _wgrad(dy, [x])
            if ctx.has_b[i] and need[5 + n + i]:
                dbs[i] = _bgrad(dy)
        if need[3] and d_t is not None:
            da = ops.lora_wgrad(d_t, x)
        if need[4] and live:
            dbt = (torch.empty if len(live) == n else torch.zeros)(a_cat.shape[0], sum(ctx.Ns), device=x.device, dtype=x.dtype)
            for i in live:
                ops.lora_wgrad(t, dys[i], dbt[:, rows[i]])
            db = dbt.t()                                          # produced as [Rp, N] (ug_lora_wgrad's orientation), viewed as [N, Rp]
        return (dx, None, None, da, db, *dws, *dbs)


def _project(x: torch.Tensor, ws, bs, lora):
    a_cat, b_bd, has = lora if lora is not None else (None, None, (False,) * len(ws))
    return Projection.apply(_rows(x), len(ws), has, a_cat, b_bd, *ws, *bs)


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], lora=None) -> torch.Tensor:
    """F.linear(x, w, b); `lora`: the (a_cat, b_bd, has) triple of HipModule._lora_autograd when adapters are live on the projection, or None."""
    return _project(x, [w], [b], lora)[0].view(*x.shape[:-1], w.shape[0])


def linear_n(x: torch.Tensor, ws, bs, lora=None):
    """[F.linear(x, w_i, b_i) for i]: x [..., K] -> views [..., N_i] of one buffer; `lora` as in linear()."""
    lead = x.shape[:-1]
    return [o.unflatten(0, lead) if len(lead) != 1 else o for o in _project(x, ws, bs, lora)]


class LinearResScale(torch.autograd.Function):
    """r + alpha * F.linear(x, w, b) on [M, K] rows - the zero-res projections `x + controlnet_add_*(z) * conditioning_scale`
    (src/UniGenTransformer.py:1104,1141,1166) - as ONE ug_gemm_bf16 with the UG_EPI_RES_SCALE epilogue (the rounding points of the three torch
    ops: Linear output, * alpha, + r each a bf16 tensor). Backward: d r = d y; d(lin) = alpha * d y, then a Linear's two GEMMs and a column sum."""

    @staticmethod
    def forward(ctx, r, x, w, b, alpha):
        M, K = x.shape
        N = w.shape[0]
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
        ops.gemm(x, w, b, out, M=M, epilogue=L.EPI_RES_SCALE, residual=r, alpha=float(alpha))
        ctx.save_for_backward(x, w)
        ctx.has_bias, ctx.alpha = b is not None, float(alpha)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        du = dy if ctx.alpha == 1.0 else (dy * ctx.alpha)
        return (dy if need[0] else None, _dgrad(du, _w_transposed(w)) if need[1] else None, _wgrad(du, [x]) if need[2] else None,
                _bgrad(du) if ctx.has_bias and need[3] else None, None)


def linear_res_scale(r: torch.Tensor, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], alpha: float) -> torch.Tensor:
    """r + alpha * linear(x): r [..., N], x [..., K] with equal leading dims."""
    return LinearResScale.apply(_rows(r), _rows(x), w, b, alpha).view(*x.shape[:-1], w.shape[0])


class LinearCat2(torch.autograd.Function):
    """F.linear(torch.cat([a, m], -1), w, b) WITHOUT the concatenation - the single block's proj_out over [attention | gelu(mlp)]
    (diffusers FluxSingleTransformerBlock, called at src/UniGenTransformer.py:1151): the m columns run as the K-segment extension of ug_gemm_bf16
    (the LoRA segment: T = m, B = w[:, Ka:]), one kernel, one fp32 accumulation in the concatenated K order -> the same bits as the GEMM over the
    materialised [M, Ka + Km] tensor. Backward: d a and d m as two GEMMs into their own buffers, d w column block by column block."""

    @staticmethod
    def forward(ctx, a, m, w, b):
        M, Ka = a.shape
        N = w.shape[0]
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
        ops.gemm(a, w[:, :Ka], b, out, M=M, lora_t=m, lora_b=w[:, Ka:])
        ctx.save_for_backward(a, m, w)
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        a, m, w = ctx.saved_tensors
        need, Ka = ctx.needs_input_grad, a.shape[1]
        dy = dy.contiguous()
        wt = _w_transposed(w) if need[0] or need[1] else None             # [Ka + Km, N]: row blocks are the transposed column blocks of w
        return (_dgrad(dy, wt[:Ka]) if need[0] else None, _dgrad(dy, wt[Ka:]) if need[1] else None, _wgrad(dy, [a, m]) if need[2] else None,
                _bgrad(dy) if ctx.has_bias and need[3] else None)


def linear_cat2(a: torch.Tensor, m: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], lora=None) -> torch.Tensor:
    """With adapters on the projection the GEMM's one K-segment is taken by them (as in the inference engine, whose [attention | mlp] operand is
    one buffer), so the concatenation is materialised; same bits as linear_cat2 + the adapter term."""
    if lora is not None:
        return linear(torch.cat([a, m], dim=-1), w, b, lora)
    return LinearCat2.apply(_rows(a), _rows(m), w, b).view(*a.shape[:-1], w.shape[0])


class MoeGate(torch.autograd.Function):
    """gates = softmax(F.linear((x + c).float(), wg.float())) [S, E] fp32 and the arg-max expert per token: ug_moe_gate_top1 forward,
    ug_moe_gate_bwd backward (deepspeed TopKGate, src/UniGenUtils.py:99). top_k = 2 (top2gating): ug_moe_gate_top2, idx [2, S] with the second
    choice drawn through `noise` (the Gumbel sample added to the logits). idx is not differentiable, and neither is the noised arg-max.
    Third output: the fp32 logits [S, E] for top_k > 2 (topkgating's capacity rule ranks them; not differentiable), an empty tensor otherwise."""

    @staticmethod
    def forward(ctx, x, c, wg, top_k=1, noise=None):
        S, D = x.shape
        E = wg.shape[0]
        gates = torch.empty(S, E, device=x.device, dtype=torch.float32)
        wgc = wg.contiguous()
        if top_k == 1:
            idx = torch.empty(S, device=x.device, dtype=torch.int32)
            ops.moe_gate_top1(x, c, wgc, gates, idx)
        elif top_k == 2:
            idx = torch.empty(2, S, device=x.device, dtype=torch.int32)
            ops.moe_gate_top2(x, c, wgc, noise, gates, idx)
        else:                                    # topkgating: idx [K, S]
            idx = torch.empty(top_k, S, device=x.device, dtype=torch.int32)
            logits = torch.empty(S, E, device=x.device, dtype=torch.float32)
            ops.moe_gate_topk(x, c, wgc, top_k, gates, logits, idx)
        if top_k <= 2:
            logits = torch.empty(0, device=x.device, dtype=torch.float32)
        ctx.save_for_backward(gates, x, c, wgc)
        ctx.mark_non_differentiable(idx, logits)
        return gates, idx, logits

    @staticmethod
    def backward(ctx, dgates, _didx, _dlogits):
        gates, x, c, wg = ctx.saved_tensors
        dxc, dwg = ops.moe_gate_bwd(gates, dgates.float().contiguous(), x, c, wg)
        return (dxc if ctx.needs_input_grad[0] else None), (dxc if ctx.needs_input_grad[1] else None), (dwg if ctx.needs_input_grad[2] else None), None, None


class GeluTanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.gelu_tanh(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.gelu_tanh_bwd(x, dy)


class AdaLNModulate(torch.autograd.Function):
    """LayerNorm(x; eps, no affine) * (1 + scale[:, None]) + shift[:, None]: x [B, L, D], shift / scale [B, D]."""

    @staticmethod
    def forward(ctx, x, shift, scale, eps):
        B, Ls, D = x.shape
        x2 = x.reshape(B * Ls, D).contiguous()
        shift, scale = shift.contiguous(), scale.contiguous()
        out = torch.empty(B * Ls, D, device=x.device, dtype=x.dtype)
        ops.adaln_modulate(x2, shift, scale, out, rows=B * Ls, D=D, rows_per_sample=Ls, mod_ld=D, eps=eps)
        ctx.save_for_backward(x2, scale)
        ctx.geom, ctx.eps = (B, Ls, D), eps
        return out.view(B, Ls, D)

    @staticmethod
    def backward(ctx, dy):
        x2, scale = ctx.saved_tensors
        B, Ls, D = ctx.geom
        dy2 = dy.reshape(B * Ls, D).contiguous()
        dx, dshift, dscale = ops.adaln_modulate_bwd(x2, dy2, scale, rows_per_sample=Ls, eps=ctx.eps)
        return dx.view(B, Ls, D), dshift, dscale, None


def adaln_modulate(x, shift, scale, eps: float = 1e-6):
    return AdaLNModulate.apply(x, shift, scale, eps)


class GateResidual(torch.autograd.Function):
    """x + gate.unsqueeze(1) * a (x, a [B, L, D]; gate [B, D]) as one kernel; backward: d x = d y, d a = gate * d y, d gate = sum_rows(d y * a)."""

    @staticmethod
    def forward(ctx, x, a, gate):
        B, Ls, D = a.shape
        a2, g2 = a.reshape(B * Ls, D).contiguous(), gate.contiguous()
        y = ops.gate_residual(x.reshape(B * Ls, D).contiguous(), a2, g2, Ls)
        ctx.save_for_backward(a2, g2)
        ctx.geom = (B, Ls, D)
        return y.view(B, Ls, D)

    @staticmethod
    def backward(ctx, dy):
        a2, g2 = ctx.saved_tensors
        B, Ls, D = ctx.geom
        dy2 = dy.reshape(B * Ls, D).contiguous()
        da = ops.gate_residual(None, dy2, g2, Ls).view(B, Ls, D) if ctx.needs_input_grad[1] else None
        dg = ops.colsum(dy2, a2, rows_per_group=Ls) if ctx.needs_input_grad[2] else None
        return dy, da, dg


def gate_residual(x, a, gate):
    return GateResidual.apply(x, a, gate)


class QKNormRope(torch.autograd.Function):
    """RMSNorm over each head (weight w [dh] or None) followed by apply_rotary_emb (cos / sin [positions, dh] fp32 or None) of one of q / k:
    x [B, L, H * dh]; row l of a sample sits at position pos_offset + l."""

    @staticmethod
    def forward(ctx, x, w, cos, sin, heads, pos_offset, eps):
        B, Ls, HD = x.shape
        dh = HD // heads
        out = x.reshape(B * Ls, HD).clone()
        ops.qk_rmsnorm_rope(out, batches=B, rows_per_batch=Ls, ld=HD, q_off=-1, k_off=0, heads=heads, dh=dh, pos_offset=pos_offset, wk_b=w, split=0,
                            cos=cos, sin=sin, eps=eps)
        ctx.save_for_backward(x.reshape(B * Ls, HD), w, cos, sin)
        ctx.geom = (B, Ls, heads, dh, pos_offset, eps)
        return out.view(B, Ls, HD)

    @staticmethod
    def backward(ctx, dy):
        x2, w, cos, sin = ctx.saved_tensors
        B, Ls, heads, dh, pos_offset, eps = ctx.geom
        dy2 = dy.reshape(B * Ls, heads * dh).contiguous()
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()                 # (a column block of a fused QKV output keeps its row stride: the kernel takes any)
        dx, dw = ops.qk_rmsnorm_rope_bwd(x2, dy2, w, cos, sin, rows_per_batch=Ls, pos_offset=pos_offset, heads=heads, dh=dh, eps=eps)
        if w is None or not ctx.needs_input_grad[1]:
            dw = None
        return dx.view(B, Ls, heads * dh), dw, None, None, None, None, None


def qk_norm_rope(x, w, rope, heads: int, pos_offset: int = 0, eps: float = 1e-6):
    cos, sin = rope if rope is not None else (None, None)
    if w is None and cos is None:
        return x
    return QKNormRope.apply(x, w, cos, sin, heads, pos_offset, eps)


class FlashAttention(torch.autograd.Function):
    """F.scaled_dot_product_attention over heads packed as [B, L, H * dh] (any row stride). Forward: ug_flash_attn_fwd. Backward, per sample and
    for all heads at once (grouped GEMMs): S = Q K^T (fp32) -> lse -> P; dP = dO V^T; dS = scale P (dP - rowsum(dO O));
    dV = P^T dO, dK = dS^T Q, dQ = dS K. Lq and Lkv become contraction lengths: other lengths are zero-padded to multiples of 64 (padded keys get
    P = 0, padded queries carry dO = 0)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale=None):
        B, Lq, HD = q.shape
        Lkv = k.shape[1]
        dh = HD // heads
        o = torch.empty(B, Lq, HD, device=q.device, dtype=q.dtype)
        # bf16: the forward kernel also leaves the rows' log-sum-exp for the backward kernels (zero padding up to a multiple of 64 rows)
        lse = None
        if q.dtype == torch.bfloat16 and os.environ.get("UG_ATTN_BWD", "flash") != "gemm":
            lse = torch.zeros(B, heads, _pad64(Lq), device=q.device, dtype=torch.float32)
        ops.flash_attn(q, k, v, o, batches=B, heads=heads, dh=dh, Lq=Lq, Lkv=Lkv, q_strides=(q.stride(1), q.stride(0)), k_strides=(k.stride(1), k.stride(0)),
                       v_strides=(v.stride(1), v.stride(0)), o_strides=(HD, Lq * HD), lse=lse, **({} if scale is None else dict(scale=float(scale))))
        ctx.save_for_backward(q, k, v, o)
        ctx.heads, ctx.lse, ctx.scale = heads, lse, scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o = ctx.saved_tensors
        H = ctx.heads
        B, Lq, HD = q.shape
        Lkv = k.shape[1]
        dh = HD // H
        dt, dev = q.dtype, q.device
        scale = dh ** -0.5 if ctx.scale is None else float(ctx.scale)
        do = do.contiguous()
        if dt == torch.bfloat16 and os.environ.get("UG_ATTN_BWD", "flash") != "gemm":
            # product path: the tiled backward kernels (csrc/attention.hip); UG_ATTN_BWD=gemm keeps the GEMM formulation below (A/B, and what fp32 runs)
            dq, dk, dv = ops.flash_attn_bwd(q, k, v, o, do, heads=H, lse=ctx.lse, **({} if ctx.scale is None else dict(scale=scale)))
            return dq, dk, dv, None, None
        Lq0, Lkv0 = Lq, Lkv
        if Lq % 64 or Lkv % 64:
            Lq, Lkv = _pad64(Lq), _pad64(Lkv)
            padr = lambda t, n: torch.nn.functional.pad(t, (0, 0, 0, n - t.shape[1]))
            q, o, do = padr(q, Lq), padr(o, Lq), padr(do, Lq)
            k, v = padr(k, Lkv), padr(v, Lkv)
        dq, dk, dv = torch.empty(B, Lq, HD, device=dev, dtype=dt), torch.empty(B, Lkv, HD, device=dev, dtype=dt), torch.empty(B, Lkv, HD, device=dev, dtype=dt)
        S, dP = torch.empty(H, Lq, Lkv, device=dev, dtype=torch.float32), torch.empty(H, Lq, Lkv, device=dev, dtype=torch.float32)
        for b in range(B):
            qb, kb, vb, ob, dob = q[b], k[b], v[b], o[b], do[b]
            ops.gemm(qb[:, :dh], kb[:, :dh], None, S, M=Lq, epilogue=L.EPI_F32, groups=H, a_gstride=dh, w_gstride=dh, c_gstride=Lq * Lkv, ldc=Lkv)
            lse = ops.row_lse(S.view(H * Lq, Lkv), scale, Lkv0)
            P = ops.attn_prob(S.view(H * Lq, Lkv), lse, scale, dt, Lkv0)
            ops.gemm(dob[:, :dh], vb[:, :dh], None, dP, M=Lq, epilogue=L.EPI_F32, groups=H, a_gstride=dh, w_gstride=dh, c_gstride=Lq * Lkv, ldc=Lkv)
            delta = ops.rowdot(dob, ob, H)                                   # [H, Lq]
            dS = ops.attn_dscore(P, dP.view(H * Lq, Lkv), delta.view(-1), scale)
            P3, dS3 = P.view(H, Lq, Lkv), dS.view(H, Lq, Lkv)
            per_head = lambda t, Lr: torch.as_strided(t, (H, Lr, dh), (dh, t.stride(0), 1))
            PT, dST = ops.transpose(P3), ops.transpose(dS3)                   # [H, Lkv, Lq]
            dOT, QT, KT = ops.transpose(per_head(dob, Lq)), ops.transpose(per_head(qb, Lq)), ops.transpose(per_head(kb, Lkv))   # [H, dh, L]
            g = dict(groups=H, c_gstride=dh, ldc=HD)
            ops.gemm(PT, dOT, None, dv[b], M=Lkv, a_gstride=Lkv * Lq, w_gstride=dh * Lq, **g)
            ops.gemm(dST, QT, None, dk[b], M=Lkv, a_gstride=Lkv * Lq, w_gstride=dh * Lq, **g)
            ops.gemm(dS3, KT, None, dq[b], M=Lq, a_gstride=Lq * Lkv, w_gstride=dh * Lkv, **g)
        return dq[:, :Lq0], dk[:, :Lkv0], dv[:, :Lkv0], None, None


def attention(q, k, v, heads: int, scale: Optional[float] = None):
    """scale: the softmax scale (None: dh ** -0.5, the default path, unchanged) - the padded cross-attention heads of unigen_amd/sana.py run at the
    slot width with the true head width's scale."""
    return FlashAttention.apply(q, k, v, heads) if scale is None else FlashAttention.apply(q, k, v, heads, scale)


class LinearAttention(torch.autograd.Function):
    """SanaLinearAttnProcessor2_0 at head width 32 over heads packed as [B, N, H * 32]: ug_linear_attn forward, ug_linear_attn_bwd backward.
    q, k, v are typically the column blocks of one fused projection output and are saved as those views (any row stride); the forward's fp32 state
    (B H 1056 floats, the start of its workspace) is cloned for the backward, which recomputes the output from it - the rounded output is not
    saved. dq | dk | dv come back as the column blocks of one [B, N, 3 H 32] buffer: the dY of a fused projection."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        B, N, D = q.shape
        o = torch.empty(B, N, D, device=q.device, dtype=q.dtype)
        ws = torch.empty(ops.linear_attn_workspace_bytes(B, heads, N), device=q.device, dtype=torch.uint8)
        st = lambda t: (t.stride(1), t.stride(0))
        ops.linear_attn(q, k, v, o, batches=B, heads=heads, N=N, q_strides=st(q), k_strides=st(k), v_strides=st(v), o_strides=(D, N * D), workspace=ws)
        state = ws[:B * heads * 1056 * 4].view(torch.float32).clone()
        ctx.save_for_backward(q, k, v, state)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, state = ctx.saved_tensors
        B, N, D = q.shape
        do = do.contiguous()
        dqkv = torch.empty(B, N, 3 * D, device=q.device, dtype=q.dtype)
        st = lambda t: (t.stride(1), t.stride(0))
        s3 = (3 * D, N * 3 * D)
        ops.linear_attn_bwd(q, k, v, do, state, dqkv, dqkv[0, 0, D:], dqkv[0, 0, 2 * D:], batches=B, heads=ctx.heads, N=N, q_strides=st(q), k_strides=st(k),
                            v_strides=st(v), do_strides=st(do), dq_strides=s3, dk_strides=s3, dv_strides=s3)
        return dqkv[:, :, :D], dqkv[:, :, D:2 * D], dqkv[:, :, 2 * D:], None


def linear_attention(q, k, v, heads: int):
    return LinearAttention.apply(q, k, v, heads)


class GluDwConv(torch.autograd.Function):
    """The middle of GLUMBConv: x [B H W, 2C] (conv_inverted's output before its SiLU), conv_depth's weight [2C, 1, 3, 3] and bias [2C] ->
    [B H W, Cp] with the columns past C zero (the K padding of the conv_point GEMM). ug_glu_dwconv3x3 forward; backward ug_glu_dwconv3x3_bwd from the
    saved x: dx, and - only when the convolution's parameters take gradients - fp32 dw9 / dbias, rounded once into the parameter's dtype and layout."""

    @staticmethod
    def forward(ctx, x, w, b, B, H, W, C, Cp):
        w9 = w.reshape(2 * C, 9).t().contiguous()
        b = b.contiguous()
        out = torch.empty(B * H * W, Cp, device=x.device, dtype=x.dtype)
        ops.glu_dwconv3x3(x, w9, b, out, B=B, H=H, W=W, C=C)
        ctx.save_for_backward(x, w9, b)
        ctx.geom = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w9, b = ctx.saved_tensors
        B, H, W, C = ctx.geom
        dout = dout.contiguous()
        dx = torch.empty(B * H * W, 2 * C, device=x.device, dtype=x.dtype)
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dw9 = torch.empty(9, 2 * C, device=x.device, dtype=torch.float32) if need_w else None
        dbias = torch.empty(2 * C, device=x.device, dtype=torch.float32) if need_w else None
        ops.glu_dwconv3x3_bwd(x, w9, b, dout, dx, B=B, H=H, W=W, C=C, dw9=dw9, dbias=dbias)
        dw = dw9.t().reshape(2 * C, 1, 3, 3).to(x.dtype) if ctx.needs_input_grad[1] else None
        db = dbias.to(x.dtype) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None, None, None
