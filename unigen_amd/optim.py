"""On-device optimizer step of the control-module training loop (reference train.py:652-662):

    clip_grad_norm_(params, 1.0)                                  accelerator.clip_grad_norm_(transformer.parameters(), max_grad_norm)  (:658)
    AdamW(params, lr, betas, eps, weight_decay, max_grad_norm=)   torch.optim.AdamW(...) (:351-359) + its .step() (:660), clipping fused in

Both run the multi-tensor HIP kernels of csrc/optim.hip: one launch covers every trainable tensor (a device table of descriptors and a list
of (tensor, chunk) pairs built once per set of addresses). bf16 parameters get fp32 master weights and fp32 moments - the reference's
DeepSpeed setup (bf16 on, fp32 masters and optimizer state) - so an update far below a bf16 ulp of the weight is not rounded away; the bf16
parameter is the round-to-nearest-even of its master after every step. fp32 parameters are updated in place with fp32 moments. No host
synchronisation in either call (clip_grad_norm_(error_if_nonfinite=True) excepted, as in torch).

AdamW(master_weights=False, state_dtype=torch.bfloat16, seed=) is the opt-in alternative where 12 B of state per element do not fit: no masters,
bf16 moments, what is kept in bf16 written with stochastic rounding (ug_adamw_step_lowp; draws of a counter-based generator, so nothing but the
seed has to be saved to resume a run bit for bit). The default is untouched by it: same state, same launches, same bits.

The kernels write through raw pointers: every written tensor's version counter is bumped after the launch, so the caches of this package
keyed on `_version` (autograd._wt_cache, the LoRA fusion, the position-id tables) see the update. Parameters that are views into the engine's
packed weight buffers are updated in place there, so the inference path reads the new values too.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence, Union

import torch

from . import lib as L

CHUNK = L.UG_OPTIM_CHUNK
_DT = {torch.bfloat16: L.UG_DT_BF16, torch.float32: L.UG_DT_F32}


def chunk_list(numels: Sequence[int], chunk: int = CHUNK) -> torch.Tensor:
    """int32 [n_chunks, 2] (tensor index, chunk index): chunk c of tensor t covers elements [c * chunk, min((c + 1) * chunk, numel)); every
    element of every tensor lies in exactly one chunk, empty tensors have none."""
    counts = torch.tensor([(int(n) + chunk - 1) // chunk for n in numels], dtype=torch.int64)
    if counts.numel() == 0 or int(counts.sum()) == 0:
        return torch.zeros(0, 2, dtype=torch.int32)
    tensor = torch.repeat_interleave(torch.arange(len(counts)), counts)
    first = torch.cumsum(counts, 0) - counts
    index = torch.arange(int(counts.sum())) - torch.repeat_interleave(first, counts)
    return torch.stack([tensor, index], 1).to(torch.int32)


def _upload(host: torch.Tensor, device: torch.device) -> torch.Tensor:
    # a fresh pinned buffer and a stream-ordered copy: the host caching allocator keeps the buffer until the copy has run, no synchronisation
    return host.pin_memory().to(device, non_blocking=True)


class _WorkList:
    """Device descriptor table + chunk list for one set of tensors. `rows`: (param, grad, master, exp_avg, exp_avg_sq, group) per tensor."""

    def __init__(self, rows, device: torch.device, n_groups: int):
        n = len(rows)
        table = (L.OptimTensor * n)()
        for i, (p, g, master, m, v, group) in enumerate(rows):
            d = table[i]
            d.grad, d.grad_dtype, d.numel = g.data_ptr(), _DT[g.dtype], g.numel()
            if p is not None:
                d.param, d.param_dtype = p.data_ptr(), _DT[p.dtype]
                d.master = master.data_ptr() if master is not None else None
                d.exp_avg, d.exp_avg_sq, d.group = m.data_ptr(), v.data_ptr(), group
        L.call("ug_optim_check_table", C.addressof(table), n, n_groups)
        self.n_tensors = n
        self.table = _upload(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8), device)
        chunks = chunk_list([r[1].numel() for r in rows])
        self.n_chunks = chunks.shape[0]
        self.chunks = _upload(chunks, device)

    def sumsq(self, max_norm: float, device: torch.device, stream: int) -> torch.Tensor:
        """-> fp32 [2] device tensor (total_norm, clip_coef)."""
        out = torch.empty(2, dtype=torch.float32, device=device)
        cdll = L.load()
        nbytes = cdll.ug_grad_sumsq_workspace_bytes(self.n_chunks)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        L.call("ug_grad_sumsq", self.table.data_ptr(), self.n_tensors, self.chunks.data_ptr(), self.n_chunks, float(max_norm), out.data_ptr(), ws.data_ptr(),
               nbytes, stream)
        return out


class _WorkListLP(_WorkList):
    """The same for ug_adamw_step_lowp. `rows`: (param, grad, master, exp_avg, exp_avg_sq, group, param_index) per tensor."""

    def __init__(self, rows, device: torch.device, n_groups: int):
        n = len(rows)
        table = (L.OptimTensorLP * n)()
        for i, (p, g, master, m, v, group, index) in enumerate(rows):
            d = table[i]
            d.grad, d.grad_dtype, d.numel = g.data_ptr(), _DT[g.dtype], g.numel()
            d.param, d.param_dtype = p.data_ptr(), _DT[p.dtype]
            d.master = master.data_ptr() if master is not None else None
            d.exp_avg, d.exp_avg_sq, d.state_dtype, d.group, d.param_index = m.data_ptr(), v.data_ptr(), _DT[m.dtype], group, index
        L.call("ug_optim_check_table_lowp", C.addressof(table), n, n_groups)
        self.n_tensors = n
        self.table = _upload(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8), device)
        chunks = chunk_list([r[1].numel() for r in rows])
        self.n_chunks = chunks.shape[0]
        self.chunks = _upload(chunks, device)
        self._grads = [r[1] for r in rows]
        self._norm: Optional[_WorkList] = None

    def sumsq(self, max_norm: float, device: torch.device, stream: int) -> torch.Tensor:
        if self._norm is None:                # ug_grad_sumsq reads ug_optim_tensor descriptors: a gradient-only table of the same tensors
            self._norm = _WorkList([(None, g, None, None, None, 0) for g in self._grads], device, 0)
        return self._norm.sumsq(max_norm, device, stream)


_grad_lists: dict = {}        # clip_grad_norm_: gradient-only work lists by (address, numel, dtype) of every grad


def _check_tensor(t: torch.Tensor, what: str) -> None:
    if t.is_sparse or t.layout != torch.strided:
        raise ValueError(f"unigen_amd.optim: sparse {what} are not supported")
    if t.is_complex():
        raise ValueError(f"unigen_amd.optim: complex {what} are not supported")
    if t.dtype not in _DT:
        raise ValueError(f"unigen_amd.optim: {what} must be bf16 or fp32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"unigen_amd.optim: {what} must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"unigen_amd.optim: {what} must be on the GPU, got {t.device}")


def _one_device(tensors) -> torch.device:
    devs = {t.device for t in tensors}
    if len(devs) != 1:
        raise ValueError(f"unigen_amd.optim: every tensor must be on one GPU, got {sorted(map(str, devs))}")
    return devs.pop()


def clip_grad_norm_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float, norm_type: float = 2.0,
                    error_if_nonfinite: bool = False, foreach: Optional[bool] = None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (same signature, in-place semantics and clip coefficient min(1, max_norm / (total_norm + 1e-6))) for
    norm_type 2: two launches for the norm, one for the scaling, no host synchronisation. Returns the total norm as a 0-dim fp32 device tensor.

    Difference from torch: the squares are summed in fp32 per lane, fp64 across a chunk and across chunks, with no rounding of per-tensor
    norms; torch computes one norm per tensor in the grad's dtype (bf16 grads: per-tensor norms and the total rounded to bf16). `foreach` is
    accepted for signature compatibility; the multi-tensor kernel is always used."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError(f"unigen_amd.optim.clip_grad_norm_: only norm_type=2 is implemented, got {norm_type}")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    key = (tuple(map(torch.Tensor.data_ptr, grads)), tuple(map(torch.Tensor.numel, grads)), tuple(g.dtype for g in grads))
    wl = _grad_lists.get(key)
    if wl is None:
        for g in grads:
            _check_tensor(g, "gradients")
        if len(_grad_lists) >= 8:
            _grad_lists.clear()
        wl = _grad_lists[key] = _WorkList([(None, g, None, None, None, 0) for g in grads], _one_device(grads), 0)
    dev = grads[0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = wl.sumsq(max_norm, dev, stream)
    total = out[0]
    if error_if_nonfinite and torch.logical_or(total.isnan(), total.isinf()):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    L.call("ug_grad_scale", wl.table.data_ptr(), wl.n_tensors, wl.chunks.data_ptr(), wl.n_chunks, out[1:].data_ptr(), stream)
    torch.autograd.graph.increment_version(grads)
    return total


_LOWP_KEYS = ("master_weights", "state_dtype", "seed")


def _check_lowp_options(group: dict) -> None:
    sd, seed = group.get("state_dtype", torch.float32), group.get("seed", 0)
    if sd not in (torch.float32, torch.bfloat16):
        raise ValueError(f"unigen_amd.optim.AdamW: state_dtype must be torch.float32 or torch.bfloat16, got {sd}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"unigen_amd.optim.AdamW: seed must be an integer in [0, 2^64), got {seed!r}")


def _lowp_options(group: dict):
    return bool(group.get("master_weights", True)), group.get("state_dtype", torch.float32), int(group.get("seed", 0))


def _fill_group(h, group: dict, step: float) -> None:
    lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
    # torch.optim.adam._single_tensor_adam's host arithmetic (Python floats), rounded to fp32 once; its division of the tensor by
    # bias_correction2_sqrt (a Python scalar) is a product with the fp32 reciprocal of the scalar's fp32 value
    h.decay, h.lerp_w, h.beta2, h.one_minus_beta2 = 1 - lr * wd, 1 - b1, b2, 1 - b2
    h.eps, h.step_size, h.inv_bc2_sqrt = eps, lr / (1 - b1 ** step), 1.0 / C.c_float((1 - b2 ** step) ** 0.5).value


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, torch's single-tensor arithmetic in fp32) as one HIP launch over every parameter with a grad.

    Hyperparameters and param groups behave as torch's: `lr`, `betas`, `eps`, `weight_decay` are read from each group at every step (LR
    schedulers work unchanged), params whose grad is None are skipped and get no state. bf16 params get `state["master_param"]` (fp32) and
    fp32 moments; fp32 params are updated in place. `max_grad_norm` fuses clip_grad_norm_ into step(): the grads are read once by the norm and
    once by the update and never rewritten; the norm of the last step is `last_grad_norm` (0-dim fp32 device tensor).

    Low-precision state (off by default; the project's own mode, not the reference's). `master_weights=False` keeps no fp32 master: the bf16
    param is read, updated in fp32 and written back with stochastic rounding, so an update below a bf16 ulp still moves it in expectation.
    `state_dtype=torch.bfloat16` keeps the moments in bf16, written with stochastic rounding too. (False, bf16) holds 4 B of state per element
    instead of 12; (False, fp32) and (True, bf16) are the two halves of it. The options touch bf16 params only, live in every param group
    (groups may differ) and, unlike the hyperparameters, are not replaced by load_state_dict: a loaded state is converted to what this
    optimizer's groups ask for. The draws are Philox4x32-10 of (`seed`, the param's ordinal in param_groups, its step count, the element): a
    run resumed from a state dict continues with the bits of the uninterrupted run (include/unigen_hip.h has the layout).
    Not implemented (ValueError): amsgrad, maximize, sparse / complex / fp16 / non-contiguous / non-GPU params."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *, amsgrad: bool = False,
                 maximize: bool = False, max_grad_norm: Optional[float] = None, master_weights: bool = True,
                 state_dtype: torch.dtype = torch.float32, seed: int = 0):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError("unigen_amd.optim.AdamW: amsgrad is not implemented")
        if maximize:
            raise ValueError("unigen_amd.optim.AdamW: maximize is not implemented")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        _check_lowp_options(dict(master_weights=master_weights, state_dtype=state_dtype, seed=seed))
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      master_weights=bool(master_weights), state_dtype=state_dtype, seed=int(seed)))
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._wl: Optional[_WorkList] = None
        self._wl_key = self._written = None

    def add_param_group(self, param_group: dict) -> None:
        _check_lowp_options(param_group)
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            _check_tensor(p, "parameters")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps, gs, sts, gis, ids = [], [], [], [], []
        index, lowp = -1, False
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("unigen_amd.optim.AdamW: amsgrad / maximize are not implemented")
            _check_lowp_options(group)
            master, sdt, _ = _lowp_options(group)
            for p in group["params"]:
                index += 1                                # the param's ordinal: what state_dict() calls it, grads or not
                g = p.grad
                if g is None:
                    continue
                st = self.state[p]
                bf = p.dtype == torch.bfloat16
                if not st or (bf and (("master_param" in st) != master or st["exp_avg"].dtype != sdt)):
                    self._init_state(p, st, master, sdt)
                    self._wl_key = None
                lowp = lowp or (bf and (not master or sdt != torch.float32))
                ps.append(p); gs.append(g); sts.append(st); gis.append(gi); ids.append(index)
        if not ps:
            return loss
        steps = [st["step"] for st in sts]
        torch._foreach_add_(steps, 1.0)                   # the CPU fp32 step counters of torch's AdamW
        slots: dict = {}
        slot = [slots.setdefault(k, len(slots)) for k in zip(gis, torch.stack(steps).tolist())]   # one group normally shares one step count
        if len(slots) > L.UG_ADAMW_MAX_GROUPS:
            raise ValueError(f"unigen_amd.optim.AdamW: more than {L.UG_ADAMW_MAX_GROUPS} (param group, step count) combinations in one step")
        # the work list is rebuilt when a grad (zero_grad(set_to_none=True)), a param (engine packing) or the set of params moved; state
        # tensors only move with the set of params or in load_state_dict, which drops the list
        # (the low-precision launch is taken as soon as one tensor of the step is in a low-precision arrangement; it carries the others unchanged)
        key = (tuple(map(torch.Tensor.data_ptr, ps)), tuple(map(torch.Tensor.data_ptr, gs)), tuple(g.dtype for g in gs), tuple(slot), lowp)
        if key != self._wl_key:
            for p, g in zip(ps, gs):
                _check_tensor(g, "gradients")
                if g.shape != p.shape:
                    raise ValueError("unigen_amd.optim.AdamW: a gradient of another shape than its parameter")
            dev = _one_device(ps)
            rows = [(p, g, st.get("master_param"), st["exp_avg"], st["exp_avg_sq"], s) for p, g, st, s in zip(ps, gs, sts, slot)]
            wl = _WorkListLP([r + (i,) for r, i in zip(rows, ids)], dev, len(slots)) if lowp else _WorkList(rows, dev, len(slots))
            self._wl, self._wl_key, self._written = wl, key, ps + [t for r in rows for t in r[2:5] if t is not None]
        wl = self._wl
        dev = ps[0].device
        hp = ((L.AdamwGroupLP if lowp else L.AdamwGroup) * len(slots))()
        for (gi, step), s in slots.items():
            _fill_group(hp[s], self.param_groups[gi], step)
            if lowp:
                hp[s].step, hp[s].seed = int(step), _lowp_options(self.param_groups[gi])[2]
        stream = torch.cuda.current_stream(dev).cuda_stream
        coef = None
        if self.max_grad_norm is not None:
            out = wl.sumsq(self.max_grad_norm, dev, stream)
            self.last_grad_norm, coef = out[0], out[1:]
        L.call("ug_adamw_step_lowp" if lowp else "ug_adamw_step", wl.table.data_ptr(), wl.n_tensors, wl.chunks.data_ptr(), wl.n_chunks, C.addressof(hp),
               len(slots), None if coef is None else coef.data_ptr(), stream)
        torch.autograd.graph.increment_version(self._written)
        return loss

    @staticmethod
    def _init_state(p: torch.Tensor, st: dict, master_weights: bool = True, state_dtype: torch.dtype = torch.float32) -> None:
        """Creates the state of `p`, or brings an existing one to the arrangement asked for: moments are cast (to bf16: round-to-nearest, once),
        a master that is not wanted is dropped, one that is missing is seeded from the param."""
        bf = p.dtype == torch.bfloat16
        sdt = state_dtype if bf else torch.float32        # the options apply to bf16 params only
        if not st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros(p.shape, dtype=sdt, device=p.device)
            st["exp_avg_sq"] = torch.zeros(p.shape, dtype=sdt, device=p.device)
        for k in ("exp_avg", "exp_avg_sq"):
            if st[k].dtype != sdt:
                st[k] = st[k].to(sdt)
        if bf and master_weights and "master_param" not in st:
            st["master_param"] = p.detach().float()
        elif bf and not master_weights:
            st.pop("master_param", None)

    def load_state_dict(self, state_dict: dict) -> None:
        """torch's loader, except that the state stays fp32 (torch casts floating state to the PARAM's dtype, which would make the moments and
        masters of bf16 params bf16). A torch.optim.AdamW state dict loads too: its moments become fp32, masters are seeded from the params.

        `master_weights`, `state_dtype` and `seed` stay those of THIS optimizer's groups, whatever the saved groups say, and the state is made to
        fit them: fp32-master state loaded into a master-less group loses the masters (the params are the caller's) and its moments are rounded to
        bf16 (nearest, once) where the group keeps them so; low-precision state loaded into a default group gets fp32 moments (exact) and masters
        seeded from the params."""
        ids, own = {}, {}
        for saved, group in zip(state_dict["param_groups"], self.param_groups):
            ids.update(zip(saved["params"], group["params"]))
        keep = [{k: group[k] for k in _LOWP_KEYS if k in group} for group in self.param_groups]
        saved_state = state_dict["state"]
        super().load_state_dict(state_dict)
        for group, k in zip(self.param_groups, keep):
            group.update(k)
            own.update((p, group) for p in group["params"])
        for pid, st in saved_state.items():
            p = ids.get(pid)
            if p is None:
                continue
            new = self.state[p]
            master, sdt, _ = _lowp_options(own[p])
            for k, v in st.items():
                if not torch.is_tensor(v):
                    continue
                if k == "step":
                    new[k] = v.detach().to("cpu", torch.float32).clone()
                elif v.is_floating_point():
                    dt = sdt if k in ("exp_avg", "exp_avg_sq") and p.dtype == torch.bfloat16 else torch.float32
                    new[k] = v.detach().to(device=p.device, dtype=dt).clone(memory_format=torch.contiguous_format)
            if "exp_avg" in new and "exp_avg_sq" in new:
                self._init_state(p, new, master, sdt)
            elif p.dtype == torch.bfloat16 and master and "master_param" not in new:
                new["master_param"] = p.detach().float()
        self._wl = self._wl_key = self._written = None
