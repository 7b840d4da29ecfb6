"""Low-precision AdamW (unigen_amd/optim.py, csrc/optim.hip) without a GPU: argument validation of the new entry points before any launch, the
ctypes mirrors of the new structs against a compile of the header, and what AdamW refuses of the new options."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a fake, aligned device address: every call below fails validation before it could be used


def _table(n=1, **kw):
    from unigen_amd import lib
    t = (lib.OptimTensorLP * n)()
    for i, d in enumerate(t):
        d.param, d.grad, d.master, d.exp_avg, d.exp_avg_sq, d.numel = P, P, None, P, P, 100
        d.param_dtype, d.grad_dtype, d.state_dtype, d.group, d.param_index = lib.UG_DT_BF16, lib.UG_DT_BF16, lib.UG_DT_BF16, 0, i
    for k, v in kw.items():
        setattr(t[0], k, v)
    return t


def test_lowp_entry_points_validate_before_launching():
    from unigen_amd import lib
    cdll = lib.load()
    err = lambda: cdll.ug_last_error()
    check = lambda t, n_groups=1: cdll.ug_optim_check_table_lowp(ctypes.addressof(t), len(t), n_groups)
    BF, F32 = lib.UG_DT_BF16, lib.UG_DT_F32
    # the arrangements of a bf16 param: (no master, bf16 state), (no master, fp32 state), (master, bf16 state), (master, fp32 state: the default's)
    assert check(_table(2)) == lib.UG_OK and check(_table(state_dtype=F32)) == lib.UG_OK
    assert check(_table(master=P)) == lib.UG_OK and check(_table(master=P, state_dtype=F32)) == lib.UG_OK
    assert check(_table(param_dtype=F32, state_dtype=F32)) == lib.UG_OK                           # an fp32 param: in place, fp32 moments
    assert check(_table(param_dtype=F32)) == lib.UG_ERR_UNSUPPORTED and b"fp32 param" in err()    # ... never bf16 moments
    assert check(_table(param_dtype=F32, state_dtype=F32, master=P)) == lib.UG_ERR_UNSUPPORTED    # ... nor a master
    assert cdll.ug_optim_check_table_lowp(None, 1, 1) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert check(_table(), 0) == lib.UG_ERR_UNSUPPORTED and check(_table(), lib.UG_ADAMW_MAX_GROUPS + 1) == lib.UG_ERR_UNSUPPORTED
    assert check(_table(numel=-1)) == lib.UG_ERR_BAD_SHAPE and b"numel < 0" in err()
    assert check(_table(grad_dtype=7)) == lib.UG_ERR_UNSUPPORTED and b"unknown grad dtype" in err()
    assert check(_table(param_dtype=2)) == lib.UG_ERR_UNSUPPORTED and b"unknown param dtype" in err()
    assert check(_table(state_dtype=2)) == lib.UG_ERR_UNSUPPORTED and b"unknown state dtype" in err()
    assert check(_table(group=1)) == lib.UG_ERR_BAD_SHAPE and b"group" in err()
    assert check(_table(grad=None)) == lib.UG_ERR_BAD_SHAPE and b"null grad" in err()
    assert check(_table(param=None)) == lib.UG_ERR_BAD_SHAPE and check(_table(exp_avg_sq=None)) == lib.UG_ERR_BAD_SHAPE
    assert check(_table(grad=None, param=None, numel=0)) == lib.UG_OK                              # an empty tensor has no chunk
    assert check(_table(grad=P + 1)) == lib.UG_ERR_BAD_ALIGN and check(_table(exp_avg=P + 1)) == lib.UG_ERR_BAD_ALIGN
    assert check(_table(exp_avg=P + 2)) == lib.UG_OK and check(_table(exp_avg=P + 2, state_dtype=F32)) == lib.UG_ERR_BAD_ALIGN
    assert check(_table(master=P + 2)) == lib.UG_ERR_BAD_ALIGN

    g = (lib.AdamwGroupLP * (lib.UG_ADAMW_MAX_GROUPS + 1))()
    for h in g:
        h.step = 1
    step = lambda *a: cdll.ug_adamw_step_lowp(*a)
    assert step(None, 1, P, 4, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert step(P, 1, P, -5, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE
    assert step(P, 0, P, 4, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE
    assert step(P, 1, None, 4, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE and b"chunk list" in err()
    assert step(P, 1, P, 4, None, 1, None, None) == lib.UG_ERR_BAD_SHAPE and b"group" in err()
    assert step(P, 1, P, 4, ctypes.addressof(g), lib.UG_ADAMW_MAX_GROUPS + 1, None, None) == lib.UG_ERR_UNSUPPORTED
    g[1].step = 0
    assert step(P, 1, P, 4, ctypes.addressof(g), 2, None, None) == lib.UG_ERR_BAD_SHAPE and b"step 0" in err()
    assert step(P, 1, P, 0, ctypes.addressof(g), 1, None, None) == lib.UG_OK                       # no chunk: nothing to launch

    sr = lambda **kw: cdll.ug_sr_round_bf16(*[{**dict(x=P, out=P, n=8, first=0, seed=1, pi=0, step=1, word=0, stream=None), **kw}[k]
                                              for k in ("x", "out", "n", "first", "seed", "pi", "step", "word", "stream")])
    assert sr(n=0) == lib.UG_OK and sr(n=0, x=None, out=None) == lib.UG_OK
    assert sr(x=None) == lib.UG_ERR_BAD_SHAPE and sr(out=None) == lib.UG_ERR_BAD_SHAPE and b"null" in err()
    assert sr(n=-1) == lib.UG_ERR_BAD_SHAPE and sr(first=-1) == lib.UG_ERR_BAD_SHAPE
    assert sr(word=3) == lib.UG_ERR_UNSUPPORTED and sr(word=-1) == lib.UG_ERR_UNSUPPORTED and b"word" in err()
    assert sr(x=P + 2) == lib.UG_ERR_BAD_ALIGN and sr(out=P + 1) == lib.UG_ERR_BAD_ALIGN
    assert sr(first=(1 << 63) - 4) == lib.UG_ERR_UNSUPPORTED


def test_lowp_descriptor_layouts_match_the_header(tmp_path):
    from unigen_amd import lib
    src = ('#include "unigen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu",'
           ' sizeof(ug_optim_tensor_lp), offsetof(ug_optim_tensor_lp, master), offsetof(ug_optim_tensor_lp, exp_avg_sq), offsetof(ug_optim_tensor_lp, numel),'
           ' offsetof(ug_optim_tensor_lp, grad_dtype), offsetof(ug_optim_tensor_lp, state_dtype), offsetof(ug_optim_tensor_lp, group),'
           ' offsetof(ug_optim_tensor_lp, param_index), sizeof(ug_adamw_group_lp), offsetof(ug_adamw_group_lp, inv_bc2_sqrt),'
           ' offsetof(ug_adamw_group_lp, step), offsetof(ug_adamw_group_lp, seed));return 0;}')
    exe = str(tmp_path / "ug_optim_lowp_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, check=True).stdout.split()))
    T, G = lib.OptimTensorLP, lib.AdamwGroupLP
    assert got == [ctypes.sizeof(T), T.master.offset, T.exp_avg_sq.offset, T.numel.offset, T.grad_dtype.offset, T.state_dtype.offset, T.group.offset,
                   T.param_index.offset, ctypes.sizeof(G), G.inv_bc2_sqrt.offset, G.step.offset, G.seed.offset]
    # the hyperparameters come first and in ug_adamw_group's order: one host routine fills both
    assert [f[0] for f in G._fields_[:7]] == [f[0] for f in lib.AdamwGroup._fields_[:7]]


def test_adamw_refuses_bad_lowp_options():
    from unigen_amd.optim import AdamW
    w = torch.nn.Parameter(torch.zeros(4))
    for bad in (torch.float16, torch.float64, torch.int32, "bf16"):
        with pytest.raises(ValueError, match="state_dtype"):
            AdamW([w], state_dtype=bad)
    with pytest.raises(ValueError, match="state_dtype"):               # per group too
        AdamW([{"params": [w], "state_dtype": torch.float16}])
    for bad in (-1, 1 << 64, 1.5, None):
        with pytest.raises(ValueError, match="seed"):
            AdamW([w], seed=bad)
    with pytest.raises(ValueError, match="amsgrad"):                   # still refused beside the new options
        AdamW([w], amsgrad=True, master_weights=False)
    with pytest.raises(ValueError, match="maximize"):
        AdamW([w], maximize=True, state_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):                       # valid options: the refusal left is the CPU parameter's
        AdamW([w], master_weights=False, state_dtype=torch.bfloat16, seed=(1 << 64) - 1)
