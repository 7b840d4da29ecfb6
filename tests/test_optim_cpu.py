"""Optimizer step (unigen_amd/optim.py, csrc/optim.hip) without a GPU: argument validation of every new entry point before any launch, the
ctypes mirrors of the descriptor structs against a compile of the header, the chunk-list builder, and what AdamW refuses."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a fake, aligned device address: every call below fails validation before it could be used


def _table(n=1, **kw):
    from unigen_amd import lib
    t = (lib.OptimTensor * n)()
    for d in t:
        d.param, d.grad, d.master, d.exp_avg, d.exp_avg_sq, d.numel = P, P, P, P, P, 100
        d.param_dtype, d.grad_dtype, d.group = lib.UG_DT_BF16, lib.UG_DT_BF16, 0
    for k, v in kw.items():
        setattr(t[0], k, v)
    return t


def test_optim_entry_points_validate_before_launching():
    from unigen_amd import lib
    cdll = lib.load()
    err = lambda: cdll.ug_last_error()
    check = lambda t, n_groups=1: cdll.ug_optim_check_table(ctypes.addressof(t), len(t), n_groups)
    assert check(_table(2)) == lib.UG_OK and check(_table(2), 0) == lib.UG_OK
    assert cdll.ug_optim_check_table(None, 1, 1) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert check(_table(numel=-1)) == lib.UG_ERR_BAD_SHAPE and b"numel < 0" in err()
    assert check(_table(grad_dtype=7)) == lib.UG_ERR_UNSUPPORTED and b"unknown grad dtype" in err()
    assert check(_table(param_dtype=2)) == lib.UG_ERR_UNSUPPORTED and b"unknown param dtype" in err()
    assert check(_table(param_dtype=2), 0) == lib.UG_OK                                       # a gradient-only table has no param
    assert check(_table(group=1)) == lib.UG_ERR_BAD_SHAPE and b"group" in err()
    assert check(_table(master=None)) == lib.UG_ERR_UNSUPPORTED and b"master" in err()         # bf16 param without a master
    assert check(_table(param_dtype=lib.UG_DT_F32)) == lib.UG_ERR_UNSUPPORTED                  # fp32 param with one
    assert check(_table(grad=None)) == lib.UG_ERR_BAD_SHAPE and b"null grad" in err()
    assert check(_table(exp_avg_sq=None)) == lib.UG_ERR_BAD_SHAPE
    assert check(_table(grad=P + 1)) == lib.UG_ERR_BAD_ALIGN
    assert check(_table(), lib.UG_ADAMW_MAX_GROUPS + 1) == lib.UG_ERR_UNSUPPORTED

    assert cdll.ug_grad_sumsq_workspace_bytes(10) == 80 and cdll.ug_grad_sumsq_workspace_bytes(0) == 8
    assert cdll.ug_grad_sumsq(None, 1, P, 4, 1.0, P, P, 1 << 20, None) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert cdll.ug_grad_sumsq(P, 1, P, -1, 1.0, P, P, 1 << 20, None) == lib.UG_ERR_BAD_SHAPE
    assert cdll.ug_grad_sumsq(P, 1, None, 4, 1.0, P, P, 1 << 20, None) == lib.UG_ERR_BAD_SHAPE and b"chunk list" in err()
    assert cdll.ug_grad_sumsq(P, 1, P, 4, 1.0, None, P, 1 << 20, None) == lib.UG_ERR_BAD_SHAPE
    assert cdll.ug_grad_sumsq(P, 1, P, 4, 1.0, P, P, 31, None) == lib.UG_ERR_BAD_SHAPE and b"workspace" in err()
    assert cdll.ug_grad_scale(None, 1, P, 4, P, None) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert cdll.ug_grad_scale(P, 1, P, 4, None, None) == lib.UG_ERR_BAD_SHAPE and b"coef" in err()
    assert cdll.ug_grad_scale(P, 0, P, 4, P, None) == lib.UG_ERR_BAD_SHAPE
    g = (lib.AdamwGroup * (lib.UG_ADAMW_MAX_GROUPS + 1))()
    assert cdll.ug_adamw_step(None, 1, P, 4, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE and b"null table" in err()
    assert cdll.ug_adamw_step(P, 1, P, -5, ctypes.addressof(g), 1, None, None) == lib.UG_ERR_BAD_SHAPE
    assert cdll.ug_adamw_step(P, 1, P, 4, None, 1, None, None) == lib.UG_ERR_BAD_SHAPE and b"group" in err()
    assert cdll.ug_adamw_step(P, 1, P, 4, ctypes.addressof(g), lib.UG_ADAMW_MAX_GROUPS + 1, None, None) == lib.UG_ERR_UNSUPPORTED


def test_optim_descriptor_layouts_match_the_header(tmp_path):
    from unigen_amd import lib
    src = ('#include "unigen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d",'
           ' sizeof(ug_optim_tensor), offsetof(ug_optim_tensor, exp_avg_sq), offsetof(ug_optim_tensor, numel), offsetof(ug_optim_tensor, grad_dtype),'
           ' offsetof(ug_optim_tensor, group), sizeof(ug_adamw_group), offsetof(ug_adamw_group, inv_bc2_sqrt), UG_OPTIM_CHUNK, UG_ADAMW_MAX_GROUPS);return 0;}')
    exe = str(tmp_path / "ug_optim_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, check=True).stdout.split()))
    T, G = lib.OptimTensor, lib.AdamwGroup
    assert got == [ctypes.sizeof(T), T.exp_avg_sq.offset, T.numel.offset, T.grad_dtype.offset, T.group.offset, ctypes.sizeof(G), G.inv_bc2_sqrt.offset,
                   lib.UG_OPTIM_CHUNK, lib.UG_ADAMW_MAX_GROUPS]


@pytest.mark.parametrize("numels,chunk", [([1, 7, 4095, (1 << 20) + 3], 65536), ([0, 5, 0, 64, 65, 1], 64), ([1], 65536), ([], 65536),
                                          ([0, 0], 16), ([3 * 65536, 65536 + 1, 65535], 65536)])
def test_chunk_list_covers_every_element_once(numels, chunk):
    from unigen_amd.optim import chunk_list
    cl = chunk_list(numels, chunk)
    assert cl.dtype == torch.int32 and cl.dim() == 2 and cl.shape[1] == 2
    seen = [torch.zeros(n, dtype=torch.int64) for n in numels]
    for t, c in cl.tolist():
        lo, hi = c * chunk, min((c + 1) * chunk, numels[t])
        assert lo < hi, (t, c)                          # no empty chunk
        seen[t][lo:hi] += 1
    assert all(bool((s == 1).all()) for s in seen)
    assert cl.shape[0] == sum((n + chunk - 1) // chunk for n in numels)


def test_adamw_refuses_what_it_does_not_implement():
    from unigen_amd.optim import AdamW, clip_grad_norm_
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW([w], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        AdamW([w], maximize=True)
    with pytest.raises(ValueError, match="sparse"):
        AdamW([torch.nn.Parameter(torch.sparse_coo_tensor(torch.zeros(1, 1, dtype=torch.long), torch.ones(1), (4,)))])
    with pytest.raises(ValueError, match="bf16 or fp32"):
        AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError, match="complex"):
        AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.complex64))])
    with pytest.raises(ValueError, match="contiguous"):
        AdamW([torch.nn.Parameter(torch.zeros(4, 4).t())])
    with pytest.raises(ValueError, match="GPU"):
        AdamW([w])                                      # a CPU parameter
    with pytest.raises(ValueError, match="bf16 or fp32"):        # params given as groups are checked too
        AdamW([{"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.float16))], "lr": 1e-4}])
    w.grad = torch.ones(4)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([w], 1.0, norm_type=float("inf"))
