"""Host side of adapter training, no GPU: `set_lora_trainable` names, the three key forms of `load_lora_state_dict` round-trip, the differentiable
fuse step equals the inference one and routes gradients to each adapter's own weights, and the C ABI still matches the header with the new symbols."""
import os
import re
import subprocess

import pytest
import torch

from unigen_amd import lib as L
from unigen_amd.flux import UniGenFlux
from unigen_amd.lora import adapter_operands, enable_lora, fuse_adapters, fuse_adapters_autograd

TINY = dict(num_layers=2, num_single_layers=4, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
ATTN = ["attn.to_q", "attn.to_k", "attn.to_v"]


def _model():
    m = UniGenFlux.from_config(dict(TINY), device="cpu", dtype=torch.bfloat16)
    m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True, single_control_dev=2))
    m.add_lora(ATTN, "canny", 8, 16.0, prefix="control_joint_trans_blocks.", init_lora_weights=False, seed=1)
    m.add_lora(ATTN[:2], "depth", 4, 4.0, prefix="control_joint_trans_blocks.", init_lora_weights=False, seed=2)
    return m


def test_set_lora_trainable_names_and_freezing():
    m = _model()
    m.init_trainable_param()
    names = m.set_lora_trainable(["depth"])
    assert names and all(".lora_A.depth." in n or ".lora_B.depth." in n for n in names)
    assert len(names) == 2 * sum("depth" in s.lora_A for s in m._lora_sites.values())
    assert [n for n, p in m.named_parameters() if p.requires_grad] == names
    both = m.set_lora_trainable()
    assert len(both) > len(names) and all(".lora_" in n for n in both)
    m.init_trainable_param()
    kept = m.set_lora_trainable(["canny"], freeze_rest=False)
    assert any(".lora_" not in n for n in kept)
    with pytest.raises(ValueError, match="unknown adapters"):
        m.set_lora_trainable(["nope"])


@pytest.mark.parametrize("form", ["peft", "transformer", "in_model"])
def test_lora_state_dict_round_trips_in_every_key_form(form):
    src, dst = _model(), _model()
    with torch.no_grad():
        for s in src._lora_sites.values():
            s.lora_A["canny"].weight.mul_(3.0); s.lora_B["canny"].weight.add_(1.0)
    sd = src.lora_state_dict("canny")
    assert all(re.fullmatch(r".+\.lora_[AB]\.weight", k) and "canny" not in k for k in sd) and len(sd) == 2 * len(src._lora_sites)
    if form == "transformer":
        sd = {"transformer." + k: v for k, v in sd.items()}
    elif form == "in_model":
        sd = {k.replace(".weight", ".canny.weight"): v for k, v in sd.items()}
    used = dst.load_lora_state_dict(sd, "canny")
    assert len(used) == len(sd)
    for n, s in src._lora_sites.items():
        d = dst._lora_sites[n]
        assert torch.equal(s.lora_A["canny"].weight, d.lora_A["canny"].weight) and torch.equal(s.lora_B["canny"].weight, d.lora_B["canny"].weight)
        if "depth" in s.lora_A:                                     # the other adapter is untouched
            assert not torch.equal(s.lora_A["canny"].weight[:4], d.lora_A["depth"].weight)
    with pytest.raises(KeyError):
        dst.load_lora_state_dict({"nowhere.lora_A.weight": torch.zeros(1)}, "canny")
    with pytest.raises(KeyError, match="missing"):
        dst.load_lora_state_dict(dict(list(src.lora_state_dict("canny").items())[:2]), "canny")


def test_differentiable_fuse_equals_inference_fuse_and_routes_gradients():
    m = _model()
    p = "control_joint_trans_blocks.0.attn."
    sites = [m._lora_sites.get(p + n) for n in ("to_q", "to_k", "to_v")] + [None]
    widths = [256, 256, 256, 64]
    sites[0].set_scale("depth", 1.5)                                # alpha != r on both adapters of to_q
    A0, B0 = fuse_adapters(sites, widths, torch.bfloat16, "cpu")
    # the builder in its merge form (HipModule._merge_into): ONE projection, explicit (A, B, scale) blocks - ranks 4 and 8, alpha / r = 2 and 1.5
    q = sites[0]
    assert {a: (q.r[a], q.scaling[a]) for a in q.live_adapters()} == {"canny": (8, 2.0), "depth": (4, 1.5)}
    blocks = [(q.lora_A[a].weight, q.lora_B[a].weight, q.scaling[a]) for a in q.live_adapters()]
    Aq, Bq = fuse_adapters([q], [256], torch.bfloat16, "cpu")
    Am, Bm = adapter_operands([blocks], [256], torch.bfloat16, "cpu")
    assert torch.equal(Am, Aq) and torch.equal(Bm, Bq) and Am.shape == (64, 256) and Bm.shape == (256, 64) and Am.is_contiguous() and Bm.is_contiguous()
    assert torch.equal(Am[:12], A0[:12]) and torch.equal(Bm[:, :12], B0[:256, :12]) and not Am[12:].any() and not Bm[:, 12:].any()   # = to_q's block of the three-way launch
    m.set_lora_trainable()
    A1, B1, has = fuse_adapters_autograd(sites, widths, torch.bfloat16, "cpu")
    assert torch.equal(A0, A1) and torch.equal(B0, B1) and has == (True, True, True, False)
    assert A1.shape == (64, 256) and B1.shape == (sum(widths), 64)
    gA, gB = torch.ones_like(A1, dtype=torch.float32), torch.ones_like(B1, dtype=torch.float32)
    torch.autograd.backward([A1.float(), B1.float()], [gA, gB])
    q = sites[0]
    assert torch.equal(q.lora_A["canny"].weight.grad.float(), torch.ones(8, 256))
    assert torch.equal(q.lora_B["canny"].weight.grad.float(), torch.full((256, 8), q.scaling["canny"]))       # the scaling reaches dB
    assert torch.equal(q.lora_B["depth"].weight.grad.float(), torch.full((256, 4), q.scaling["depth"]))
    # a scaling of 0: not live, no operand, no gradient
    for s in sites[:3]:
        s.set_scale("canny", 0)
        s.set_scale("depth", 0)
    assert fuse_adapters_autograd(sites, widths, torch.bfloat16, "cpu") is None
    for s in sites[:3]:
        s.unscale_layer(None)                                       # back to alpha / r: live again
    assert fuse_adapters(sites, widths, torch.bfloat16, "cpu")[0] is not None
    # every adapter switched off by enable_lora: no operands in any of the three forms
    with enable_lora(list(m.modules()), []):
        assert fuse_adapters(sites, widths, torch.bfloat16, "cpu") == (None, None)
        assert fuse_adapters_autograd(sites, widths, torch.bfloat16, "cpu") is None
        assert adapter_operands([[(q.lora_A[a].weight, q.lora_B[a].weight, q.scaling[a]) for a in q.live_adapters()]], [256], torch.bfloat16, "cpu") == (None, None)


def test_header_and_exports_agree_with_the_new_symbols():
    from unigen_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "unigen_hip.h")).read()
    declared = set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", hdr))
    assert {"ug_lora_wgrad_bf16", "ug_lora_wgrad_f32", "ug_lora_wgrad_workspace_bytes"} <= declared
    assert declared == set(L.SIGNATURES)
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("ug_")}
    assert declared <= exported, declared - exported
    assert "lora_bwd.hip" in build.SOURCES
