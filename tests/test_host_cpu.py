"""CPU tests of the host side: the C-ABI library loads and exports every symbol include/unigen_hip.h declares (no compute calls
without a GPU), the drop-in classes keep the reference's names / state-dict keys / error behaviour, the product path refuses to
run without the HIP device, and the multi-process harness works over gloo with world_size 2."""
import ctypes
import importlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(num_layers=2, num_single_layers=4, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
CONTROL = dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True, single_control_dev=2)


def test_library_exports_every_declared_symbol(tmp_path):
    from unigen_amd import build, lib
    build.build()
    hdr = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)                 # a `ug_x(` inside a comment declares nothing
    declared = set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 154 and declared == set(lib.SIGNATURES), declared ^ set(lib.SIGNATURES)
    cdll = lib.load()
    for name in declared:
        assert getattr(cdll, name) is not None
    assert cdll.ug_version() >= 100
    # every generated ctypes.Structure has the C layout: size, and offset and size of every field, against a compile of the header
    structs = sorted(set(re.findall(r"typedef struct (ug_\w+)", hdr)))
    assert structs == sorted(lib.STRUCTS) and len(structs) >= 8
    named = dict(GemmDesc="ug_gemm_desc", ConvDesc="ug_conv_desc", VaeTile="ug_vae_tile", VaeBlendDesc="ug_vae_blend_desc", OptimTensor="ug_optim_tensor",
                 AdamwGroup="ug_adamw_group", OptimTensorLP="ug_optim_tensor_lp", AdamwGroupLP="ug_adamw_group_lp")
    assert all(getattr(lib, py) is lib.STRUCTS[c] for py, c in named.items())
    rows = [(s, f) for s in structs for f, _ in lib.STRUCTS[s]._fields_]
    assert len(rows) >= 130 and [f for s, f in rows if s == "ug_gemm_desc"][:4] == ["A", "lda", "a_rpb", "a_bstride"]
    src = '#include "unigen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){\n'
    src += "".join(f'printf("%zu\\n", sizeof({s}));\n' for s in structs)
    src += "".join(f'printf("%zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));\n' for s, f in rows) + "return 0;}\n"
    exe = str(tmp_path / "ug_layout_check")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = [tuple(map(int, ln.split())) for ln in subprocess.run([exe], capture_output=True, check=True, text=True).stdout.splitlines()]
    assert got[:len(structs)] == [(ctypes.sizeof(lib.STRUCTS[s]),) for s in structs]
    assert got[len(structs):] == [(getattr(lib.STRUCTS[s], f).offset, getattr(lib.STRUCTS[s], f).size) for s, f in rows]


def test_error_codes_without_gpu_compute():
    """Argument validation happens before any launch: safe to call on a GPU-less box."""
    from unigen_amd import lib
    cdll = lib.load()
    assert cdll.ug_gemm_bf16(None, None) == lib.UG_ERR_BAD_SHAPE
    assert b"null descriptor" in cdll.ug_last_error()
    d = lib.GemmDesc()
    d.M, d.N, d.K = 8, 8, 72
    assert cdll.ug_gemm_bf16(ctypes.byref(d), None) == lib.UG_ERR_UNSUPPORTED
    assert cdll.ug_flash_attn_fwd(1, 8, 8, 1, 8, 8, 1, 8, 8, 1, 8, 8, 1, 1, 8, 8, 96, 1.0, None) == lib.UG_ERR_UNSUPPORTED
    with pytest.raises(lib.UniGenHipError):
        lib.check(lib.UG_ERR_UNSUPPORTED, "x")
    # round-2 entry points validate before launching too
    c = lib.ConvDesc()
    assert cdll.ug_conv2d_nhwc(None, None) == lib.UG_ERR_BAD_SHAPE and cdll.ug_conv2d_nhwc(ctypes.byref(c), None) == lib.UG_ERR_BAD_SHAPE
    c.x, c.w, c.out, c.B, c.H, c.W, c.Cin, c.Ho, c.Wo, c.Cout, c.KH, c.KW, c.stride, c.pad_t, c.pad_l = 16, 16, 16, 1, 8, 8, 48, 8, 8, 64, 3, 3, 1, 1, 1
    assert cdll.ug_conv2d_nhwc(ctypes.byref(c), None) == lib.UG_ERR_UNSUPPORTED and b"multiple of 64" in cdll.ug_last_error()
    c.Cin, c.Ho = 64, 12
    assert cdll.ug_conv2d_nhwc(ctypes.byref(c), None) == lib.UG_ERR_BAD_SHAPE and b"output larger" in cdll.ug_last_error()
    assert cdll.ug_groupnorm_nhwc(16, 16, 16, 16, 16, 1 << 20, 1, 64, 96, 32, 1e-6, 0, None) == lib.UG_ERR_UNSUPPORTED      # 3 channels per group
    assert cdll.ug_groupnorm_nhwc(16, 16, 16, 16, 16, 8, 1, 64, 64, 32, 1e-6, 0, None) == lib.UG_ERR_BAD_SHAPE             # workspace too small
    assert cdll.ug_groupnorm_workspace_bytes(2, 1000, 32) >= 2 * 16 * 32 * 16
    assert cdll.ug_pack_latents(16, 16, 1, 16, 7, 8, None) == lib.UG_ERR_BAD_SHAPE                                           # odd height
    assert cdll.ug_probe_mfma_bf16(2, 256, 10, 16, None, None) == lib.UG_ERR_BAD_SHAPE
    assert cdll.ug_gemm_f32(None, None) == lib.UG_ERR_BAD_SHAPE and cdll.ug_flash_attn_fwd_f32(16, 4, 4, 16, 4, 4, 16, 4, 4, 16, 4, 4, 1, 1, 8, 8, 96, 1.0, None) == lib.UG_ERR_UNSUPPORTED
    # backward-pass entry points (training row)
    assert cdll.ug_transpose(16, 4, 0, 16, 4, 0, 1, 8, 8, 8, None) == lib.UG_ERR_BAD_SHAPE                                   # ld_src < cols
    assert cdll.ug_colsum(16, 64, None, 0, 16, 64, 10, 64, 4, 1.0, 16, 1 << 20, None) == lib.UG_ERR_BAD_SHAPE               # rows not a multiple of the group
    assert cdll.ug_colsum(16, 60, None, 0, 16, 60, 8, 60, 4, 1.0, 16, 1 << 20, None) == lib.UG_ERR_BAD_ALIGN                # cols % 8
    assert cdll.ug_colsum(16, 64, None, 0, 16, 64, 8, 64, 4, 1.0, 16, 8, None) == lib.UG_ERR_BAD_SHAPE and b"workspace" in cdll.ug_last_error()
    assert cdll.ug_colsum_workspace_bytes(4608, 3072, 4608) == 36 * 3072 * 4
    assert cdll.ug_qk_rmsnorm_rope_bwd(16, 128, 16, 128, 16, 128, None, 16, None, None, 4, 4, 0, 1, 128, 1e-6, None) == lib.UG_ERR_BAD_SHAPE   # weight without dwx
    assert cdll.ug_attn_prob(16, 64, 16, 16, 64, 4, 64, 65, 1.0, None) == lib.UG_ERR_BAD_SHAPE                               # valid_cols > cols
    args = [16, 128, 1024] * 8
    assert cdll.ug_flash_attn_bwd(*args, 1, 1, 8, 8, 96, 1.0, None, 16, 1 << 20, None) == lib.UG_ERR_UNSUPPORTED            # head dim
    assert cdll.ug_flash_attn_bwd(*args, 1, 1, 8, 8, 128, 1.0, None, 16, 8, None) == lib.UG_ERR_BAD_SHAPE and b"workspace" in cdll.ug_last_error()
    assert cdll.ug_flash_attn_fwd_lse(16, 128, 1024, 16, 128, 1024, 16, 128, 1024, 16, 128, 1024, 1, 1, 8, 8, 128, 1.0, 16, 4, None) == lib.UG_ERR_BAD_SHAPE   # lse_ld < Lq
    assert cdll.ug_flash_attn_bwd_workspace_bytes(2, 24, 4608) == 2 * 2 * 24 * 4608 * 4
    assert cdll.ug_gelu_tanh_bwd_f32(None, 16, 16, 8, None) == lib.UG_ERR_BAD_SHAPE
    assert cdll.ug_qk_rmsnorm_rope_bwd_partials(9216, 24) == 2048 and cdll.ug_qk_rmsnorm_rope_bwd_partials(3, 2) == 2      # capped / one block per 4 vectors
    assert cdll.ug_adaln_modulate_bwd_partials(9216, 4608) == 512 and cdll.ug_adaln_modulate_bwd_partials(70000, 1) == 1 and cdll.ug_adaln_modulate_bwd_partials(20, 10) == 3
    assert cdll.ug_adaln_modulate_bwd(16, 64, 16, 64, 16, 64, 4, 16, 64, None, 8, 64, 1e-6, None) == lib.UG_ERR_BAD_SHAPE                 # no partials buffer
    assert cdll.ug_adaln_modulate_bwd(16, 8192, 16, 8192, 16, 8192, 4, 16, 8192, 16, 8, 8192, 1e-6, None) == lib.UG_ERR_BAD_ALIGN and b"4096" in cdll.ug_last_error()
    assert cdll.ug_qk_rmsnorm_rope_bwd(16, 1024, 16, 1024, 16, 1024, 16, 16, None, None, 4, 4, 0, 1, 1024, 1e-6, None) == lib.UG_ERR_UNSUPPORTED   # head width > 256
    assert cdll.ug_moe_gate_bwd(16, 16, 16, 16, 64, 16, 4, 64, 17, 16, 64, 16, None) == lib.UG_ERR_BAD_SHAPE and b"E <= 16" in cdll.ug_last_error()  # 17 experts
    assert cdll.ug_moe_gate_bwd(16, 16, 16, 16, 64, 16, 4, 60, 16, 16, 64, 16, None) == lib.UG_ERR_BAD_ALIGN                # D % 8
    assert cdll.ug_moe_gate_bwd_f32(16, 16, 16, 16, 64, 16, 4, 60, 2, 16, 64, 16, None) == lib.UG_ERR_BAD_ALIGN
    assert cdll.ug_rowdot(16, 191, 16, 192, 16, 4, 3, 64, None) == lib.UG_ERR_BAD_SHAPE                                      # lda < groups * cols
    assert cdll.ug_rowdot_f32(16, 192, 16, 191, 16, 4, 3, 64, None) == lib.UG_ERR_BAD_SHAPE                                  # ldb < groups * cols
    assert cdll.ug_adaln_modulate_bwd(16, 4104, 16, 4104, 16, 4104, 4, 16, 4104, 16, 8, 4104, 1e-6, None) == lib.UG_ERR_BAD_ALIGN and b"4096" in cdll.ug_last_error()


def test_forward_projection_abi_rejections():
    """The fused q/k epilogue, the LoRA segment and the stand-alone q/k pass refuse what they do not implement, before any launch (fake,
    aligned pointers: every descriptor below differs from a valid one in exactly the field under test)."""
    from unigen_amd import lib
    cdll = lib.load()
    P = 4096

    def qkv(**kw):
        d = lib.GemmDesc()
        d.A, d.W, d.C, d.lda, d.ldw, d.ldc, d.M, d.N, d.K = P, P, P, 64, 64, 768, 256, 768, 64
        d.epilogue, d.qk_wq, d.qk_wk, d.rope_cs, d.qk_until_n, d.qk_dh, d.qk_eps = lib.EPI_QKV_ROPE, P, P, P, 512, 128, 1e-6
        for k, v in kw.items():
            setattr(d, k, v)
        rc = cdll.ug_gemm_bf16(ctypes.byref(d), None)
        return rc, cdll.ug_last_error()

    lora = dict(lora_T=P, ldt=64, lora_B=P, ldb=64, lora_r=64)
    rc, msg = qkv(**lora)
    assert rc == lib.UG_ERR_UNSUPPORTED and b"LoRA" in msg
    rc, msg = qkv(groups=2)
    assert rc == lib.UG_ERR_UNSUPPORTED and b"grouped" in msg
    for rpb in (1, 128, 255):                                               # positions would wrap more than once per 16-row group
        assert qkv(rope_rpb=rpb)[0] == lib.UG_ERR_BAD_SHAPE
    rc, msg = qkv(c_rpb=448, c_bstride=512)                                 # the C row map would split a 256-row tile
    assert rc == lib.UG_ERR_UNSUPPORTED and b"multiple of 256" in msg
    assert qkv(gelu_from_n=256)[0] == lib.UG_ERR_BAD_SHAPE                  # GELU inside the q | k columns
    assert qkv(c_shift_from_n=256, c_shift=8, ldc=776)[0] == lib.UG_ERR_BAD_SHAPE
    assert qkv(qk_dh=96)[0] == lib.UG_ERR_UNSUPPORTED
    assert qkv(rope_cs=None)[0] == lib.UG_ERR_BAD_ALIGN                     # the table may only be omitted at head width 64
    # the LoRA segment of the plain epilogues
    rc, msg = qkv(epilogue=lib.EPI_BIAS, **dict(lora, lora_r=96))
    assert rc == lib.UG_ERR_UNSUPPORTED and b"lora_r" in msg
    rc, msg = qkv(epilogue=lib.EPI_BIAS, groups=2, **lora)
    assert rc == lib.UG_ERR_UNSUPPORTED and b"not grouped" in msg
    assert qkv(epilogue=lib.EPI_BIAS, **dict(lora, ldt=60))[0] == lib.UG_ERR_BAD_ALIGN
    # ug_qk_rmsnorm_rope(buf, ld, batches, rows_per_batch, batch_stride_rows, pos_offset, q_off, k_off, heads, dh, wq_a, wk_a, wq_b, wk_b, split,
    #                    cos, sin, eps, stream)
    qk = lambda dh=128, wq_b=P, wk_b=P, cos=P, sin=P, q_off=0: cdll.ug_qk_rmsnorm_rope(P, 768, 1, 16, 16, 0, q_off, 256, 2, dh, None, None, wq_b, wk_b,
                                                                                       0, cos, sin, 1e-6, None)
    assert qk(dh=96) == lib.UG_ERR_UNSUPPORTED
    assert qk(sin=None) == lib.UG_ERR_BAD_SHAPE and qk(cos=None) == lib.UG_ERR_BAD_SHAPE
    assert qk(wk_b=None) == lib.UG_ERR_BAD_SHAPE and b"pairs" in cdll.ug_last_error()
    assert qk(wq_b=None) == lib.UG_ERR_BAD_SHAPE


def test_no_cpu_fallback():
    from unigen_amd import lib, ops
    a = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(lib.UniGenHipError, match="GPU tensor"):
        ops.gemm(a, a, None, torch.zeros(8, 8, dtype=torch.bfloat16), M=8)
    # no product module (unigen_amd/*.py, src/*.py) may import or name the oracle package; prose may say "the oracle"
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "unigen_amd", "*.py")) + glob.glob(os.path.join(ROOT, "src", "*.py")))
    assert len(files) >= 12, files
    for fn in files:
        text = open(fn).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f"{fn} imports the oracle"
        assert "oracle" not in re.sub(r"(the|fp32|bf16|CPU) oracle('s)?", "", text), f"{fn} must not reference the oracle package"
    # and the CSRC never falls back either: no host compute path in the library
    for fn in glob.glob(os.path.join(ROOT, "unigen_amd", "csrc", "*.hip")):
        assert "oracle" not in open(fn).read().replace("the oracle", "")


def _model(n_cond=1, cls="UniGenFlux", **ctl):
    m = getattr(importlib.import_module("src.UniGenTransformer"), cls).from_config(dict(TINY))
    cp = dict(CONTROL); cp.update(ctl)
    m.init_condition_block(condition_nums=n_cond, condition_types=["canny", "depth", "openpose"][:n_cond], control_params=cp)
    return m


def test_dropin_names_and_state_dict_keys():
    from oracle import unigen_ref as R
    mt = importlib.import_module("src.UniGenTransformer")
    assert {"UniGenFlux", "MultiCondtionUniGenFlux"} <= set(dir(mt))
    mp = importlib.import_module("src.UniGenPipeline")
    assert hasattr(mp, "UniGenFLUXPipeline")
    m = _model()
    sd = m.state_dict()
    ref = R.state_shapes(R.FluxConfig(**TINY))
    assert set(sd) == set(ref) and all(tuple(sd[k].shape) == tuple(ref[k]) for k in ref)
    for k in ("transformer_blocks.0.attn.to_q.weight", "single_transformer_blocks.3.proj_out.bias", "control_joint_trans_blocks.0.ff_context.net.2.weight",
              "controlnet_add_single_blocks.1.weight", "moe.moe_layer.gate.wg.weight", "moe.moe_layer.experts.deepspeed_experts.5.1.1.bias",
              "shared_expert.1.attn.norm_added_k.weight", "control_condition_embed.text_embedder.linear_2.weight", "norm_out.linear.weight"):
        assert k in sd
    assert m.config.in_channels == 64 and m.config.guidance_embeds is False and m.dtype == torch.bfloat16
    assert set(m.trainable_control_modules) >= {"control_x_embedder", "control_joint_trans_blocks", "moe", "shared_expert"}
    m3 = _model(3, "MultiCondtionUniGenFlux")
    assert m3.state_dict()["moe.moe_layer.gate.wg.weight"].shape[0] == 12            # (3 + 1) * 3 experts
    # full FLUX geometry: parameter count of the headline configuration (no allocation: shapes only)
    from unigen_amd.flux import base_param_shapes, control_param_shapes, FLUX_SCHNELL_CONFIG
    from types import SimpleNamespace
    cfg = SimpleNamespace(**FLUX_SCHNELL_CONFIG)
    ctl = SimpleNamespace(cn_joint_layers=9, cn_single_layers=19, use_single_trans_blocks=True, expert_nums=6, use_shared_expert=True)
    n = sum(int(torch.Size(s).numel()) for s in {**base_param_shapes(cfg), **control_param_shapes(cfg, ctl)}.values())
    assert 18.0e9 < n < 19.5e9, n


def test_config_errors_mirror_reference_constraints():
    cls = importlib.import_module("src.UniGenTransformer").UniGenFlux
    m = cls.from_config(dict(TINY))
    with pytest.raises(AssertionError):
        m.init_condition_block(condition_nums=1)                                       # control_params missing (reference :718)
    with pytest.raises(ValueError, match="use_rope"):
        m.init_condition_block(condition_nums=1, control_params=dict(use_rope=False))
    with pytest.raises(RuntimeError, match="init_condition_block"):
        cls.from_config(dict(TINY))(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="axes_dims_rope"):
        cls.from_config(dict(TINY, attention_head_dim=64))


def test_packing_keeps_state_dict_and_load_state_dict(tmp_path):
    m = _model()
    m.init_synthetic_(seed=2, std=0.05, bias_std=0.02)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    w, b = m._attn_qkv("transformer_blocks.0.attn")
    assert w.shape == (3 * 256, 256) and m.get_parameter("transformer_blocks.0.attn.to_k.weight").data_ptr() == w[256:].data_ptr()
    ws = m._pack_stack("moe.wc", [f"moe.moe_layer.experts.deepspeed_experts.{e}.0.0.weight" for e in range(6)])
    assert ws.shape == (6, 256, 256)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # loading new weights writes through the packed views
    new = {k: torch.randn_like(v.float()).to(v.dtype) for k, v in before.items()}
    res = m.load_state_dict(new, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m._attn_qkv("transformer_blocks.0.attn")[0][256:512], new["transformer_blocks.0.attn.to_k.weight"])
    # from_pretrained: local dir with config.json + safetensors (base weights only), then control init + strict=False load
    from safetensors.torch import save_file
    d = tmp_path / "transformer"
    d.mkdir()
    base = {k: v.contiguous() for k, v in new.items() if not (k.startswith("control") or k.startswith("moe.") or k.startswith("shared_expert"))}
    save_file(base, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(dict(TINY, in_channels=64, guidance_embeds=False, axes_dims_rope=[16, 56, 56])))
    cls = importlib.import_module("src.UniGenTransformer").UniGenFlux
    m2 = cls.from_pretrained(pretrained_model_name_or_path=str(tmp_path), subfolder="transformer")
    assert torch.equal(m2.state_dict()["x_embedder.weight"], new["x_embedder.weight"])
    with pytest.raises(OSError):
        cls.from_pretrained("black-forest-labs/FLUX.1-schnell")


def test_pipeline_schedule_and_pack_roundtrip():
    from unigen_amd import pipeline as P
    assert P.flow_match_sigmas(4) == [1.0, 0.75, 0.5, 0.25, 0.0]
    assert len(P.flow_match_sigmas(28)) == 29 and abs(P.flow_match_sigmas(28)[-2] - 1 / 28) < 1e-12
    mu = P.calculate_shift(4096)
    assert abs(mu - 1.15) < 1e-9
    s = P.flow_match_sigmas(4, use_dynamic_shifting=True, mu=mu)
    assert s[0] == 1.0 and 0.25 < s[3] < 1.0
    # the pipeline hands the scheduler's own base / max lengths and shifts to the loop (src/UniGenPipeline.py:663-670); a config that names none gets diffusers' defaults
    pp = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline(scheduler_config=dict(use_dynamic_shifting=True, base_shift=0.4, max_shift=1.0))
    sc = pp.scheduler.config
    assert (sc["base_image_seq_len"], sc["max_image_seq_len"], sc["base_shift"], sc["max_shift"]) == (256, 4096, 0.4, 1.0)
    assert abs(P.calculate_shift(4096, sc["base_image_seq_len"], sc["max_image_seq_len"], sc["base_shift"], sc["max_shift"]) - 1.0) < 1e-9
    x = torch.randn(2, 16, 8, 12)
    p = P.pack_latents(x)
    assert p.shape == (2, 24, 64) and torch.equal(P.unpack_latents(p, 64, 96, 8), x)
    ids = P.prepare_latent_image_ids(3, 4, "cpu", torch.bfloat16)
    from oracle import unigen_ref as R
    assert torch.equal(ids, R.make_ids(3, 4))
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=None)
    assert pipe.transformer is None and pipe.vae_scale_factor == 8
    pipe.transformer = _model()
    with pytest.raises(NotImplementedError, match="encode_prompt"):           # text given, no encoder attached
        pipe(prompt="a cat", condition_prompt="canny", control_image=torch.zeros(1, 4, 64))
    with pytest.raises(NotImplementedError, match="VAE"):                      # pixels given, no VAE attached
        pipe(prompt_embeds=torch.zeros(1, 8, 64), pooled_prompt_embeds=torch.zeros(1, 64), condition_pooled_prompt_embeds=torch.zeros(1, 64),
             control_image=torch.zeros(1, 3, 64, 64))


def test_pipeline_call_delegates_to_attached_encoders_and_vae(monkeypatch):
    """infer.py:204-216 call shape: pipe(prompt=, condition_prompt=, control_image=<pixels>, height, width, num_inference_steps, guidance_scale,
    max_sequence_length, dtype, generator).images with the caller's text encoders and VAE attached. The denoise loop itself needs the GPU
    (tests/test_flux_gpu.py); here it is replaced by a recorder so the delegation runs on the CPU."""
    from types import SimpleNamespace
    from unigen_amd import pipeline as P
    calls = []

    def encode_prompt(prompt=None, prompt_2=None, prompt_embeds=None, pooled_prompt_embeds=None, device=None, num_images_per_prompt=1,
                      max_sequence_length=512, lora_scale=None):
        calls.append(("encode", prompt, max_sequence_length))
        n = len(prompt) if isinstance(prompt, (list, tuple)) else 1
        return torch.full((n, max_sequence_length, 64), 0.5), torch.full((n, 64), 0.25), torch.zeros(max_sequence_length, 3)

    class VAE:
        dtype = torch.bfloat16
        config = SimpleNamespace(scaling_factor=0.3611, shift_factor=0.1159)

        def encode(self, x):
            calls.append(("vae.encode", tuple(x.shape)))
            z = torch.arange(x.shape[0] * 16 * (x.shape[2] // 8) * (x.shape[3] // 8), dtype=torch.float32).view(x.shape[0], 16, x.shape[2] // 8, x.shape[3] // 8) / 100
            return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: z.to(torch.bfloat16)))

        def decode(self, z, return_dict=False):
            calls.append(("vae.decode", tuple(z.shape)))
            return (z[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3),)

    def fake_loop(tr, **kw):
        calls.append(("loop", {k: (tuple(v.shape) if torch.is_tensor(v) else v) for k, v in kw.items() if k in
                               ("latents", "control_tokens", "prompt_embeds", "pooled_prompt_embeds", "condition_pooled_prompt_embeds", "num_inference_steps")}))
        fake_loop.control = kw["control_tokens"]
        return kw["latents"]

    monkeypatch.setattr(P, "denoise_loop", fake_loop)
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=None)
    pipe.transformer = _model()
    pipe.encode_prompt, pipe.vae = encode_prompt, VAE()
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, 64, 96) * 2 - 1
    res = pipe(prompt=["a cat", "a dog"], condition_prompt=["canny", "canny"], control_image=img, height=64, width=96, num_inference_steps=4,
               guidance_scale=3.5, max_sequence_length=16, dtype=torch.bfloat16, generator=g, output_type="pt")
    kinds = [c[0] for c in calls]
    assert kinds == ["encode", "encode", "vae.encode", "loop", "vae.decode"], kinds
    assert calls[0][1] == ["a cat", "a dog"] and calls[1][1] == ["canny", "canny"] and calls[0][2] == 16
    loop = calls[3][1]
    assert loop["latents"] == (2, 4 * 6, 64) and loop["control_tokens"] == (2, 24, 64) and loop["prompt_embeds"] == (2, 16, 64)
    assert loop["condition_pooled_prompt_embeds"] == (2, 64) and loop["num_inference_steps"] == 4
    # the control tokens are pack((z - shift) * scale) of what the VAE returned (src/UniGenPipeline.py:635-647)
    z = VAE().encode(img).latent_dist.sample()
    exp = P.pack_latents(((z - 0.1159) * 0.3611).to(torch.bfloat16))
    assert torch.equal(fake_loop.control, exp)
    assert res.images.shape == (2, 3, 64, 96)                                  # unpack -> / scale + shift -> decode
    # pre-computed embeds + packed latents still work without any attachment, as in round 1
    pipe2 = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=_model())
    out = pipe2(prompt_embeds=torch.zeros(1, 8, 64), pooled_prompt_embeds=torch.zeros(1, 64), condition_pooled_prompt_embeds=torch.zeros(1, 64),
                control_image=torch.zeros(1, 16, 64), height=64, width=64, num_inference_steps=2)
    assert out.images.shape == (1, 16, 64)


def test_pipeline_call_prepares_the_control_image_as_the_reference_does(monkeypatch):
    """src/UniGenPipeline.py:622-657 / :293-316: ONE control image serves every prompt of the batch (repeat to batch_size x num_images_per_prompt), the
    latents take the PREPARED image's height / width (not the arguments'), and the SD3 pipeline doubles the image batch under classifier-free
    guidance and widens a one-channel depth map to three channels before the VAE."""
    from types import SimpleNamespace
    from unigen_amd import pipeline as P
    seen = {}

    class VAE:
        dtype = torch.bfloat16
        config = SimpleNamespace(scaling_factor=0.5, shift_factor=0.25)

        def encode(self, x):
            seen["vae_in"] = tuple(x.shape)
            z = x[:, :1].float().mean(dim=(2, 3), keepdim=True).expand(x.shape[0], 16, x.shape[2] // 8, x.shape[3] // 8)
            return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: z.to(torch.bfloat16)))

    def fake_loop(tr, **kw):
        seen["latents"], seen["control"] = tuple(kw["latents"].shape), kw.get("control_tokens", kw.get("control_latents"))
        return kw["latents"]

    monkeypatch.setattr(P, "denoise_loop", fake_loop)
    monkeypatch.setattr(P, "sd3_denoise_loop", fake_loop)
    mod = importlib.import_module("src.UniGenPipeline")
    pipe = mod.UniGenFLUXPipeline.from_pretrained(None, transformer=_model())
    pipe.vae = VAE()
    img = torch.full((1, 3, 32, 48), 0.75)
    emb = dict(prompt_embeds=torch.zeros(3, 8, 64), pooled_prompt_embeds=torch.zeros(3, 64), condition_pooled_prompt_embeds=torch.zeros(3, 64))
    pipe(control_image=img, height=64, width=64, num_inference_steps=2, **emb)           # height / width arguments disagree with the tensor: the tensor wins
    assert seen["vae_in"] == (3, 3, 32, 48) and seen["latents"] == (3, 2 * 3, 64) and tuple(seen["control"].shape) == (3, 6, 64)
    assert torch.equal(seen["control"], torch.full((3, 6, 64), 0.25, dtype=torch.bfloat16))          # (0.75 - 0.25) * 0.5 for every repeated sample
    # SD3: CFG doubles the prepared batch, the latents stay at one copy per sample; a one-channel map reaches the VAE with three channels
    sd3 = mod.UniGenSD3Pipeline.from_pretrained(None, transformer=SimpleNamespace(device=torch.device("cpu"), dtype=torch.bfloat16, config=SimpleNamespace(in_channels=16)))
    sd3.vae = VAE()
    depth = torch.full((1, 1, 32, 32), 0.75)
    e3 = dict(prompt_embeds=torch.zeros(2, 8, 64), pooled_prompt_embeds=torch.zeros(2, 64), negative_prompt_embeds=torch.zeros(2, 8, 64),
              negative_pooled_prompt_embeds=torch.zeros(2, 64), condition_pooled_prompt_embeds=torch.zeros(2, 64))
    sd3(control_image=depth, guidance_scale=7.0, num_inference_steps=2, **e3)
    assert seen["vae_in"] == (4, 3, 32, 32) and seen["latents"] == (2, 16, 4, 4) and tuple(seen["control"].shape) == (4, 16, 4, 4)
    sd3(control_image=depth, guidance_scale=1.0, num_inference_steps=2, **{k: v for k, v in e3.items() if not k.startswith("negative")})
    assert seen["vae_in"] == (2, 3, 32, 32) and seen["latents"] == (2, 16, 4, 4)
    sd3(control_image=torch.zeros(2, 16, 4, 4), guidance_scale=7.0, num_inference_steps=2, **e3)        # VAE latents pass through, one copy per sample
    assert seen["latents"] == (2, 16, 4, 4) and tuple(seen["control"].shape) == (2, 16, 4, 4)


def test_rope_cache_is_keyed_on_content_identity():
    """RoPE tables were cached by (data_ptr, shape, dtype) of the ids tensors; a freed 4 x 2 grid's ids and a fresh 2 x 4
    grid's (same N, same shape) can share an address. The cache entry now keeps the ids alive and tracks `_version`."""
    from unigen_amd import pipeline as P
    m = _model()
    txt = torch.zeros(4, 3, dtype=torch.bfloat16)
    ids1 = P.prepare_latent_image_ids(4, 2, "cpu", torch.bfloat16)
    c1, s1 = m._rope([txt, ids1], None)
    c1, s1 = c1.clone(), s1.clone()
    p1 = ids1.data_ptr()
    del ids1                                            # the cache still references it: its storage cannot be recycled
    ids2 = P.prepare_latent_image_ids(2, 4, "cpu", torch.bfloat16)
    assert ids2.data_ptr() != p1
    c2, s2 = m._rope([txt, ids2], None)
    from oracle import unigen_ref as R
    rc, rs = R.flux_pos_embed(torch.cat([txt, ids2], 0), m.config.axes_dims_rope)
    assert torch.equal(c2, rc) and torch.equal(s2, rs) and not torch.equal(c2, c1)
    assert m._rope([txt, ids2], None)[0] is c2          # a hit on the same tensors
    ids2[:, 1] += 1                                     # in-place edit: _version moves, the entry is not reused
    c3, _ = m._rope([txt, ids2], None)
    assert torch.equal(c3, R.flux_pos_embed(torch.cat([txt, ids2], 0), m.config.axes_dims_rope)[0]) and not torch.equal(c3, c2)


def test_sd3_default_sigmas_match_diffusers_0_32_2():
    """FlowMatchEulerDiscreteScheduler(shift=3).set_timesteps(28) of diffusers 0.32.2 (the release the reference pins): the scheduler's
    training sigmas are shifted in __init__ (sigma_min = 0.0029940), the linspace runs between THOSE, then the shift is applied again.
    Literal values computed from that release's formulas (numpy, float32 storage); ADVICE r1: the last sigma is 0.0089, not 0.0030."""
    from unigen_amd import pipeline as P
    lit = [1.0, 0.9873806, 0.9741077, 0.9601293, 0.9453875, 0.9298179, 0.913349, 0.8959003, 0.8773819, 0.8576923, 0.8367167, 0.8143248, 0.7903683,
           0.7646771, 0.7370558, 0.7072785, 0.6750823, 0.6401602, 0.6021506, 0.560625, 0.5150721, 0.464876, 0.4092888, 0.3473926, 0.2780488, 0.199827,
           0.1109057, 0.0089286]
    sig = P.flow_match_sigmas(28, sigmas=P.sd3_default_sigmas(28, 3.0), shift=3.0)
    assert len(sig) == 29 and sig[-1] == 0.0
    assert max(abs(a - b) for a, b in zip(sig, lit)) < 1e-6


def test_both_denoise_loops_run_the_transformer_without_autograd(monkeypatch):
    """`@torch.no_grad()` of the reference's pipeline `__call__`s (src/UniGenPipeline.py:143, 486) sits on BOTH loops here: a model whose
    control modules require grad (after `init_trainable_param()`) must still take the inference forward inside the sampling loop, with no
    graph kept across the steps (the decorator had slipped onto a helper above `sd3_denoise_loop`)."""
    from types import SimpleNamespace
    from unigen_amd import ops, pipeline as P
    seen = []

    class Fake:
        config = SimpleNamespace(guidance_embeds=False)

        def __call__(self, hidden_states=None, **kw):
            seen.append(torch.is_grad_enabled())
            return (torch.zeros_like(hidden_states),)

    monkeypatch.setattr(ops, "euler_step", lambda lat, pred, dt: lat)
    monkeypatch.setattr(ops, "cfg_combine", lambda a, b, s, out: out)
    w = torch.nn.Parameter(torch.ones(1))              # something that requires grad is alive while the loops run
    with torch.enable_grad():
        P.denoise_loop(Fake(), latents=torch.zeros(1, 4, 8) * w.detach(), control_tokens=torch.zeros(1, 4, 8), prompt_embeds=torch.zeros(1, 2, 8),
                       pooled_prompt_embeds=torch.zeros(1, 8), condition_pooled_prompt_embeds=torch.zeros(1, 8), text_ids=torch.zeros(2, 3),
                       latent_image_ids=torch.zeros(4, 3), condition_ids=torch.zeros(4, 3), num_inference_steps=2)
        n_flux = len(seen)
        P.sd3_denoise_loop(Fake(), latents=torch.zeros(1, 4, 4, 4), control_latents=torch.zeros(1, 4, 4, 4), prompt_embeds=torch.zeros(2, 2, 8),
                           pooled_prompt_embeds=torch.zeros(2, 8), condition_pooled_prompt_embeds=torch.zeros(2, 8), num_inference_steps=3)
        assert torch.is_grad_enabled()
    assert n_flux == 2 and len(seen) == 5 and not any(seen)
    # the helpers that sit next to the loops are plain functions
    assert P.sd3_default_sigmas_unshifted(4)[0] == 1.0 and P.control_keep(4, 0.0, 0.5) == [1.0, 1.0, 0.0, 0.0]


def test_vae_dropin_names_and_loading(tmp_path):
    """unigen_amd.vae.AutoencoderKL keeps diffusers' parameter names / shapes (FLUX VAE: 83.8 M parameters) and loads the diffusers directory layout."""
    from types import SimpleNamespace
    from oracle import vae_ref as V
    from safetensors.torch import save_file
    from unigen_amd.vae import AutoencoderKL, FLUX_VAE_CONFIG, vae_param_shapes
    full = vae_param_shapes(SimpleNamespace(**FLUX_VAE_CONFIG))
    assert full == V.vae_state_shapes(V.VAEConfig()) and sum(int(torch.Size(s).numel()) for s in full.values()) == 83819683
    for k in ("encoder.down_blocks.1.resnets.0.conv_shortcut.weight", "encoder.down_blocks.2.downsamplers.0.conv.bias", "decoder.mid_block.attentions.0.to_out.0.weight",
              "decoder.up_blocks.2.upsamplers.0.conv.weight", "decoder.conv_norm_out.bias", "encoder.conv_out.weight"):
        assert k in full
    tiny = dict(block_out_channels=(64, 128), layers_per_block=1)
    m = AutoencoderKL.from_config(tiny)
    assert m.config.scaling_factor == 0.3611 and m.config.shift_factor == 0.1159 and m.dtype == torch.bfloat16
    st = V.make_vae_state(V.VAEConfig(**tiny), seed=1)
    d = tmp_path / "vae"; d.mkdir()
    save_file({k: v.contiguous() for k, v in st.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(dict(tiny, latent_channels=16, scaling_factor=1.5305, shift_factor=0.0609, _class_name="AutoencoderKL")))
    m2 = AutoencoderKL.from_pretrained(str(tmp_path), subfolder="vae")
    assert m2.config.scaling_factor == 1.5305 and all(torch.equal(m2.state_dict()[k], st[k]) for k in st)
    wp, bp = m2._conv_w("encoder.conv_in")                # packed [Cout_p, KH, KW, Cin_p]: channels zero-padded to the conv's K granularity
    assert wp.shape == (64, 3, 3, 64) and torch.equal(wp[:, :, :, :3], st["encoder.conv_in.weight"].permute(0, 2, 3, 1)) and float(wp[:, :, :, 3:].abs().max()) == 0
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(str(tmp_path), transformer=None)
    assert isinstance(pipe.vae, AutoencoderKL)
    with pytest.raises(Exception):
        m2.encode(torch.zeros(1, 3, 32, 32))              # no CPU path


def test_shard_ranges_cover_the_global_batch():
    from unigen_amd.dist_utils import shard_range
    for G, W in ((64, 8), (64, 1), (10, 4), (3, 8)):
        spans = [shard_range(G, r, W) for r in range(W)]
        assert spans[0][0] == 0 and spans[-1][1] == G and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(b - a for a, b in spans) - min(b - a for a, b in spans) <= 1
    assert shard_range(64, 3, 8) == (24, 32)


_WORKER = r"""
import os, sys, time, torch
sys.path.insert(0, %r)
from unigen_amd import dist_utils as DU
dev = torch.device("cpu")
rank, world = DU.init_distributed(dev)
a, b = DU.shard_range(10, rank, world)
DU.barrier(dev, world)
elapsed = 0.5 + rank            # pretend rank 1 is slower
mx = DU.max_over_ranks(elapsed, dev, world)
tot = DU.sum_over_ranks(b - a, dev, world)
assert mx == 1.5 and tot == 10 and DU.rank_seed(12443, rank) == 12443 + rank, (mx, tot)
rec = DU.all_gather_floats([b - a, elapsed, rank], dev, world)
assert rec == [[5.0, 0.5, 0.0], [5.0, 1.5, 1.0]], rec
DU.barrier(dev, world)
if rank == 0:
    print("GLOO_OK", world, mx, tot)
"""


def test_two_rank_gloo_harness(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "GLOO_OK 2 1.5 10.0" in r.stdout


def test_enable_lora_context_manager_semantics():
    """src/lora_switching_module.py: non-enabled adapters are zeroed inside the context; exit restores THROUGH set_scale, i.e. scales
    by lora_alpha / r once more - idempotent only when alpha == r, kept as the reference has it."""
    mod = importlib.import_module("src.lora_switching_module")
    lin = mod.LoRALinear(64, 32)
    lin.add_adapter("canny", r=4, lora_alpha=4)
    lin.add_adapter("depth", r=4, lora_alpha=8)
    assert mod.module_active_adapters(lin) == ["canny", "depth"] and lin.scaling == {"canny": 1.0, "depth": 2.0}
    with mod.enable_lora([lin, object()], ["canny"]):
        assert lin.scaling == {"canny": 1.0, "depth": 0.0}
        A, Bm = lin._fused_adapters()
        assert A.shape == (64, 64) and Bm.shape == (32, 64)          # one active adapter, rank padded to 64
    assert lin.scaling == {"canny": 1.0, "depth": 4.0}                # 2.0 * (alpha / r = 2): the reference's restore quirk
    assert mod.module_active_adapters(object()) == []


def test_add_lora_makes_the_projections_peft_shaped_layers_enable_lora_switches():
    """A12 on the hot path: `HipModule.add_lora` turns the holders of the named projections into PEFT-shaped layers that
    `enable_lora(list(model.modules()), [...])` - the reference's call shape, src/lora_switching_module.py:11-38 - finds and switches; the base
    parameters stay the same objects under the same state-dict keys; targets the engine cannot extend are refused, not ignored."""
    from unigen_amd import lib as L
    from unigen_amd.lora import LoRALayer, fuse_adapters
    mod = importlib.import_module("src.lora_switching_module")
    m = _model(3, cls="MultiCondtionUniGenFlux")
    keys0 = set(m.state_dict())
    wq = m.get_parameter("control_joint_trans_blocks.0.attn.to_q.weight")
    assert mod.enable_lora(list(m.modules()), ["canny"]).lora_modules == []          # nothing attached yet (as on the reference without PEFT layers)
    specs = [("canny", 8, 16.0), ("depth", 4, 4.0), ("openpose", 16, 8.0)]
    for i, (name, r, alpha) in enumerate(specs):
        hits = m.add_lora(["attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0"], name, r, alpha, prefix="control_", init_lora_weights=False, seed=i)
    n_joint, n_single = m._ctl.cn_joint_layers, m._ctl.cn_single_layers
    assert len(hits) == 4 * n_joint + 3 * n_single and all(h.startswith("control_") for h in hits)
    assert m.get_parameter("control_joint_trans_blocks.0.attn.to_q.weight") is wq      # same Parameter object, same key
    new_keys = set(m.state_dict()) - keys0
    assert keys0 <= set(m.state_dict()) and len(new_keys) == 2 * 3 * len(hits)
    assert "control_joint_trans_blocks.0.attn.to_q.lora_A.canny.weight" in new_keys and "control_single_trans_blocks.1.attn.to_v.lora_B.openpose.weight" in new_keys
    layers = [x for x in m.modules() if isinstance(x, LoRALayer)]
    assert len(layers) == len(hits) and all(mod.module_active_adapters(x) == ["canny", "depth", "openpose"] for x in layers)
    lay = m.get_submodule("control_joint_trans_blocks.0.attn.to_q")
    assert lay.scaling == {"canny": 2.0, "depth": 1.0, "openpose": 0.5}
    ctx = mod.enable_lora(list(m.modules()), ["canny"])
    assert len(ctx.lora_modules) == len(hits)
    with ctx:
        assert lay.scaling == {"canny": 2.0, "depth": 0.0, "openpose": 0.0} and lay.live_adapters() == ["canny"]
        assert m._lora_live(["control_joint_trans_blocks.0.attn.to_q"]) and not m._lora_live(["transformer_blocks.0.attn.to_q"])
        A, Bm = fuse_adapters([lay, m.get_submodule("control_joint_trans_blocks.0.attn.to_k"), None], [256, 256, 256], torch.bfloat16, "cpu")
        assert A.shape == (64, 256) and Bm.shape == (768, 64)                       # 8 + 8 ranks, padded to the K-tile
        assert torch.equal(A[:8], lay.lora_A["canny"].weight) and not Bm[:256, 8:].any() and not Bm[256:512, :8].any() and not Bm[512:].any()
        assert torch.equal(Bm[:256, :8], (lay.lora_B["canny"].weight.float() * 2.0).to(torch.bfloat16))
        # the fused operands say what peft's LoRA Linear says, projection by projection (fp32): [x W^T | ...] + (x A_cat^T) B_bd^T
        from oracle import unigen_ref as R
        lk = m.get_submodule("control_joint_trans_blocks.0.attn.to_k")
        x = torch.randn(5, 256)
        A32, B32 = fuse_adapters([lay, lk, None], [256, 256, 256], torch.float32, "cpu")
        fusedy = (x @ A32.t()) @ B32.t()
        for j, ly in enumerate((lay, lk)):
            want = R.lora_linear(x, torch.zeros(256, 256), None, [(ly.lora_A["canny"].weight.float(), ly.lora_B["canny"].weight.float(), 2.0)])
            assert torch.allclose(fusedy[:, j * 256:(j + 1) * 256], want, atol=1e-5)
        assert not fusedy[:, 512:].any()
    # Q10: the reference "restores" through set_scale(saved scaling) = saved * alpha / r (idempotent only when alpha == r)
    assert lay.scaling == {"canny": 4.0, "depth": 1.0, "openpose": 0.25}
    # diffusers scale_lora_layers / unscale_lora_layers around a forward (joint_attention_kwargs["scale"])
    with m._lora_scaled({"scale": 0.5}):
        assert lay.scaling == {"canny": 2.0, "depth": 0.5, "openpose": 0.125}
    assert lay.scaling == {"canny": 4.0, "depth": 1.0, "openpose": 0.25}
    with pytest.raises(L.UniGenHipError, match="not a projection the HIP engine can extend"):
        m.add_lora(["norm1.linear"], "x", 4, 4.0)
    with pytest.raises(L.UniGenHipError, match="not a projection"):
        m.add_lora(["proj_out"], "x", 4, 4.0)                                        # the model's final proj_out (the single blocks' proj_out is fine under a prefix)
    assert m.add_lora(["proj_out", "proj_mlp"], "x", 4, 4.0, prefix="single_transformer_blocks.0.") == ["single_transformer_blocks.0.proj_mlp", "single_transformer_blocks.0.proj_out"]
    with pytest.raises(ValueError, match="no module"):
        m.add_lora(["attn.to_q"], "x", 4, 4.0, prefix="nowhere.")


def test_control_checkpoint_wire_formats(tmp_path):
    """the reference's `--transformer` formats (infer.py:124-140, src/hook.py:10-27) all reach load_state_dict."""
    from safetensors.torch import save_file
    from unigen_amd.checkpoint import load_control_checkpoint, read_control_state_dict
    m = _model()
    m.init_synthetic_(seed=5, std=0.05, bias_std=0.02)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ctrl = {k: v.float() for k, v in sd.items() if k.startswith(("control", "moe.", "shared_expert"))}       # fp32 on disk, like zero_to_fp32
    assert ctrl
    # 2. single torch.save file
    f = tmp_path / "pytorch_model_fp32.bin"
    torch.save(ctrl, str(f))
    assert set(read_control_state_dict(str(f))) == set(ctrl)
    # 1. ZeRO directory with a consolidated file; a raw one with a missing tag directory is an error (the merge: test_zero_shard_merge)
    z = tmp_path / "zero"; z.mkdir(); (z / "latest").write_text("global_step100")
    with pytest.raises(OSError, match="tag directory"):
        read_control_state_dict(str(z))
    torch.save(ctrl, str(z / "pytorch_model_fp32.bin"))
    assert set(read_control_state_dict(str(z))) == set(ctrl)
    # 3. safetensors shards
    s = tmp_path / "st"; s.mkdir()
    keys = sorted(ctrl)
    save_file({k: ctrl[k].contiguous() for k in keys[::2]}, str(s / "a.safetensors"))
    save_file({k: ctrl[k].contiguous() for k in keys[1::2]}, str(s / "b.safetensors"))
    assert set(read_control_state_dict(str(s))) == set(ctrl)
    # 4. hook files: one partial dict per module family; overlapping files are an error
    h = tmp_path / "hook"; h.mkdir()
    fam = {}
    for k in keys:
        fam.setdefault(k.split(".")[0], {})[k] = ctrl[k]
    for name, part in fam.items():
        torch.save(part, str(h / f"{name}_weights_0.bin"))
    assert set(read_control_state_dict(str(h))) == set(ctrl)
    torch.save(next(iter(fam.values())), str(h / "zz_weights_1.bin"))
    with pytest.raises(ValueError, match="already defined"):
        read_control_state_dict(str(h))
    # loading casts to bf16 and writes through the packed views
    m2 = _model()
    res = load_control_checkpoint(m2, str(s))
    assert not res.unexpected_keys and all(not k.startswith(("control", "moe.", "shared_expert")) for k in res.missing_keys)
    got = m2.state_dict()
    assert all(torch.equal(got[k], ctrl[k].to(got[k].dtype)) for k in ctrl)
    with pytest.raises(OSError):
        read_control_state_dict(str(tmp_path / "nope"))


class _FakeLossScaler:          # a non-torch object pickled beside the tensors, as DeepSpeed's shards carry
    def __init__(self):
        self.cur_scale = 65536.0


def _write_zero_checkpoint(root, tag, params, frozen, buffers, world, stage, ngroups=2):
    """Restates the SAVE side of deepspeed 0.16.5 (stage3.py / stage_1_and_2.py + engine._save_zero_checkpoint): trainable fp32 master
    weights flattened per param group and partitioned over ranks (stage 3: every parameter padded to a multiple of world and split
    rank-major; stages 1/2: the group's flat buffer padded to 2*world alignment and split evenly), frozen params as per-rank fragments."""
    import collections
    d = root / tag
    d.mkdir(parents=True)
    (root / "latest").write_text(tag)
    names = list(params)
    groups = [names[i::ngroups] for i in range(ngroups)]
    shapes = [collections.OrderedDict((n, params[n].shape) for n in g) for g in groups]
    for r in range(world):
        if stage == 3:
            flat_groups = []
            for g in groups:
                parts = []
                for n in g:
                    t = params[n].reshape(-1).float()
                    part = -(-t.numel() // world)
                    t = torch.cat([t, t.new_zeros(part * world - t.numel())])
                    parts.append(t[r * part:(r + 1) * part])
                flat_groups.append(torch.cat(parts))
            osd = dict(zero_stage=3, partition_count=world, fp32_flat_groups=flat_groups, loss_scaler=_FakeLossScaler())
            frag = {}
            for n, v in frozen.items():
                t = v.reshape(-1)
                part = -(-t.numel() // world)
                t = torch.cat([t, t.new_zeros(part * world - t.numel())])
                frag[n] = t[r * part:(r + 1) * part].clone()
            msd = dict(module={**buffers}, buffer_names=list(buffers), param_shapes=shapes, shared_params=[["alias.weight", names[0]]],
                       frozen_param_shapes=collections.OrderedDict((n, v.shape) for n, v in frozen.items()), frozen_param_fragments=frag,
                       ds_config=_FakeLossScaler(), ds_version="0.16.5")
            torch.save(msd, str(d / f"zero_pp_rank_{r}_mp_rank_00_model_states.pt"))
        else:
            parts = []
            for g in groups:
                flat = torch.cat([params[n].reshape(-1).float() for n in g])
                align = 2 * world
                flat = torch.cat([flat, flat.new_zeros(-(-flat.numel() // align) * align - flat.numel())])
                per = flat.numel() // world
                parts.append(flat[r * per:(r + 1) * per].clone())
            osd = dict(zero_stage=stage, partition_count=[world] * ngroups, single_partition_of_fp32_groups=parts, loss_scaler=_FakeLossScaler())
            if r == 0:
                msd = dict(module={**buffers}, buffer_names=list(buffers), param_shapes=shapes, shared_params=[["alias.weight", names[0]]],
                           frozen_param_shapes=collections.OrderedDict((n, v.shape) for n, v in frozen.items()),
                           frozen_param_fragments={n: v.clone() for n, v in frozen.items()}, ds_version="0.16.5")
                torch.save(msd, str(d / "mp_rank_00_model_states.pt"))
        torch.save(dict(optimizer_state_dict=osd), str(d / f"bf16_zero_pp_rank_{r}_mp_rank_00_optim_states.pt"))


@pytest.mark.parametrize("stage,world", [(3, 4), (3, 3), (2, 4), (1, 2)])
def test_zero_shard_merge(tmp_path, stage, world):
    """infer.py:124-128 `get_fp32_state_dict_from_zero_checkpoint`: the per-rank ZeRO shards merge back to the full fp32 state dict
    (odd sizes exercise the padding; a pickled non-torch object exercises the stub unpickler; no deepspeed import)."""
    from unigen_amd.checkpoint import load_control_checkpoint, merge_zero_checkpoint, read_control_state_dict
    m = _model()
    m.init_synthetic_(seed=9, std=0.05, bias_std=0.02)
    sd = {k: v.detach().float().clone() for k, v in m.state_dict().items()}
    ctrl = {k: v for k, v in sd.items() if k.startswith(("control", "moe.", "shared_expert"))}
    ctrl["odd.weight"] = torch.randn(7, 5)                                                    # numel 35: not a multiple of any world size
    frozen = {"x_embedder.weight": sd["x_embedder.weight"], "frozen.odd": torch.randn(11)}
    buffers = {"some.buffer": torch.arange(6, dtype=torch.bfloat16)}
    _write_zero_checkpoint(tmp_path, "global_step7", ctrl, frozen, buffers, world, stage)
    got = merge_zero_checkpoint(str(tmp_path))
    assert set(got) == set(ctrl) | set(frozen) | set(buffers) | {"alias.weight"}
    for k, v in {**ctrl, **frozen}.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k], v), k
    assert torch.equal(got["alias.weight"], ctrl[next(iter(ctrl))]) and torch.equal(got["some.buffer"], buffers["some.buffer"].float())
    assert "deepspeed" not in sys.modules
    # the reference's resolution order picks the directory up through its `latest` file, and the model loads it
    assert set(read_control_state_dict(str(tmp_path))) == set(got)
    m2 = _model()
    res = load_control_checkpoint(m2, str(tmp_path))
    assert set(res.unexpected_keys) == {"odd.weight", "frozen.odd", "some.buffer", "alias.weight"}
    g2 = m2.state_dict()
    assert all(torch.equal(g2[k], ctrl[k].to(g2[k].dtype)) for k in ctrl if k in g2)


class _EvalPayload:
    """A shard entry whose __reduce__ names builtins.eval / os.system: what an attacker-written `*_optim_states.pt` would carry."""
    def __init__(self, fn, arg):
        self.fn, self.arg = fn, arg

    def __reduce__(self):
        return (self.fn, (self.arg,))


@pytest.mark.parametrize("protocol", [2, 4])
def test_zero_unpickler_runs_no_payload(tmp_path, protocol):
    """the ZeRO shard reader resolves an exact allowlist of globals; `builtins.eval`, `os.system`, `torch.hub.load` and
    the like become inert stubs, so a crafted shard executes nothing - while real tensors, containers and dtypes still load."""
    import builtins, os as _os
    from unigen_amd.checkpoint import _zero_load, merge_zero_checkpoint, _Stub
    marker = tmp_path / "pwned"
    code = f"open({str(marker)!r}, 'w').write('x')"
    shard = dict(optimizer_state_dict=dict(zero_stage=2, partition_count=1, single_partition_of_fp32_groups=[torch.arange(6.0)],
                                           evil1=_EvalPayload(builtins.eval, code), evil2=_EvalPayload(_os.system, f"touch {marker}"),
                                           evil3=_EvalPayload(builtins.exec, code), evil4=_EvalPayload(getattr(builtins, "__import__"), "antigravity"),
                                           scaler=_FakeLossScaler(), dt=torch.bfloat16, sz=torch.Size([2, 3]), half=torch.ones(3, dtype=torch.bfloat16)))
    f = tmp_path / "mp_rank_00_optim_states.pt"
    torch.save(shard, str(f), pickle_protocol=protocol)
    got = _zero_load(str(f))["optimizer_state_dict"]
    assert not marker.exists()
    assert all(isinstance(got[k], _Stub) for k in ("evil1", "evil2", "evil3", "evil4", "scaler"))
    assert got["dt"] is torch.bfloat16 and got["sz"] == torch.Size([2, 3]) and torch.equal(got["half"], torch.ones(3, dtype=torch.bfloat16))
    assert torch.equal(got["single_partition_of_fp32_groups"][0], torch.arange(6.0))
    # a directory whose shards lack the ZeRO entries is a clear error, not a KeyError
    d = tmp_path / "ck"; (d / "t").mkdir(parents=True); (d / "latest").write_text("t")
    torch.save(dict(optimizer_state_dict=dict(partition_count=1)), str(d / "t" / "mp_rank_00_optim_states.pt"))
    with pytest.raises(ValueError, match="zero_stage"):
        merge_zero_checkpoint(str(d))
    # a field the merge arithmetic needs that resolved to a stub (here partition_count stored as a numpy scalar: numpy's reconstructor is
    # not allow-listed) fails with the blocked global's name, not with a later `int(_Stub)` TypeError
    import numpy as np
    torch.save(dict(optimizer_state_dict=dict(zero_stage=2, partition_count=np.int64(1), single_partition_of_fp32_groups=[torch.arange(6.0)])),
               str(d / "t" / "mp_rank_00_optim_states.pt"))
    with pytest.raises(ValueError, match=r"partition_count.*numpy"):
        merge_zero_checkpoint(str(d))


@pytest.mark.parametrize("cls", ["UniGenFlux", "UniGenSD3"])
def test_control_modules_start_from_the_reference_initial_values(cls):
    """src/UniGenTransformer.py:727-773, 833-842 (Flux) / :26-128 (SD3): deep copies of the base embedders, torch default nn.Linear init for the
    control blocks / gate / experts (every expert a copy of ONE module), RMSNorm weights = 1, zeros ONLY for the zero-res projections."""
    torch.manual_seed(0)
    if cls == "UniGenFlux":
        m = _model()
        sd = m.state_dict()
        for dst, src in (("control_time_text_embed.", "time_text_embed."), ("control_condition_embed.", "time_text_embed."), ("control_x_embedder.", "x_embedder.")):
            keys = [k for k in sd if k.startswith(dst)]
            assert keys and all(torch.equal(sd[k], sd[src + k[len(dst):]]) for k in keys), dst
        zero = ("controlnet_add_joint_blocks.", "controlnet_add_single_blocks.")
        fresh = ("control_context_embedder.", "control_joint_trans_blocks.", "control_single_trans_blocks.", "shared_expert.", "moe.")
    else:
        m = importlib.import_module("src.UniGenTransformer").UniGenSD3.from_config(dict(sample_size=16, num_layers=2, attention_head_dim=64, num_attention_heads=2,
                joint_attention_dim=64, caption_projection_dim=128, pooled_projection_dim=64, pos_embed_max_size=12, dual_attention_layers=(0,)))
        m.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True))
        sd = m.state_dict()
        zero = ("controlnet_add_blocks.",)
        fresh = ("control_pos_embed_input.proj", "control_time_text_embed.", "control_condition_embed.", "control_context_embedder.",
                 "control_transformer_blocks.", "shared_expert.", "moe.")
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
    for k, v in sd.items():
        if k.startswith(zero):
            assert float(v.abs().max()) == 0.0, k
        elif k.startswith(fresh):
            if k.endswith(".weight") and v.dim() == 1:
                assert torch.equal(v, torch.ones_like(v)), k                       # RMSNorm
            elif k.endswith(".weight"):
                bound = 1.0 / v[0].numel() ** 0.5                                   # kaiming_uniform_(a = sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                vf = v.float()
                assert float(vf.abs().max()) <= bound * 1.01 and float(vf.std()) > 0.4 * bound, (k, bound, float(vf.std()))
    # deepspeed Experts: num_experts deep copies of one module -> identical experts, but a non-degenerate (untied) gate
    pe = "moe.moe_layer.experts.deepspeed_experts."
    e0 = {k[len(pe) + 2:]: v for k, v in sd.items() if k.startswith(pe + "0.")}
    n_e = sd["moe.moe_layer.gate.wg.weight"].shape[0]
    assert n_e == 6 and all(torch.equal(sd[f"{pe}{e}.{r}"], v) for e in range(1, n_e) for r, v in e0.items())
    wg = sd["moe.moe_layer.gate.wg.weight"].float()
    assert float((wg[0] - wg[1]).abs().max()) > 0
    assert all(p.requires_grad is False for p in m.parameters())


def _run_bench(args, env_extra=None, timeout=180):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=root)


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` with NO launcher must work (the driver's N = 1 form; reference script/infer.sh:49-67 starts
    one process per GPU). The parent spawns one fresh child per rank before anything touches a GPU; here the harness is rehearsed on the
    CPU (gloo, --dry-run: no GPU work, value null): rendezvous, barriers, max over ranks, exactly one JSON line from rank 0."""
    import json
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dry_run"] is True and d["value"] is None and d["steps"] == 2 and d["scaling"] == "weak"
    assert d["ms_per_step"] >= 19.0                       # MAX over ranks: rank 1 sleeps 20 ms per step, rank 0 only 10
    # the all_gather of per-rank (images, seconds, device) makes the straggler visible in the one line
    pr = d["per_rank"]
    assert [x["rank"] for x in pr] == [0, 1] and all(x["images"] == 2 for x in pr)
    assert pr[1]["seconds"] > 1.5 * pr[0]["seconds"] and pr[0]["seconds"] >= 0.019
    assert "torch.cuda.device_count() = 0" in r.stderr


def test_bench_refuses_more_ranks_than_gpus():
    """Without --dry-run the launcher prints the device count and fails clearly when the node has fewer GPUs than ranks (never fabricates)."""
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "shows only 0 GPU(s)" in (r.stderr + r.stdout)
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    # a torchrun-style environment whose world size disagrees with --gpus is an error too
    r = _run_bench(["--gpus", "2", "--dry-run"], env_extra=dict(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)
    r = _run_bench(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


def test_bench_dump_output_is_float32_capped_and_reproducible(tmp_path):
    """--dump-outputs writes float32 .npy files; an output above the element cap becomes a seeded sample that is the same on every run."""
    import numpy as np
    import bench
    t = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    assert not bench.dump_output(str(tmp_path / "full.npy"), t, 1000)
    full = np.load(tmp_path / "full.npy")
    assert full.dtype == np.float32 and full.shape == (3, 5, 7) and np.array_equal(full, t.float().numpy())
    assert bench.dump_output(str(tmp_path / "s1.npy"), t, 50) and bench.dump_output(str(tmp_path / "s2.npy"), t, 50)
    s1, s2 = np.load(tmp_path / "s1.npy"), np.load(tmp_path / "s2.npy")
    assert s1.dtype == np.float32 and s1.shape == (50,) and np.array_equal(s1, s2) and np.isin(s1, full).all()


def test_bench_measures_beyond_the_headline_only_with_full(monkeypatch):
    """A plain run makes no measurement after its timed steps; --full makes every one the run's shape allows, and each --no-* option
    leaves its own out."""
    import bench
    monkeypatch.setattr(bench, "_under_profiler", lambda: False)

    def extra(argv, world=1):
        args = bench.parser().parse_args(argv)
        config = args.config or ("cfg2" if world == 1 else "cfg4")
        args.batch = args.batch or (4 if config == "cfg2" else 8)
        return bench.extra_blocks(args, world, config)

    everything = {"probe", "scaling_base", "cpu_baseline", "small_m", "other_configs", "pmc"}
    for argv in ([], ["--steps", "5", "--warmup", "2"], ["--config", "cfg3"], ["--graph"], ["--dump-outputs", "d"]):
        assert extra(argv) == set(), argv
    assert extra([], world=2) == set()
    assert extra(["--full"]) == everything
    assert extra(["--full", "--no-cpu-baseline", "--no-other-configs", "--no-scaling-base"]) == {"probe", "pmc"}
    assert extra(["--full", "--no-pmc"]) == everything - {"pmc"}
    assert extra(["--full", "--no-kernel-timer"]) == {"scaling_base", "cpu_baseline"}
    assert extra(["--full", "--graph"]) == {"cpu_baseline"}
    assert extra(["--full", "--batch", "8"]) == extra(["--full", "--small"]) == {"probe", "cpu_baseline"}
    assert extra(["--full", "--config", "cfg5"]) == {"probe", "cpu_baseline"}
    assert extra(["--full"], world=2) == {"probe"}
    monkeypatch.setattr(bench, "_under_profiler", lambda: True)          # under a profiler the counter passes stay out
    assert extra(["--full"]) == everything - {"pmc"}


def test_consis_module_parameters_follow_the_reference():
    """use_consis_module (src/UniGenTransformer.py:893-923): two joint blocks `consis_module.{0,1}` under the reference's key names, trainable,
    default-initialised; the oracle's state shapes agree; with the flag off (every shipped configuration) nothing is registered."""
    from oracle import unigen_ref as R
    on, off = _model(use_consis_module=True), _model()
    ks_on, ks_off = set(on.state_dict()), set(off.state_dict())
    extra = ks_on - ks_off
    assert extra and all(k.startswith("consis_module.") for k in extra) and not any(k.startswith("consis_module.") for k in ks_off)
    assert {k.split(".")[1] for k in extra} == {"0", "1"} and "consis_module.0.attn.to_add_out.weight" in extra
    assert ks_on == set(R.state_shapes(R.FluxConfig(condition_nums=1, use_consis_module=True, **TINY)))
    assert "consis_module" in on.trainable_control_modules and "consis_module" not in off.trainable_control_modules
    w = on.state_dict()["consis_module.0.attn.to_q.weight"].float()
    assert float(w.std()) > 0 and torch.equal(on.state_dict()["consis_module.1.attn.norm_q.weight"], torch.ones(TINY["attention_head_dim"], dtype=w.dtype if False else on.state_dict()["consis_module.1.attn.norm_q.weight"].dtype))


# ----------------------------------------------------------------------------------------------------------------------
# first contact on a clean clone with N ranks: one build, serialised, outputs appear atomically
# ----------------------------------------------------------------------------------------------------------------------

_FAKE_HIPCC = r"""#!/usr/bin/env python3
# stands for hipcc in the race tests: logs the call, takes a while, then writes its -o target in two halves (a reader in between would see a torn file)
import os, sys, time
out = sys.argv[sys.argv.index("-o") + 1]
with open(os.environ["FAKE_HIPCC_LOG"], "a") as f:
    f.write(f"{os.getpid()} {time.time():.3f} start {'link' if '-shared' in sys.argv else 'cc'} {os.path.basename(out)}\n")
with open(out, "w") as f:
    f.write("first half;")
    f.flush()
    time.sleep(0.15)
    f.write("second half")
with open(os.environ["FAKE_HIPCC_LOG"], "a") as f:
    f.write(f"{os.getpid()} {time.time():.3f} end {os.path.basename(out)}\n")
"""


def _clean_clone(tmp_path):
    """A copy of the tree as a clean clone has it (sources, no *.o / *.so) with a stand-in hipcc."""
    import shutil
    root = tmp_path / "clone"
    shutil.copytree(os.path.join(ROOT, "unigen_amd"), root / "unigen_amd", ignore=shutil.ignore_patterns("*.o", "*.so", "__pycache__", ".build.lock", "*.tmp*"))
    shutil.copytree(os.path.join(ROOT, "include"), root / "include")
    shutil.copy(os.path.join(ROOT, "bench.py"), root / "bench.py")
    fake = tmp_path / "fake_hipcc"
    fake.write_text(_FAKE_HIPCC)
    fake.chmod(0o755)
    log = tmp_path / "hipcc.log"
    log.write_text("")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "UG_LIB_PATH")}
    env.update(HIPCC=str(fake), FAKE_HIPCC_LOG=str(log))
    return root, log, env


def test_concurrent_builds_are_serialised_and_atomic(tmp_path):
    """Four processes call unigen_amd.build.build() at once on a clean clone (what every rank's lib.load() does): exactly ONE of them compiles
    (the others wait on the lock, then find fresh outputs), and a watcher polling the final .so path never sees a partially written file."""
    root, log, env = _clean_clone(tmp_path)
    so = root / "unigen_amd" / "libunigen_hip.so"
    code = f"import sys; sys.path.insert(0, {str(root)!r}); from unigen_amd import build; print(build.build())"
    procs = [subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(4)]
    torn = 0
    while any(p.poll() is None for p in procs):
        if so.exists() and so.read_text() != "first half;second half":
            torn += 1
    outs = [p.communicate(timeout=60) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all(o[0].strip() == str(so) for o in outs)
    assert torn == 0 and so.read_text() == "first half;second half"
    from unigen_amd import build as B
    calls = [ln.split() for ln in log.read_text().splitlines() if " start " in ln]
    assert len(calls) == len(B.SOURCES) + 1, calls                     # every source once + one link: no second build
    assert [c for c in calls if c[3] == "link"][0] == calls[-1]         # the link after every object
    assert not [f for f in os.listdir(root / "unigen_amd" / "csrc") if ".tmp" in f] and not [f for f in os.listdir(root / "unigen_amd") if ".tmp" in f]


def test_bench_parent_builds_before_it_spawns_ranks(tmp_path):
    """`python bench.py --gpus 2` on a clean clone: the parent builds the library (hipcc only, it never touches the GPU) BEFORE the ranks exist,
    so they never race in lib.load(); rehearsed with --dry-run over gloo."""
    root, log, env = _clean_clone(tmp_path)
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-run"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=str(root))
    assert r.returncode == 0, r.stderr[-2000:]
    assert (root / "unigen_amd" / "libunigen_hip.so").exists()
    err = r.stderr
    assert "libunigen_hip.so ready" in err
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    # the communicator as torch.distributed reports it on rank 0
    assert d["dist"] == dict(initialized=True, backend="gloo", world_size=2, rank=0, note="backend nccl = RCCL on ROCm")
    pids = {ln.split()[0] for ln in log.read_text().splitlines()}
    from unigen_amd import build as B
    assert len([ln for ln in log.read_text().splitlines() if " start " in ln]) == len(B.SOURCES) + 1 and len(pids) == len(B.SOURCES) + 1


def test_alternating_pack_groupings_keep_the_weight_bytes_constant():
    """a three-way q|k|v pack after the four-way [q|k|v|proj_mlp] pack of the same block must not leave proj_mlp pointing into the old
    buffer (that keeps the whole old storage alive beside the new copy): the storage the parameters hold stays the size of the parameters."""
    cls = importlib.import_module("src.UniGenTransformer").UniGenFlux
    model = cls.from_config(dict(TINY), device="cpu", dtype=torch.bfloat16)
    p = "single_transformer_blocks.0"

    def held_bytes():
        seen = {}
        for q in model.parameters():
            st = q.data.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
        return sum(seen.values())

    want = sum(q.numel() * q.element_size() for q in model.parameters())
    before = {n: q.detach().clone() for n, q in model.named_parameters() if n.startswith(p)}
    assert model._single_qkv_mlp(p) is not None and held_bytes() == want
    for _ in range(3):
        model._attn_qkv(p + ".attn")
        assert held_bytes() == want, (held_bytes(), want)
        model._single_qkv_mlp(p)
        assert held_bytes() == want, (held_bytes(), want)
    assert all(torch.equal(before[n], q) for n, q in model.named_parameters() if n.startswith(p))
    assert len([k for k in model._packed if k.startswith(p)]) <= 4


_FAKE_ROCPROFV3 = r"""#!/usr/bin/env python3
# stands for rocprofv3 in the same-run traffic test: checks the command shape bench.py builds and writes the counter CSV a real pass would
import os, sys
a = sys.argv[1:]
assert "--kernel-trace" in a and "--output-format" in a and a[a.index("--output-format") + 1] == "csv", a
sep = a.index("--")
prog = a[sep + 1:]
assert os.path.basename(prog[0]).startswith("python") and prog[1].endswith("bench.py") and prog[2:] == ["--pmc-child"], prog      # the program itself after `--`
counters = a[a.index("--pmc") + 1:a.index("--output-format")]
if os.environ.get("FAKE_PMC_FAIL") == counters[0]:
    sys.exit(3)
out = os.path.join(a[a.index("-d") + 1], "host"); os.makedirs(out)
rows = ["Kernel_Name,Counter_Name,Counter_Value,Start_Timestamp,End_Timestamp"]
val = dict(FETCH_SIZE=1000.0, WRITE_SIZE=300.0, SQ_VALU_MFMA_BUSY_CYCLES=700.0 * 1024, GRBM_GUI_ACTIVE=8 * 1000.0)
for i in range(12):        # two identical steps of 6 launches; the FIRST (cold: packing, allocation, cold caches) reads 3 x the bytes and must not be counted
    name = ["void (anonymous namespace)::gemm256_kernel<2, false, 128, false>(ug_gemm_desc)", "void (anonymous namespace)::gemm128_kernel<2>(ug_gemm_desc)",
            "void (anonymous namespace)::flash_attn_kernel<128>(x)"][i % 3]
    for c in counters:
        rows.append(f'"{name}",{c},{val[c] * (3 if i < 6 and c.endswith("SIZE") else 1)},{1000 * i},{1000 * i + 500}')
rows[1:] = rows[1:][::-1]      # file order is not dispatch order
open(os.path.join(out, "1_counter_collection.csv"), "w").write("\n".join(rows) + "\n")
"""


def test_same_run_traffic_reads_its_own_counter_passes(tmp_path, monkeypatch):
    """bench.same_run_traffic(): one rocprofv3 child per counter pass with the program straight after `--`, bytes per GEMM launch =
    (2 x FETCH_SIZE + WRITE_SIZE) x 1024 over gemm256 + gemm128 launches only, matrix-pipe busy of gemm256 alone; a failing pass raises (bench.py then
    keeps the recorded profile and says so). The child runs the step twice and only the second, warm step's launches are counted."""
    import bench
    fake = tmp_path / "rocprofv3"
    fake.write_text(_FAKE_ROCPROFV3)
    fake.chmod(0o755)
    monkeypatch.setenv("PATH", f"{tmp_path}:{os.environ['PATH']}")
    r = bench.same_run_traffic(limit_s=30)
    assert r["launches"] == 4                                             # 2 x gemm256 + 2 x gemm128 of the 6 kernels of the fake trace's SECOND (warm) step
    assert r["fetch_bytes_per_launch_corrected"] == 2 * 1000.0 * 1024 and r["write_bytes_per_launch"] == 300.0 * 1024
    assert r["traffic"] == (2 * 1000.0 + 300.0) * 1024
    assert abs(r["gemm256"]["mfma_busy"] - 0.7) < 1e-12 and r["gemm256"]["launches"] == 2 and abs(r["gemm256"]["effective_clock_ghz"] - 2.0) < 1e-12
    blocks = bench._roofline_blocks(dict(gemm=dict(flops=1e15, ms=1000.0, launches=4)), 1.0, 2000.0, 1900.0, "attn", None, r)
    assert blocks["roofline"]["traffic"] == r["traffic"] and blocks["roofline"]["traffic_source"]["measured_in_this_run"] is True
    assert blocks["roofline"]["pmc_gemm256"]["measured_in_this_run"] is True
    assert r["attn"]["launches"] == 2 and r["attn"]["traffic"] == (2 * 1000.0 + 300.0) * 1024 and abs(r["attn"]["mfma_busy"] - 0.7) < 1e-12
    both = bench._roofline_blocks(dict(gemm=dict(flops=1e15, ms=1000.0, launches=4), attn=dict(flops=1e14, ms=200.0, launches=2)), 1.0, 2000.0, 1900.0, "attn", None, r)
    assert both["roofline_attention"]["traffic"] == r["attn"]["traffic"] and both["roofline_attention"]["pmc_attn"]["measured_in_this_run"] is True
    monkeypatch.setenv("FAKE_PMC_FAIL", "WRITE_SIZE")
    with pytest.raises(RuntimeError, match="WRITE_SIZE"):
        bench.same_run_traffic(limit_s=30)


def test_fullsize_children_are_scheduled_beside_the_suite():
    """tests/conftest.py: the four full-size oracle comparisons are started as background children when collection ends and their tests run last
    (VERDICT r5 item 4). Without a GPU nothing is started; the mapping from test ids to child commands and the reordering are checked here."""
    import conftest as CT
    assert CT.CHILD_THREADS + CT.SUITE_THREADS == 16
    for key, cmd in CT.FULLSIZE_JOBS.items():
        assert os.path.exists(os.path.join(ROOT, cmd[0])), cmd
        assert CT._job_key("tests/test_fullsize_gpu.py::" + key) == key
    assert CT._job_key("tests/test_fullsize_gpu.py::test_cfg3_three_conditions_b8_whole_forward_properties") is None
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests"), "-q", "-m", "gpu", "--collect-only"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    ids = [l for l in r.stdout.splitlines() if "::" in l]
    tail = ids[-4:]
    assert [CT._job_key(i) for i in tail] == list(CT.FULLSIZE_JOBS), tail
    assert not any(CT._job_key(i) for i in ids[:-4])
