"""tests/depth_ref.py (the plain-torch restatement of Depth Anything that the GPU tests use as their truth) against transformers' own modules and
against tests/golden/depth_tiny.safetensors, and the host side of unigen_amd/depth.py: sizes, resampling tables, state-dict keys, config refusals,
from_pretrained. No GPU."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_tiny.safetensors")


@pytest.fixture(scope="module")
def gold():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


@pytest.fixture(scope="module")
def sd(gold):
    s = R.random_state(R.TINY)
    assert torch.equal(R.fingerprint(s), gold["w.fingerprint"]), "depth_ref.random_state no longer draws the weights the fixture was made with"
    return s


@pytest.fixture(scope="module")
def truth(sd):
    return {name: R.forward(sd, R.TINY, R.pixel_values(R.case_images(name))) for name in R.CASES}


def _gen():
    pytest.importorskip("transformers", reason="transformers is the oracle of this test")
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(ROOT, "tests", "golden", "make_depth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", list(R.CASES))
def test_depth_ref_matches_the_stored_float64_run(gold, truth, name):
    stored = [k[len(name) + 1:] for k in gold if k.startswith(name + ".") and not k.endswith(".err")]
    assert "predicted_depth" in stored and "embeddings" in stored and len(stored) >= 6
    got = dict(R.stage_list(truth[name]))
    for k in stored:
        assert got[k].shape == gold[f"{name}.{k}"].shape, k
        assert R.rel_l2(got[k], gold[f"{name}.{k}"]) < 2e-7, (k, R.rel_l2(got[k], gold[f"{name}.{k}"]))       # the file holds fp32: 2^-24 per element
    err = gold[name + ".err"]
    assert err.shape == (14, 2) and (err[:, 0] > 0).all() and (err[:, 0] < 1e-5).all() and (err[:, 1] > 1e-3).all() and (err[:, 1] < 5e-2).all()
    d = truth[name]["predicted_depth"]
    assert 0.3 <= float((d > 0).double().mean()) <= 0.98 and float(d.max() - d.min()) > 1


def test_depth_ref_matches_transformers_modules(sd, truth):
    G = _gen()
    m = G.hf_model(R.TINY, sd).double()
    for name in R.CASES:
        want = R.stage_list(G.hf_stages(m, R.pixel_values(R.case_images(name))))
        for (k, a), (_, b) in zip(R.stage_list(truth[name]), want):
            assert a.shape == b.shape and R.rel_l2(a, b) < 1e-9, (name, k, R.rel_l2(a, b))


def test_bf16_switch_lands_at_transformers_own_bf16_error(gold, sd, truth):
    """The rounding points of depth_ref (and of the HIP path): with them switched on, the error against float64 is that of transformers' bf16 run."""
    for name in R.CASES:
        got = R.forward(sd, R.TINY, R.pixel_values(R.case_images(name)), dtype=torch.float32, round_bf16=True)
        e = R.rel_l2(got["predicted_depth"], truth[name]["predicted_depth"])
        assert 0.3 * float(gold[name + ".err"][-1, 1]) < e < 3 * float(gold[name + ".err"][-1, 1]), (name, e)


def test_every_state_dict_key_is_consumed_and_nothing_else_expected(sd):
    from unigen_amd.depth import DepthAnythingForDepthEstimation
    m = DepthAnythingForDepthEstimation(R.TINY)
    exp = m.expected_keys()
    assert set(exp) | {"backbone.embeddings.mask_token"} == set(sd)
    assert all(tuple(sd[k].shape) == exp[k] for k in exp)
    assert m.load_state_dict(sd) == ([], [])
    with pytest.raises(KeyError):
        m.load_state_dict({**sd, "head.conv4.weight": torch.zeros(1)})
    with pytest.raises(KeyError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "neck.convs.2.weight"})
    with pytest.raises(ValueError):
        m.load_state_dict({**sd, "head.conv3.bias": torch.zeros(2)})
    try:
        G = _gen()
    except pytest.skip.Exception:
        return
    assert set(G.hf_model(R.TINY, sd).state_dict()) == set(sd)


def test_load_time_packing(sd):
    from unigen_amd.depth import DepthAnythingForDepthEstimation
    m = DepthAnythingForDepthEstimation(R.TINY, dtype=torch.float32)
    m.load_state_dict(sd)
    p = m._p
    assert p["patch_w"].shape == (128, 640) and (p["patch_w"][:, 588:] == 0).all()
    assert p["l0.qkv_w"].shape == (384, 128) and torch.equal(p["l0.qkv_w"][128:256], sd["backbone.encoder.layer.0.attention.attention.key.weight"].float())
    assert p["n0.proj_w"].shape == (64, 128) and (p["n0.proj_w"][24:] == 0).all() and (p["n0.proj_b"][24:] == 0).all()
    w = sd["neck.reassemble_stage.layers.0.resize.weight"].float()                       # [Cin][Cout][ky][kx]
    assert p["n0.up_w"].shape == (16 * 24, 64) and p["n0.up_w"][(2 * 4 + 3) * 24 + 5, 7] == w[7, 5, 2, 3] and (p["n0.up_w"][:, 24:] == 0).all()
    assert p["n3.down_w"].shape == (128, 3, 3, 128) and p["n1.conv_w"].shape == (64, 3, 3, 64) and (p["n1.conv_w"][..., 48:] == 0).all()
    assert p["h.c1_w"].shape == (64, 3, 3, 64) and (p["h.c1_w"][32:] == 0).all() and p["h.c2_w"].shape == (32, 3, 3, 64) and (p["h.c2_w"][..., 32:] == 0).all()
    pos, cls = m.position_table(5, 7)
    want = R.forward(sd, R.TINY, torch.zeros(1, 3, 70, 98), dtype=torch.float32)          # embeddings of a zero image: bias + positions
    assert pos.shape == (35, 128) and cls.shape == (1, 128)
    b = sd["backbone.embeddings.patch_embeddings.projection.bias"].float()
    assert torch.allclose(want["embeddings"][0, 1:] - b, pos, atol=1e-6) and torch.allclose(want["embeddings"][0, :1], cls, atol=1e-6)
    assert m.position_table(5, 7)[0] is pos and m.position_table(5, 5)[0].shape == (25, 128)


def test_from_pretrained_round_trips(tmp_path, sd):
    from safetensors.torch import save_file
    from unigen_amd.depth import DepthAnythingConfig, DepthAnythingForDepthEstimation
    with open(tmp_path / "config.json", "w") as f:
        json.dump(R.TINY, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m = DepthAnythingForDepthEstimation.from_pretrained(tmp_path, dtype=torch.float32)
    assert m.config.hidden_size == 128 and m.config.out_indices == [1, 2, 3, 4] and m.config.neck_hidden_sizes == (24, 48, 96, 128)
    got = m.state_dict()
    assert set(got) == set(sd) - {"backbone.embeddings.mask_token"} and all(torch.equal(got[k], sd[k].float()) for k in got)
    again = DepthAnythingConfig(m.config.to_dict())
    assert again.to_dict() == m.config.to_dict()
    with pytest.raises(OSError):
        DepthAnythingForDepthEstimation.from_pretrained("LiheYoung/depth-anything-small-hf")


def test_config_defaults_and_refusals():
    from unigen_amd.depth import DepthAnythingConfig
    c = DepthAnythingConfig()
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.mlp_ratio, c.patch_size) == (384, 12, 6, 4, 14)
    assert c.out_indices == [9, 10, 11, 12] and c.neck_hidden_sizes == (48, 96, 192, 384) and c.fusion_hidden_size == 64 and c.head_hidden_size == 32
    assert DepthAnythingConfig(R.SMALL).to_dict() == c.to_dict()
    assert DepthAnythingConfig(dict(backbone_config=dict(out_features=["stage9", "stage10", "stage11", "stage12"]))).out_indices == [9, 10, 11, 12]
    bb = R.TINY["backbone_config"]
    with pytest.raises(NotImplementedError, match="use_swiglu_ffn"):
        DepthAnythingConfig({**R.TINY, "backbone_config": {**bb, "use_swiglu_ffn": True}})
    with pytest.raises(NotImplementedError, match="reshape_hidden_states"):
        DepthAnythingConfig({**R.TINY, "backbone_config": {**bb, "reshape_hidden_states": True}})
    with pytest.raises(NotImplementedError, match="num_attention_heads"):
        DepthAnythingConfig({**R.TINY, "backbone_config": {**bb, "num_attention_heads": 4}})
    assert DepthAnythingConfig({**R.TINY, "backbone_config": {**bb, "num_attention_heads": 1}}).num_attention_heads == 1          # head width 128
    with pytest.raises(ValueError, match="depth estimation type"):
        DepthAnythingConfig({**R.TINY, "depth_estimation_type": "absolute"})


SIZES = [(60, 100), (45, 33), (1024, 1024), (518, 518), (480, 640), (640, 480), (333, 500), (500, 333), (37, 37), (7, 7), (14, 14), (1, 1000), (1000, 30),
         (259, 259), (777, 518), (518, 777), (1036, 1554), (1554, 1036), (2072, 2220), (2220, 2072), (148, 37), (37, 148), (300, 301), (301, 300), (512, 768),
         (768, 512), (720, 1280), (1080, 1920), (1920, 1080), (2160, 3840), (100, 60), (33, 45), (64, 64), (99, 100), (518, 1000), (1000, 518), (21, 777),
         (400, 600), (600, 400), (1, 1), (2, 3), (123, 457), (457, 123), (518, 525), (525, 518), (74, 111), (111, 74)]


def test_output_size_is_get_resize_output_image_size():
    pytest.importorskip("transformers", reason="transformers is the oracle of this test")
    from transformers.models.dpt.image_processing_pil_dpt import get_resize_output_image_size
    from unigen_amd.depth import DepthImageProcessor
    halves = 0
    for size in (518, 56, (384, 512)):
        p = DepthImageProcessor(size=size)
        for keep in (True, False):
            p.keep_aspect_ratio = keep
            for H, W in SIZES:
                want = get_resize_output_image_size(np.zeros((3, H, W)), p.size, keep, 14)
                assert p.output_size(H, W) == (want.height, want.width), (size, keep, H, W)
                sh, sw = p.size[0] / H, p.size[1] / W
                if keep:
                    sh = sw = sw if abs(1 - sw) < abs(1 - sh) else sh
                halves += sum(abs((v / 14) % 1 - 0.5) < 1e-12 for v in (sh * H, sw * W))
    assert len(SIZES) >= 40 and halves >= 8, halves                                  # exact .5 multiples: Python's round goes to the even one
    assert DepthImageProcessor(size=518).output_size(1036, 1554) == (518, 784)     # 777 / 14 = 55.5 -> 56
    assert DepthImageProcessor(size=518).output_size(1024, 1024) == (518, 518)


def test_bicubic_tables_reproduce_pil_bytes(gold):
    from unigen_amd.image import resample_tables
    for tag in ("img0", "img1"):
        want = gold[tag + ".bicubic"].numpy()
        got = R.resize_pil_tables(gold[tag + ".u8"].numpy(), want.shape[0], want.shape[1], "bicubic")
        assert np.array_equal(got, want), tag
    assert gold["img0.bicubic"].shape[:2] == (56, 98) and gold["img1.bicubic"].shape[:2] == (56, 42)            # one image shrinks, one grows
    pil = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for (H, W), (h, w) in (((20, 30), (70, 98)), ((300, 200), (28, 42)), ((33, 33), (33, 14))):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_pil_tables(img, h, w), np.array(pil.fromarray(img).resize((w, h), pil.BICUBIC)))
    b, c, k = resample_tables(100, 98, "bicubic")
    assert k == 2 * int(np.ceil(2.0 * 100 / 98)) + 1 and resample_tables(100, 98)[2] == 2 * int(np.ceil(3.0 * 100 / 98)) + 1       # the default stays Lanczos
    with pytest.raises(NotImplementedError):
        resample_tables(10, 20, "nearest")


def test_processor_and_postprocess_restatements_match_the_stored_oracle(gold):
    for tag in ("img0", "img1"):
        assert torch.equal(R.pixel_values(gold[tag + ".bicubic"][None]), gold[tag + ".pixel_values"]), tag          # the rounding points, bit for bit
        H, W = gold[tag + ".u8"].shape[:2]
        up, u8 = R.postprocess(gold[tag + ".depth_in"], H, W)
        assert torch.equal(up, gold[tag + ".depth_up"]) and torch.equal(u8, gold[tag + ".depth_u8"])
        assert np.array_equal(R.minmax_u8(up.numpy()), u8.numpy())
        share, worst = gold[tag + ".share_fp32"].tolist()
        assert 0 < share <= 0.002 and worst == 1
    rows = R.patch_rows(gold["img1.pixel_values"], 14)
    assert rows.shape == (12, 640) and (rows[:, 588:] == 0).all() and rows[5, 2 * 196 + 3 * 14 + 9] == gold["img1.pixel_values"][0, 2, 14 + 3, 2 * 14 + 9]


def test_condition_depth_still_refuses_and_names_depth_image():
    from unigen_amd.condition import Condition, depth_image
    import src.condition
    with pytest.raises(NotImplementedError, match="depth-estimation") as e:
        Condition("depth", raw_img=np.zeros((8, 8, 3), np.uint8))
    assert "depth_image" in str(e.value)
    assert src.condition.depth_image is depth_image
    c = Condition("depth", raw_img=np.zeros((8, 8, 3), np.uint8), no_process=True)
    assert c.type_id == 0
    from unigen_amd.image import VaeImageProcessor
    with pytest.raises(NotImplementedError):
        VaeImageProcessor(resample="bicubic")


def test_new_entry_points_are_declared_and_built():
    from unigen_amd import build, lib, ops
    hdr = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    declared = set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", hdr))
    new = {"ug_img_u8_to_patches", "ug_relu", "ug_deconv_scatter_nhwc", "ug_bilinear_nhwc", "ug_depth_head_out", "ug_bicubic_f32", "ug_minmax_to_u8",
           "ug_minmax_workspace_bytes"}
    twins = {n + "_f32" for n in new if n not in ("ug_bicubic_f32", "ug_minmax_to_u8", "ug_minmax_workspace_bytes")}
    assert new | twins <= declared and new | twins <= set(lib.SIGNATURES) and "depth.hip" in build.SOURCES
    for n in twins:
        assert lib.SIGNATURES[n] == lib.SIGNATURES[n[:-4]] and lib._F32_TWINS[n] == n[:-4]
    assert all(callable(getattr(ops, f)) for f in ("img_u8_to_patches", "relu", "deconv_scatter_nhwc", "bilinear_nhwc", "depth_head_out", "bicubic_f32", "minmax_to_u8"))
    L = lib.load()
    assert int(L.ug_minmax_workspace_bytes(2, 1000)) == 2 * 64 * 8 and int(L.ug_minmax_workspace_bytes(0, 5)) == 0
