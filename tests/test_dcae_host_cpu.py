"""The host side of AutoencoderDC (unigen_amd/dcae.py) without a GPU: diffusers' keys, what the constructor refuses (each message names the
argument), and the load-time permutation of the attention weights against tests/dcae_ref.py."""
import pytest
import torch

from tests import dcae_ref as R
from unigen_amd.dcae import DCAE_CONFIG, DCAE_F32C32_SANA, AutoencoderDC


@pytest.mark.parametrize("name", ["a", "b"])
def test_keys_are_the_reference_modules_keys(name):
    ref = R.DCAERef(**R.TINY[name]).state_dict()
    exp = AutoencoderDC(R.TINY[name]).expected_keys()
    assert set(exp) == set(ref)
    for k, shape in exp.items():
        assert tuple(ref[k].shape) == shape, k


def test_published_geometry_keys():
    e = AutoencoderDC(DCAE_F32C32_SANA).expected_keys()
    assert e["encoder.conv_in.weight"] == (128, 3, 3, 3) and e["encoder.conv_out.weight"] == (32, 1024, 3, 3)
    assert e["encoder.down_blocks.0.2.conv.weight"] == (64, 128, 3, 3)                        # pixel_unshuffle: the convolution to Cout / 4
    assert e["encoder.down_blocks.3.0.attn.to_qkv_multiscale.0.proj_in.weight"] == (1536, 1, 5, 5)
    assert e["encoder.down_blocks.3.0.attn.to_qkv_multiscale.0.proj_out.weight"] == (1536, 32, 1, 1)
    assert e["encoder.down_blocks.5.2.attn.to_out.weight"] == (1024, 2048) and "encoder.down_blocks.5.3.conv.weight" not in e
    assert e["decoder.up_blocks.0.0.conv.weight"] == (512, 256, 3, 3)                         # pixel_shuffle: 4 x 128 from stage 1's 256
    assert e["decoder.up_blocks.5.0.attn.to_q.weight"] == (1024, 1024) and e["decoder.up_blocks.4.0.conv.weight"] == (4096, 1024, 3, 3)
    assert e["decoder.up_blocks.3.3.conv_out.conv_inverted.weight"] == (4096, 512, 1, 1) and e["decoder.norm_out.bias"] == (128,)
    assert sum(torch.Size(s).numel() for s in e.values()) > 300e6
    assert AutoencoderDC(DCAE_F32C32_SANA).spatial_factor == 32 and AutoencoderDC().config.scaling_factor == DCAE_CONFIG["scaling_factor"]


REFUSED = [
    (dict(attention_head_dim=64), NotImplementedError, "attention_head_dim"),
    (dict(attention_head_dim=8), NotImplementedError, "attention_head_dim"),
    (dict(decoder_norm_types="batch_norm"), NotImplementedError, "decoder_norm_types"),
    (dict(decoder_norm_types=("batch_norm", "rms_norm", "rms_norm")), NotImplementedError, "decoder_norm_types"),
    (dict(decoder_act_fns="relu6"), NotImplementedError, "decoder_act_fns"),
    (dict(decoder_act_fns=("relu", "silu", "silu")), NotImplementedError, "decoder_act_fns"),
    (dict(encoder_layers_per_block=(0, 1, 1)), NotImplementedError, r"encoder_layers_per_block\[0\]"),
    (dict(decoder_layers_per_block=(0, 1, 1)), NotImplementedError, r"decoder_layers_per_block\[0\]"),
    (dict(encoder_layers_per_block=(1, 0, 1)), NotImplementedError, "encoder_layers_per_block"),
    (dict(encoder_block_out_channels=(64, 96, 128)), NotImplementedError, "encoder_block_out_channels"),
    (dict(decoder_block_out_channels=(64, 128, 1024)), ValueError, "decoder_block_out_channels"),
    (dict(encoder_block_out_channels=(64, 128)), ValueError, "encoder"),
    (dict(latent_channels=4), NotImplementedError, "latent_channels"),
    (dict(latent_channels=24), ValueError, "latent_channels"),
    (dict(encoder_qkv_multiscales=((), (7,), ())), NotImplementedError, "encoder_qkv_multiscales"),
    (dict(encoder_block_types=("ResBlock", "Attention", "ResBlock")), ValueError, "encoder_block_types"),
    (dict(downsample_block_type="avg_pool"), ValueError, "downsample_block_type"),
    (dict(upsample_block_type="bilinear"), ValueError, "upsample_block_type"),
    (dict(sample_size=512), ValueError, "sample_size"),
    (dict(decoder_in_shortcut=False), NotImplementedError, "decoder_in_shortcut"),
]


@pytest.mark.parametrize("change,exc,match", REFUSED, ids=[",".join(c[0]) + "-" + str(i) for i, c in enumerate(REFUSED)])
def test_constructor_refusals_name_the_argument(change, exc, match):
    with pytest.raises(exc, match=match):
        AutoencoderDC(dict(R.TINY["a"], **change))


def test_dtype_refusal_and_bookkeeping_keys():
    with pytest.raises(TypeError):
        AutoencoderDC(R.TINY["a"], dtype=torch.float16)
    m = AutoencoderDC(dict(R.TINY["a"], _class_name="AutoencoderDC", _diffusers_version="0.32.0", encoder_out_shortcut=True))
    assert m.config.encoder_block_types == ("ResBlock", "EfficientViTBlock", "EfficientViTBlock") and m.config.decoder_norm_types == ("rms_norm",) * 3


def test_packed_attention_weights_are_the_reference_permutation():
    """the packed copies on the CPU: the stacked q / k / v rows, proj_in's taps and proj_out's groups in 32-blocks part * heads + g; the named
    parameters stay what was loaded"""
    sd = R.tiny_state_dict("a")
    m = AutoencoderDC(R.TINY["a"])
    m.load_state_dict(sd)
    p, C, heads = "encoder.down_blocks.1.0", 128, 4
    stack = torch.cat([sd[f"{p}.attn.{n}.weight"] for n in ("to_q", "to_k", "to_v")], 0)
    assert torch.equal(m._p[p + ".qkv_w"], R.permute_blocks(stack, heads))
    w_in, w_out = sd[f"{p}.attn.to_qkv_multiscale.0.proj_in.weight"], sd[f"{p}.attn.to_qkv_multiscale.0.proj_out.weight"]
    assert torch.equal(m._p[p + ".ms0_dw"], R.permute_blocks(w_in, heads).reshape(3 * C, 25).t())
    assert torch.equal(m._p[p + ".ms0_pw"], R.permute_blocks(w_out, heads).reshape(3 * heads, 32, 32))
    assert m._p[p + ".qkv_w"].is_contiguous() and m._p[p + ".ms0_dw"].is_contiguous()
    w = m._p["encoder.conv_in.w"]
    assert tuple(w.shape) == (64, 3, 3, 64) and torch.equal(w[:, :, :, :3], sd["encoder.conv_in.weight"].permute(0, 2, 3, 1)) and not bool(w[..., 3:].any())
    assert p + ".conv_out.conv_point.b" not in m._p and "encoder.down_blocks.0.0.conv2.b" not in m._p          # no bias: none is made up
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
