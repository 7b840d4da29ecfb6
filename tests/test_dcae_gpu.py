"""AutoencoderDC (unigen_amd/dcae.py) against tests/dcae_ref.py: whole-model paths with the bounds of tests/test_vae_gpu.py - the fp32 path within 1e-3
rel-L2 of the float64 truth; the bf16 path no further from that truth than 1.25 x the reference's own bf16 evaluation on the CPU.

Configuration "a" (tests/golden/dcae_tiny.safetensors holds its inputs and float64 outputs): "Conv" / "interpolate", one layer per stage, a 5 x 5 scale at
the middle stage; 32 x 32 (64 and 256 tokens at the attention stages) and 24 x 40 images. Configuration "b": "pixel_unshuffle" / "pixel_shuffle", two
layers per stage, widths (64, 128, 256), the reference evaluated here; its 16 x 16 image has 16 tokens at the last stage, where diffusers takes its
quadratic branch and this package the same linear kernel. Configuration "w": two EfficientViTBlock stages at the published attention widths 512 and
1024 (16 and 32 heads, G = 48 and 96 in the multiscale projection, GLU at 2048 and 4096 channels), 32 latent channels, on a 24 x 40 image: two row and
two column tiles of ug_msconv_proj written in place behind its input, N = 960 and 240 tokens, the shortcuts 512 <-> 1024 and the latent ones with a
group and a repeat of 32. Its 66 M weights come from the seeded grid; the fixture holds its float64 outputs too (their evaluation takes longer than
all the rest of its test), tests/test_dcae_ref_cpu.py checks them against a fresh evaluation, and the reference's bf16 evaluation is made here, once
per process."""
import os
import time

import pytest
import torch

from tests import dcae_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcae_tiny.safetensors")


def rel(a, b):
    return float((a.detach().double().cpu() - b.double()).norm() / b.double().norm())


_TRUTH = {}


def truth(run):
    """(float64 latent, float64 image, bf16-evaluated latent, bf16-evaluated image) of a run; "a" and "w" read the float64 pair from the fixture"""
    if run not in _TRUTH:
        name = R.TINY_RUNS[run][0]
        if name in ("a", "w"):
            from safetensors.torch import load_file
            fx = load_file(GOLDEN)
            assert torch.equal(fx["fingerprint" if name == "a" else "fingerprint.w"], R.fingerprint(name)), \
                "the seeded weight generator no longer gives the fixture's weights"
            assert torch.equal(fx[f"run{run}.x"], R.tiny_inputs(run)["x"]) and torch.equal(fx[f"run{run}.z"], R.tiny_inputs(run)["z"])
            lat, img = fx[f"run{run}.latent"], fx[f"run{run}.sample"]
        else:
            lat, img = R.evaluate(run)
        lat16, img16 = R.evaluate(run, BF)
        _TRUTH[run] = (lat, img, lat16, img16)
    return _TRUTH[run]


_MODELS = {}


def model(name, dtype, gpu):
    from unigen_amd.dcae import AutoencoderDC
    if (name, dtype) not in _MODELS:
        m = AutoencoderDC(R.TINY[name], device=gpu, dtype=dtype)
        missing, unexpected = m.load_state_dict(R.tiny_state_dict(name))
        assert not missing and not unexpected
        _MODELS[(name, dtype)] = m
    return _MODELS[(name, dtype)]


@pytest.mark.parametrize("run", range(len(R.TINY_RUNS)))
def test_encode_decode_against_fp64(gpu, run):
    name = R.TINY_RUNS[run][0]
    i = R.tiny_inputs(run)
    t0 = time.perf_counter()
    lat, img, lat16, img16 = truth(run)
    t1 = time.perf_counter()
    m32, m16 = model(name, F32, gpu), model(name, BF, gpu)
    z32, y32 = m32.encode(i["x"].float()).latent, m32.decode(i["z"].float()).sample
    assert z32.shape == lat.shape and y32.shape == img.shape and z32.dtype == F32
    e_z32, e_y32 = rel(z32, lat), rel(y32, img)
    z16, y16 = m16.encode(i["x"]).latent, m16.decode(i["z"]).sample
    assert z16.dtype == BF and bool(torch.isfinite(z16).all()) and bool(torch.isfinite(y16).all())
    e_z, e_y, r_z, r_y = rel(z16, lat), rel(y16, img), rel(lat16, lat), rel(img16, img)
    print(f"run {run} {R.TINY_RUNS[run]}: fp32 path encode {e_z32:.3e} decode {e_y32:.3e} (bound 1e-3); bf16 encode {e_z:.3e} (reference's bf16 {r_z:.3e}) "
          f"decode {e_y:.3e} ({r_y:.3e}); the reference took {t1 - t0:.1f} s of {time.perf_counter() - t0:.1f} s")
    assert e_z32 <= 1e-3 and e_y32 <= 1e-3, (e_z32, e_y32)
    assert e_z <= 1.25 * r_z and e_y <= 1.25 * r_y, (e_z, r_z, e_y, r_y)


def test_state_dict_round_trip_and_keys(gpu):
    from unigen_amd.dcae import AutoencoderDC
    for name in ("a", "b"):
        sd = R.tiny_state_dict(name)
        m = model(name, BF, gpu)
        assert set(m.expected_keys()) == set(sd) == set(R.DCAERef(**R.TINY[name]).state_dict())      # every key is consumed, none is unexpected
        out = m.state_dict()
        assert list(out) == list(m.expected_keys())
        for k, v in sd.items():
            assert out[k].dtype == BF and torch.equal(out[k].cpu(), v), k
        m2 = AutoencoderDC(R.TINY[name], device=gpu, dtype=BF)
        with pytest.raises(KeyError, match="missing"):
            m2.load_state_dict({k: v for k, v in sd.items() if not k.endswith("norm_out.bias")})
        with pytest.raises(KeyError, match="unexpected"):
            m2.load_state_dict(dict(sd, **{"encoder.mid_block.weight": torch.zeros(1)}))
        with pytest.raises(ValueError, match="shape"):
            m2.load_state_dict(dict(sd, **{"encoder.conv_in.bias": torch.zeros(3)}))


def test_from_pretrained_and_forward(gpu, tmp_path):
    import json
    from safetensors.torch import save_file
    from unigen_amd.dcae import AutoencoderDC
    cfg = dict(R.TINY["a"], _class_name="AutoencoderDC", _diffusers_version="0.32.0")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in R.tiny_state_dict("a").items()}, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    m = AutoencoderDC.from_pretrained(str(tmp_path), device=gpu)
    assert m.config.scaling_factor == 0.41407 and m.dtype == BF and m.spatial_factor == 4
    x = R.tiny_inputs(0)["x"]
    z = m.encode(x).latent
    assert torch.equal(z, model("a", BF, gpu).encode(x).latent)
    y = m(x).sample                                      # forward = decode(encode(x))
    assert y.shape == x.shape and torch.equal(y, m.decode(z).sample) and torch.equal(m.decode(z, return_dict=False)[0], y)
    assert torch.equal(m(x).sample, y), "decode(encode(x)) is deterministic: DC-AE has no posterior"
    with pytest.raises(OSError):
        AutoencoderDC.from_pretrained(str(tmp_path / "nowhere"))


def test_refusals_at_run_time(gpu):
    m = model("a", BF, gpu)
    with pytest.raises(ValueError, match="spatial factor 4"):
        m.encode(torch.zeros(1, 3, 30, 32))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m.encode(torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError, match=r"\[B, 8, H, W\]"):
        m.decode(torch.zeros(1, 3, 8, 8))
    from unigen_amd.dcae import AutoencoderDC
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        AutoencoderDC(R.TINY["a"], device=gpu).encode(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="backward"):
        m.set_trainable()


def test_published_geometry_runs_and_repeats(gpu):
    """dc-ae-f32c32-sana geometry, synthetic weights made on the device: one encode and one decode of a 256 x 256 image, finite, and the same bits again"""
    from unigen_amd.dcae import DCAE_F32C32_SANA, AutoencoderDC
    m = AutoencoderDC(DCAE_F32C32_SANA, device=gpu).init_synthetic_(3)
    assert m.spatial_factor == 32 and m.config.latent_channels == 32
    g = torch.Generator(device=gpu).manual_seed(4)
    x = torch.randn(1, 3, 256, 256, generator=g, device=gpu).to(BF)
    z = m.encode(x).latent
    assert z.shape == (1, 32, 8, 8) and bool(torch.isfinite(z).all())
    y = m.decode(z).sample
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    assert torch.equal(m.encode(x).latent, z) and torch.equal(m.decode(z).sample, y)
