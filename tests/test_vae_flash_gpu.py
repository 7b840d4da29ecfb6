"""AutoencoderKL.enable_flash_attention(): the mid-block attention as one flash-attention launch over the batch (unigen_amd/vae.py, _flash_attention).

  - decode and encode with the switch on against the oracle (oracle/vae_ref.py on the CPU), bounds of tests/test_vae_gpu.py: fp32 rel-L2 <= 1e-3, bf16 no
    further from the fp32 truth than 1.25 x the oracle's own bf16 evaluation - at a 512-wide mid-block (ug_flash_attn_fwd_wide) with 256 tokens and with
    240 (no multiple of 64: this route masks ragged tails), and at the 128-wide TINY configuration (ug_flash_attn_fwd);
  - the route's attention scratch is q, k, v, o at [B*HW, C]: no [HW, HW] scores or probabilities, no v^T;
  - switched off again, the model is bit-identical to one that never had it on; a mid-block width without a flash kernel (256) is refused by name;
  - tiling composes: the tiled routes equal the literal per-tile algorithm over the model's own untiled flash decode / encode, a 32-token corner
    tile included (which the default route refuses, unchanged); the pipeline-level switch is the VAE-level one."""
import functools
import importlib

import pytest
import torch

from oracle import vae_ref as V
from tests import vae_tiled_ref as TR
from tests.util import rel_l2, report

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
WIDE = dict(block_out_channels=(64, 512), layers_per_block=1, norm_num_groups=32)       # one 512-wide head: the width of the FLUX / SD3.5 VAE's mid-block
TINY = dict(block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32)
CONFIGS = dict(wide=WIDE, tiny=TINY)
SCRATCH_OF_THE_DEFAULT_ROUTE = ("at_s", "at_p", "at_vT")


def _cls():
    return importlib.import_module("unigen_amd.vae").AutoencoderKL


def _new(gpu, cfg, dt=BF, seed=3):
    m = _cls().from_config(dict(cfg), device=gpu, dtype=BF).init_synthetic_(seed)
    if dt == F32:
        m32 = _cls().from_config(dict(cfg), device=gpu, dtype=F32)
        res = m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
        assert not res.missing_keys and not res.unexpected_keys
        return m32
    return m


@functools.lru_cache(maxsize=None)
def _oracle(name, h, w):
    """the oracle's configuration and the inputs of one case: images [2, 3, 2h, 2w], noise and latents [2, 16, h, w] (drawn once, read-only)"""
    cfg = V.VAEConfig(**CONFIGS[name])
    g = torch.Generator().manual_seed(40 + h)
    img = (torch.rand(2, 3, 2 * h, 2 * w, generator=g) * 2 - 1).to(BF)
    noise = torch.randn(2, 16, h, w, generator=g).to(BF)
    lat = torch.randn(2, 16, h, w, generator=g).to(BF)
    return cfg, img, noise, lat


@pytest.mark.parametrize("name,h,w", [("wide", 16, 16), ("wide", 12, 20), ("tiny", 16, 16), ("tiny", 12, 20)],
                         ids=["wide-256tok", "wide-240tok", "tiny-256tok", "tiny-240tok"])
def test_flash_route_matches_the_oracle(gpu, name, h, w):
    cfg, img, noise, lat = _oracle(name, h, w)
    m16, m32 = _new(gpu, CONFIGS[name], BF), _new(gpu, CONFIGS[name], F32)
    state = {k: v.detach().cpu() for k, v in m16.state_dict().items()}
    assert set(state) == set(V.vae_state_shapes(cfg))
    for m in (m16, m32):
        assert m.use_flash_attention is False
        m.enable_flash_attention()
        assert m.use_flash_attention is True
    z_t, z_r = V.encode_condition(state, cfg, img, noise, F32), V.encode_condition(state, cfg, img, noise, BF)
    z32 = m32.encode_scaled(img.to(gpu), noise=noise.to(gpu))
    r = report(f"vae_flash_encode_f32_{name}_{h}x{w}", z32, z_t)
    assert z32.shape == z_t.shape and r["rel_l2"] <= 1e-3, r
    z16 = m16.encode_scaled(img.to(gpu), noise=noise.to(gpu))
    e_hip, e_ref = rel_l2(z16, z_t), rel_l2(z_r, z_t)
    report(f"vae_flash_encode_bf16_{name}_{h}x{w}", z16, z_r, err_hip_vs_fp32=e_hip, err_oraclebf16_vs_fp32=e_ref)
    assert e_hip <= 1.25 * e_ref, ("encode", e_hip, e_ref)
    d_t, d_r = V.decode_latents(state, cfg, lat, F32), V.decode_latents(state, cfg, lat, BF)
    d32 = m32.decode_scaled(lat.to(gpu))
    r = report(f"vae_flash_decode_f32_{name}_{h}x{w}", d32, d_t)
    assert d32.shape == (2, 3, 2 * h, 2 * w) and r["rel_l2"] <= 1e-3, r
    d16 = m16.decode_scaled(lat.to(gpu))
    e_hip, e_ref = rel_l2(d16, d_t), rel_l2(d_r, d_t)
    report(f"vae_flash_decode_bf16_{name}_{h}x{w}", d16, d_r, err_hip_vs_fp32=e_hip, err_oraclebf16_vs_fp32=e_ref)
    assert e_hip <= 1.25 * e_ref, ("decode", e_hip, e_ref)
    if (h * w) % 64:                                       # the default route still refuses this token count
        lib = importlib.import_module("unigen_amd.lib")
        m16.disable_flash_attention()
        with pytest.raises(lib.UniGenHipError, match="multiple of 64"):
            m16.decode_scaled(lat.to(gpu))


@pytest.mark.parametrize("name", ["wide", "tiny"])
def test_flash_route_allocates_no_score_scratch(gpu, name):
    m = _new(gpu, CONFIGS[name])
    C = CONFIGS[name]["block_out_channels"][-1]
    m.enable_flash_attention()
    g = torch.Generator().manual_seed(9)
    m.decode(torch.randn(2, 16, 16, 16, generator=g).to(gpu, BF))
    m.encode((torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(gpu, BF))
    torch.cuda.synchronize()
    att = {k[0]: k[1] for k in m._ws._bufs if k[0].startswith("at_")}
    assert not set(att) & set(SCRATCH_OF_THE_DEFAULT_ROUTE), att
    assert att == {n: (2 * 256, C) for n in ("at_n", "at_q", "at_k", "at_v", "at_o")}, att
    # ... where the default route on the same model holds the [256, 256] scores (and would hold [HW, HW] at any size)
    m.disable_flash_attention()
    m.decode(torch.randn(2, 16, 16, 16, generator=g).to(gpu, BF))
    assert {"at_s", "at_p", "at_vT"} <= {k[0] for k in m._ws._bufs}


def test_switching_off_restores_the_default_route_bit_for_bit(gpu):
    a, b = _new(gpu, WIDE), _new(gpu, WIDE)
    g = torch.Generator().manual_seed(10)
    z = torch.randn(2, 16, 16, 16, generator=g).to(gpu, BF)
    x = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(gpu, BF)
    a.enable_flash_attention()
    on = a.decode(z).sample.clone()
    a.encode(x)
    a.disable_flash_attention()
    assert a.use_flash_attention is False
    want_img, want_m = b.decode(z).sample, b.encode(x).latent_dist._m
    assert torch.equal(a.decode(z).sample, want_img) and torch.equal(a.encode(x).latent_dist._m, want_m)
    # the two routes round at the same point (P to bf16) but sum in another order: close, not equal
    assert not torch.equal(on, want_img) and rel_l2(on, want_img) <= 2e-2


def test_a_width_without_a_flash_kernel_is_refused(gpu):
    lib = importlib.import_module("unigen_amd.lib")
    m = _new(gpu, dict(WIDE, block_out_channels=(64, 256)))
    z = torch.randn(1, 16, 16, 16, generator=torch.Generator().manual_seed(11)).to(gpu, BF)
    img = m.decode(z).sample
    assert img.shape == (1, 3, 32, 32) and bool(torch.isfinite(img.float()).all())
    m.enable_flash_attention()
    with pytest.raises(lib.UniGenHipError, match=r"512, 128 or 64, not 256.*default route"):
        m.decode(z)


@pytest.mark.parametrize("name", ["wide", "tiny"])
def test_tiling_composes_with_the_flash_route(gpu, name):
    m = _new(gpu, CONFIGS[name])
    m.tile_latent_min_size, m.tile_sample_min_size, m.tile_overlap_factor = 16, 32, 0.25
    m.enable_flash_attention()
    g = torch.Generator().manual_seed(12)
    z = torch.randn(2, 16, 32, 44, generator=g).to(gpu, BF)                      # tiles of 16, 16, 8 x 16, 16, 16, 8
    stride, E, crop = TR.plan(16, 2, 0.25)
    want = TR.tiled_literal(z, lambda t: m.decode(t, return_dict=False)[0], 16, stride, E, crop)
    x = (torch.rand(2, 3, 64, 88, generator=g) * 2 - 1).to(gpu, BF)
    s2, E2, crop2 = TR.plan(32, 2, 0.25, down=True)

    def moments(t):
        rows, B, h, w = m._encode_moments(t)
        return rows.view(B, h, w, rows.shape[1]).permute(0, 3, 1, 2).clone()
    want_m = TR.tiled_literal(x, moments, 32, s2, E2, crop2)
    m.enable_tiling()
    assert torch.equal(m.decode(z).sample, want)
    B, Cp, Hl, Wl = want_m.shape
    assert torch.equal(m.encode(x).latent_dist._m.view(B, Hl, Wl, Cp).permute(0, 3, 1, 2), want_m)
    m.enable_slicing()
    assert torch.equal(m.decode(z).sample, torch.cat([m.decode(z[i:i + 1]).sample for i in range(2)]))
    assert not set(SCRATCH_OF_THE_DEFAULT_ROUTE) & {k[0] for k in m._ws._bufs}


def test_a_32_token_corner_tile_decodes_on_the_flash_route_only(gpu):
    """[1, 16, 32, 16] at tile 16, stride 12: the last column of tiles is 4 wide, its last tile 8 x 4 = 32 tokens. The default route refuses it up
    front (tests/test_vae_tiled_gpu.py pins the message); the flash kernels mask ragged tails, so the tile plan consults the switch."""
    lib = importlib.import_module("unigen_amd.lib")
    m = _new(gpu, TINY)
    m.tile_latent_min_size, m.tile_sample_min_size, m.tile_overlap_factor = 16, 32, 0.25
    z = torch.randn(1, 16, 32, 16, generator=torch.Generator().manual_seed(4)).to(gpu, BF)
    m.enable_tiling()
    with pytest.raises(lib.UniGenHipError, match=r"mid-block attention needs H\*W at the latent resolution to be a multiple of 64 \(got 32\)"):
        m.decode(z)
    m.enable_flash_attention()
    m.disable_tiling()
    stride, E, crop = TR.plan(16, 2, 0.25)
    want = TR.tiled_literal(z, lambda t: m.decode(t, return_dict=False)[0], 16, stride, E, crop)
    m.enable_tiling()
    got = m.decode(z).sample
    assert got.shape == (1, 3, 64, 32) and torch.equal(got, want) and bool(torch.isfinite(got.float()).all())
    m.disable_flash_attention()
    with pytest.raises(lib.UniGenHipError, match=r"multiple of 64 \(got 32\)"):
        m.decode(z)


def test_pipeline_enable_vae_flash_attention_equals_the_vae_level_call(gpu):
    r = lambda g, *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(BF)
    tcfg = dict(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
    tr = importlib.import_module("src.UniGenTransformer").UniGenFlux.from_config(tcfg, device=gpu, dtype=BF)
    tr.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True,
                                                                                               single_control_dev=2))
    tr.init_synthetic_(seed=1, std=0.05, bias_std=0.02)
    vcfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
    vae, twin = _cls().from_config(dict(vcfg), device=gpu, dtype=BF).init_synthetic_(2), _cls().from_config(dict(vcfg), device=gpu, dtype=BF).init_synthetic_(2)
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=tr)
    with pytest.raises(RuntimeError, match="no VAE is attached"):
        pipe.enable_vae_flash_attention()
    pipe.vae = vae
    pipe.enable_vae_flash_attention()
    assert vae.use_flash_attention is True
    seen = []
    inner = vae.decode_scaled
    vae.decode_scaled = lambda z: seen.append(z.clone()) or inner(z)
    g = torch.Generator().manual_seed(0)
    B, H, W = 2, 128, 128
    img = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(BF)
    out = pipe(prompt_embeds=r(g, B, 16, 64, scale=0.1), pooled_prompt_embeds=r(g, B, 64), condition_pooled_prompt_embeds=r(g, B, 64), control_image=img, height=H,
               width=W, num_inference_steps=2, generator=g, output_type="pt").images
    del vae.decode_scaled
    assert out.shape == (B, 3, H, W) and len(seen) == 1
    twin.enable_flash_attention()                                     # the VAE-level call, on a model the pipeline never touched
    assert torch.equal(out, twin.decode_scaled(seen[0]))
    assert not set(SCRATCH_OF_THE_DEFAULT_ROUTE) & {k[0] for k in vae._ws._bufs}       # the encode of the condition image and the decode: both flash
    pipe.disable_vae_flash_attention()
    assert vae.use_flash_attention is False
    twin.disable_flash_attention()
    assert torch.equal(vae.decode_scaled(seen[0]), twin.decode_scaled(seen[0])) and not torch.equal(vae.decode_scaled(seen[0]), out)
    sd3 = importlib.import_module("unigen_amd.pipeline").UniGenSD3Pipeline
    assert callable(getattr(sd3, "enable_vae_flash_attention")) and callable(getattr(sd3, "disable_vae_flash_attention"))
