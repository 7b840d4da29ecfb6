"""AutoencoderKL tiling and slicing on the GPU. Kernel: ug_vae_tile_blend / _f32 against the literal restatement of diffusers' blend / crop / cat
(tests/vae_tiled_ref.py, evaluated on the CPU) - exact equality over the CPU test's shape list, every stride layout the kernel has a path for, NaN
canvases inside guard bands. Model: tiled_decode / tiled_encode and the routed decode / encode of a tiny VAE against the same literal algorithm driven
by the model's OWN untiled decode / encode per tile - exact equality, both sides run the same kernels on the same tiles."""
import functools
import importlib

import pytest
import torch

from tests import vae_tiled_ref as TR

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
TINY = dict(block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32)       # scale factor 2, as tests/golden/vae_tiny.safetensors
GUARD = 64                                                                                # elements either side of a canvas (keeps its 16-byte alignment)
# (tile layout, canvas layout, channels): the 8-channel path with a C % 8 tail; the decoder's NHWC rows -> NCHW canvas with one padded group (C = 3 in
# rows of 8) and with a second group; element-by-element for everything else
LAYOUTS = [("nhwc", "nhwc", 11), ("nhwc", "nchw", 3), ("nhwc", "nchw", 11), ("nchw", "nchw", 3)]


def _id(c):
    return f"B{c['B']}_{c['H']}x{c['W']}_f{c['f']}"


@functools.lru_cache(maxsize=None)
def _case_ref(idx, C, dt):
    rows, E, crop = TR.random_tiles(TR.CASES[idx], C, dt, seed=10 + idx)
    return rows, E, crop, TR.literal_from_tiles(rows, E, crop)


def _pad8(n):
    return (n + 7) // 8 * 8


def _upload(t, layout, gpu):
    """raw CPU tile [B, C, H, W] -> its logical [B, C, H, W] view on the device in the given memory layout"""
    B, C, H, W = t.shape
    if layout == "nchw":
        return t.to(gpu).contiguous()
    rows = torch.zeros(B * H * W, _pad8(C), dtype=t.dtype)
    rows[:, :C] = t.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return rows.to(gpu).view(B, H, W, _pad8(C)).permute(0, 3, 1, 2)[:, :C]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l[0]}-{l[1]}-C{l[2]}")
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("idx", range(len(TR.CASES)), ids=lambda i: _id(TR.CASES[i]))
def test_tile_blend_kernel_equals_literal_reference(gpu, idx, dt, layout):
    """One launch per tile through the host's own loop. Canvas widths of 2 x {4, 6, 15, 17, 19, 20, 21}: rows that start off a 16-byte boundary, heads
    and tails of every length, tiles narrower than 8, element counts that are no multiple of the 256-thread block. The canvas starts as NaN between two NaN
    guard bands: afterwards every canvas element equals the reference (so each was written) and both bands, like the channels a padded NHWC canvas has
    beyond C, still hold NaN."""
    lib = importlib.import_module("unigen_amd.lib")
    assert getattr(lib.load(), "ug_vae_tile_blend" if dt == BF else "ug_vae_tile_blend_f32") is not None      # the exported symbol this test is about
    AutoencoderKL = importlib.import_module("unigen_amd.vae").AutoencoderKL
    src, dst, C = layout
    rows, E, crop, want = _case_ref(idx, C, dt)
    B, _, Hc, Wc = want.shape
    grid = [[_upload(t, src, gpu) for t in row] for row in rows]
    Cc = _pad8(C) if dst == "nhwc" else C
    n = B * Cc * Hc * Wc
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dt, device=gpu)
    body = buf[GUARD:GUARD + n]
    canvas = body.view(B, Hc, Wc, Cc).permute(0, 3, 1, 2)[:, :C] if dst == "nhwc" else body.view(B, C, Hc, Wc)
    AutoencoderKL._blend_tiles(canvas, grid, E, crop)
    torch.cuda.synchronize()
    got = canvas.cpu()
    assert torch.equal(got, want), (TR.CASES[idx], layout, int((got != want).sum()), int(torch.isnan(got.float()).sum()))
    assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[GUARD + n:].float()).all()), "wrote outside the canvas"
    if Cc > C:
        assert bool(torch.isnan(body.view(B, Hc, Wc, Cc)[..., C:].float()).all()), "wrote channels beyond C"


def test_tile_blend_refuses_what_the_closed_form_cannot_do(gpu):
    from unigen_amd import lib, ops
    t = lambda h, w: torch.zeros(1, 3, h, w, device=gpu, dtype=BF)
    out = torch.zeros(1, 3, 8, 8, device=gpu, dtype=BF)
    with pytest.raises(lib.UniGenHipError, match="at least 2 E"):
        ops.vae_tile_blend(t(8, 8), t(8, 8), None, None, out, 5)                 # U.H = 8 < e_v + E = 10
    with pytest.raises(lib.UniGenHipError, match="upper-left tile"):
        ops.vae_tile_blend(t(8, 8), t(8, 8), t(8, 8), None, out, 4)
    with pytest.raises(lib.UniGenHipError, match="upper tile must have T's width"):
        ops.vae_tile_blend(t(8, 8), t(8, 7), None, None, out, 4)
    assert torch.equal(ops.vae_tile_blend(t(8, 8) + 1, None, None, None, out, 4), torch.ones_like(out))      # no neighbours: the crop, copied


# ----------------------------------------------------------------------------------------------------------------------------------
# model
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(gpu, dt):
    cls = importlib.import_module("unigen_amd.vae").AutoencoderKL
    m = cls.from_config(dict(TINY), device=gpu, dtype=BF).init_synthetic_(3)
    if dt == F32:
        m32 = cls.from_config(dict(TINY), device=gpu, dtype=F32)
        m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
        m = m32
    m.tile_latent_min_size, m.tile_sample_min_size, m.tile_overlap_factor = 16, 32, 0.25
    return m


def _fresh(m):
    m.disable_tiling(); m.disable_slicing()
    return m


def _moments_nchw(m, x):
    """the model's own untiled encoder (+ quant_conv) on one tile, as an NCHW tensor of its own"""
    rows, B, h, w = m._encode_moments(x)
    return rows.view(B, h, w, rows.shape[1]).permute(0, 3, 1, 2).clone()


@pytest.mark.parametrize("shape", [(32, 32), (32, 44), (32, 8)], ids=["32x32", "32x44", "32x8"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_tiled_decode_equals_literal_over_the_models_own_untiled_decode(gpu, dt, shape):
    """latent 32 -> tiles of 16, 16, 8 (every tile's H*W a multiple of 64); non-square: 44 wide -> 16, 16, 16, 8, and 8 wide -> one column of tiles.
    (A 32 x 16 latent cannot be tiled at this tile size: see test_a_32x16_latent_is_refused_up_front.)"""
    m = _fresh(_model(gpu, dt))
    z = torch.randn(2, 16, *shape, generator=torch.Generator().manual_seed(5)).to(gpu, dt)
    stride, E, crop = TR.plan(16, 2, 0.25)
    assert (stride, E, crop) == (12, 8, 24)
    want = TR.tiled_literal(z, lambda t: m.decode(t, return_dict=False)[0], 16, stride, E, crop)
    want_scaled = TR.tiled_literal(z, lambda t: m.decode_scaled(t), 16, stride, E, crop)
    assert want.shape == (2, 3, 2 * shape[0], 2 * shape[1]) and not torch.equal(want, want_scaled)
    assert torch.equal(m.tiled_decode(z).sample, want) and torch.equal(m.tiled_decode(z, return_dict=False)[0], want)
    plain = m.decode(z).sample                                   # tiling off: the whole canvas at once - a different image at the seams
    assert plain.shape == want.shape and not torch.equal(plain, want)
    m.enable_tiling()
    assert torch.equal(m.decode(z).sample, want) and torch.equal(m.decode(z, return_dict=False)[0], want)
    assert torch.equal(m.decode_scaled(z), want_scaled)


@pytest.mark.parametrize("shape", [(64, 64), (64, 88), (64, 16)], ids=["64x64", "64x88", "64x16"])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_tiled_encode_equals_literal_over_the_models_own_untiled_encode(gpu, dt, shape):
    """the mirror image: sample tiles of 32, 32, 16 (stride 24), the MOMENTS blended over int(16 * 0.25) = 4 and cropped to 12"""
    from unigen_amd import ops
    m = _fresh(_model(gpu, dt))
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(2, 3, *shape, generator=g) * 2 - 1).to(gpu, dt)
    stride, E, crop = TR.plan(32, 2, 0.25, down=True)
    assert (stride, E, crop) == (24, 4, 12)
    want = TR.tiled_literal(x, lambda t: _moments_nchw(m, t), 32, stride, E, crop)            # [B, Cp, H / 2, W / 2]
    B, Cp, Hl, Wl = want.shape
    assert (Hl, Wl) == (shape[0] // 2, shape[1] // 2)
    nchw = lambda d: d._m.view(B, Hl, Wl, Cp).permute(0, 3, 1, 2)
    assert torch.equal(nchw(m.tiled_encode(x).latent_dist), want) and torch.equal(nchw(m.tiled_encode(x, return_dict=False)[0]), want)
    assert not torch.equal(nchw(m.encode(x).latent_dist), want)                                # tiling off: one pass over the whole image
    m.enable_tiling()
    d = m.encode(x).latent_dist
    assert torch.equal(nchw(d), want) and torch.equal(d.mode(), want[:, :16])
    noise = torch.randn(B, 16, Hl, Wl, generator=g).to(gpu, dt)
    rows = want.permute(0, 2, 3, 1).reshape(B * Hl * Wl, Cp).contiguous()
    want_z = ops.vae_sample(rows, noise, B=B, latent=16, H=Hl, W=Wl, shift=m.config.shift_factor, scale=m.config.scaling_factor)
    assert torch.equal(m.encode_scaled(x, noise=noise), want_z)


def test_a_32x16_latent_is_refused_up_front(gpu):
    """diffusers' loop starts a tile at every multiple of the stride below the size, so a side of exactly one tile (16) still gets a second tile
    of 16 - 12 = 4: the 32 x 16 latent has a last tile of 8 x 4 = 32 tokens, which the mid-block attention does not take. The tiled route says so
    before it launches anything; with tiling off the same latent decodes (512 tokens)."""
    from unigen_amd import lib
    m = _fresh(_model(gpu, BF))
    z = torch.randn(1, 16, 32, 16, generator=torch.Generator().manual_seed(4)).to(gpu, BF)
    assert m.decode(z).sample.shape == (1, 3, 64, 32)
    m.enable_tiling()
    before = set(m._ws._bufs)
    with pytest.raises(lib.UniGenHipError, match=r"mid-block attention needs H\*W at the latent resolution to be a multiple of 64 \(got 32\)"):
        m.decode(z)
    assert set(m._ws._bufs) == before                       # no tile ran


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_tiling_on_leaves_inputs_up_to_the_tile_size_alone(gpu, dt):
    m = _fresh(_model(gpu, dt))
    g = torch.Generator().manual_seed(7)
    zs = [torch.randn(1, 16, h, w, generator=g).to(gpu, dt) for h, w in ((16, 16), (8, 16), (16, 4))]
    xs = [(torch.rand(1, 3, h, w, generator=g) * 2 - 1).to(gpu, dt) for h, w in ((32, 32), (16, 32))]
    off = [m.decode(z).sample for z in zs] + [m.decode_scaled(z) for z in zs] + [m.encode(x).latent_dist._m for x in xs]
    m.enable_tiling()
    on = [m.decode(z).sample for z in zs] + [m.decode_scaled(z) for z in zs] + [m.encode(x).latent_dist._m for x in xs]
    assert all(torch.equal(a, b) for a, b in zip(off, on))


@pytest.mark.parametrize("tiling", [False, True], ids=["untiled", "tiled"])
def test_slicing_equals_the_single_sample_calls(gpu, tiling):
    m = _fresh(_model(gpu, BF))
    m.enable_tiling(tiling)
    g = torch.Generator().manual_seed(8)
    z = torch.randn(3, 16, 32, 8, generator=g).to(gpu, BF)
    x = (torch.rand(3, 3, 64, 16, generator=g) * 2 - 1).to(gpu, BF)
    want_img = torch.cat([m.decode(z[i:i + 1]).sample for i in range(3)])
    want_scaled = torch.cat([m.decode_scaled(z[i:i + 1]) for i in range(3)])
    want_mode = torch.cat([m.encode(x[i:i + 1]).latent_dist.mode() for i in range(3)])
    m.enable_slicing()
    assert torch.equal(m.decode(z).sample, want_img) and torch.equal(m.decode_scaled(z), want_scaled)
    d = m.encode(x).latent_dist
    assert d._shape == (3, 16, 32, 8) and torch.equal(d.mode(), want_mode)


def test_tiled_route_keeps_the_attention_scratch_at_tile_size(gpu):
    """the point of tiling: the mid-block attention's [HW, HW] scores never exceed one tile's (16 x 16 = 256 tokens), where the untiled decode of the
    same 32 x 32 latent holds 1024 x 1024"""
    cls = importlib.import_module("unigen_amd.vae").AutoencoderKL
    shapes = lambda m: {k[1] for k in m._ws._bufs if k[0] == "at_s"}
    z = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(9)).to(gpu, BF)
    m = cls.from_config(dict(TINY), device=gpu, dtype=BF).init_synthetic_(3)
    m.tile_latent_min_size, m.tile_sample_min_size = 16, 32
    m.enable_tiling()
    m.decode(z)
    assert shapes(m) == {(256, 256), (128, 128), (64, 64)}, shapes(m)
    m.disable_tiling()
    m.decode(z)
    assert (1024, 1024) in shapes(m)


def test_pipeline_enable_vae_tiling_equals_the_vae_level_call(gpu):
    """UniGenFLUXPipeline with pixels in and output_type='pt' at 160 x 160: latent 20 x 20 = 2 x 2 tiles of 16 and 8 (tile_latent_min_size 16), the
    condition image 2 x 2 tiles of 128 and 64. The images the pipeline returns are the VAE-level tiled decode of the latents it handed over, which
    in turn is the literal algorithm over the untiled decode."""
    r = lambda g, *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(BF)
    tcfg = dict(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
    tr = importlib.import_module("src.UniGenTransformer").UniGenFlux.from_config(tcfg, device=gpu, dtype=BF)
    tr.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True,
                                                                                               single_control_dev=2))
    tr.init_synthetic_(seed=1, std=0.05, bias_std=0.02)
    vae = importlib.import_module("unigen_amd.vae").AutoencoderKL.from_config(dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1), device=gpu, dtype=BF).init_synthetic_(2)
    vae.tile_latent_min_size, vae.tile_sample_min_size = 16, 128
    pipe = importlib.import_module("src.UniGenPipeline").UniGenFLUXPipeline.from_pretrained(None, transformer=tr)
    pipe.vae = vae
    pipe.enable_vae_tiling()
    assert vae.use_tiling
    seen = []
    inner = vae.decode_scaled
    vae.decode_scaled = lambda z: seen.append(z.clone()) or inner(z)
    g = torch.Generator().manual_seed(0)
    B, H, W = 1, 160, 160
    img = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(BF)
    out = pipe(prompt_embeds=r(g, B, 16, 64, scale=0.1), pooled_prompt_embeds=r(g, B, 64), condition_pooled_prompt_embeds=r(g, B, 64), control_image=img, height=H,
               width=W, num_inference_steps=2, generator=g, output_type="pt").images
    del vae.decode_scaled
    assert out.shape == (B, 3, H, W) and len(seen) == 1 and seen[0].shape == (B, 16, 20, 20)
    assert torch.equal(out, vae.decode_scaled(seen[0]))
    stride, E, crop = TR.plan(16, 8, 0.25)
    pipe.disable_vae_tiling()
    assert not vae.use_tiling
    want = TR.tiled_literal(seen[0], lambda t: vae.decode_scaled(t), 16, stride, E, crop)
    assert torch.equal(out, want)
    # both VAE stages went tile by tile: no attention scratch beyond a 16 x 16 tile's (the 400-token latent would not even pass the untiled rule)
    assert {k[1] for k in vae._ws._bufs if k[0] == "at_s"} == {(256, 256), (128, 128), (64, 64)}
