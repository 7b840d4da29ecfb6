"""GPU tests of the image front end (unigen_amd/csrc/image.hip, unigen_amd/image.py, unigen_amd/condition.py) against tests/image_ref.py (pinned by
tests/test_image_ref_cpu.py) and PIL's bytes in tests/golden/image_tiny.safetensors. Integer arithmetic or exactly specified fp32 arithmetic: every
comparison is equality on integers or on fp32 / bf16 bit patterns, no element is exempt (docs/PARITY_TOLERANCES.md, "Image front end: exact").
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import image_ref as R
from tests.test_image_ref_cpu import RESIZE_PAIRS, all_bf16_non_nan, canny_edge_case_counts, halfway_fp32

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (3, 3), (13, 17), (64, 64), (97, 131), (128, 256)]


@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return load_file(os.path.join(HERE, "golden", "image_tiny.safetensors"))


@functools.lru_cache(maxsize=None)
def canny_case(H, W, C, B, levels):
    """Input and the reference's three stages, computed once per case and shared."""
    img = R.synth(B, H, W, C, seed=11 if (H, W, C, B) == (97, 131, 3, 1) else 1000 + H + 7 * W + C + B, levels=levels)
    dx, dy, mag = R.canny_grad(img)
    emap = R.canny_nms(dx, dy, mag, 100, 200)
    return img, dx, dy, mag, emap, R.canny_hysteresis(emap)


def eq(t: torch.Tensor, a: np.ndarray) -> bool:
    return tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)


# ---- Canny ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, 4], ids=["noisy", "4level"])
@pytest.mark.parametrize("C,B", [(1, 1), (3, 1), (3, 3), (1, 3)])
@pytest.mark.parametrize("H,W", SIZES)
def test_canny_stages_and_whole(gpu, H, W, C, B, levels):
    from unigen_amd import ops
    img, dx, dy, mag, emap, edges = canny_case(H, W, C, B, levels)
    x = torch.from_numpy(img).to(gpu)
    gdx, gdy, gmag = ops.canny_grad(x)
    assert eq(gdx, dx) and eq(gdy, dy) and eq(gmag, mag)
    to = lambda a: torch.from_numpy(a).to(gpu)
    gmap = ops.canny_nms(to(dx), to(dy), to(mag), 100, 200)
    assert eq(gmap, emap)
    assert eq(ops.canny_nms(to(dx), to(dy), to(mag), 200, 100), emap)            # low > high swaps
    gedges, sweeps = ops.canny_hysteresis(to(emap))
    assert eq(gedges, edges) and 1 <= sweeps <= ops.canny_max_sweeps(H, W) == H * W + 1
    whole, sweeps = ops.canny_u8(x, 100, 200)
    assert eq(whole, edges) and 1 <= sweeps <= H * W + 1


def test_canny_four_level_case_has_the_ties(gpu):
    """The reference itself meets, on the 4-level 97 x 131 image: equal-neighbour ties in NMS, mag == low, mag == high, channel ties."""
    img = canny_case(97, 131, 3, 1, 4)[0]
    props = canny_edge_case_counts(img, 100, 200)
    assert props["nms_ties"] >= 1 and props["mag_eq_low"] >= 1 and props["mag_eq_high"] >= 1 and props["channel_ties"] >= 1, props


@pytest.mark.parametrize("C", [1, 3])
def test_canny_non_contiguous_rows(gpu, C):
    from unigen_amd import ops
    from unigen_amd.image import canny
    img, dx, dy, mag, emap, edges = canny_case(97, 131, C, 3, None)
    for pad in (5, 13):                       # a window of a wider image: row stride (131 + pad) * C bytes, not a multiple of 4 / a multiple of 4 with C = 1
        wide = torch.zeros(3, 99, 131 + pad, C, dtype=torch.uint8, device=gpu)
        view = wide[:, 1:98, 2:133]
        view.copy_(torch.from_numpy(img))
        assert not view.is_contiguous()
        gdx, gdy, gmag = ops.canny_grad(view)
        assert eq(gdx, dx) and eq(gdy, dy) and eq(gmag, mag)
        assert eq(ops.canny_u8(view)[0], edges)
    assert np.array_equal(canny(img[0]), edges[0]) and np.array_equal(canny(img), edges)          # ndarray in, ndarray out
    assert eq(canny(torch.from_numpy(img).to(gpu)), edges)
    if C == 1:
        assert np.array_equal(canny(img[0, :, :, 0]), edges[0])


def _serpentine(H, W):
    """A one-pixel-wide path: every second row, joined alternately at the right and the left end. Returns the map (0 on the path, 1 elsewhere) and
    the path's pixels in order."""
    m = np.ones((H, W), np.uint8)
    path = []
    for i, y in enumerate(range(0, H, 2)):
        xs = range(W) if i % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if i % 2 == 0 else 0))
    for y, x in path:
        m[y, x] = 0
    return m, path


def test_hysteresis_hand_built_maps(gpu):
    from unigen_amd import ops
    H, W = 96, 160
    bound = ops.canny_max_sweeps(H, W)
    assert bound == H * W + 1

    def run(m):
        out, sweeps = ops.canny_hysteresis(torch.from_numpy(m[None]).to(gpu))
        assert 1 <= sweeps <= bound
        return out[0].cpu().numpy(), sweeps

    snake, path = _serpentine(H, W)
    on_path = snake == 0
    seeded = snake.copy()
    seeded[path[0]] = 2
    out, sweeps = run(seeded)                                     # crosses every 64 x 32 tile many times: all of it turns 255
    assert np.array_equal(out, np.where(on_path, 255, 0).astype(np.uint8)) and sweeps > 3
    assert np.array_equal(out, R.canny_hysteresis(seeded[None])[0])
    cut = 161 * 31 + 80                                           # the middle of a run (a run and its connector are 161 pixels)
    gap = seeded.copy()
    gap[path[cut]] = 1                                            # a one-pixel gap: only the seeded part
    want = np.zeros((H, W), np.uint8)
    for y, x in path[:cut]:
        want[y, x] = 255
    assert path[cut][1] not in (0, W - 1)                         # the gap sits inside a run, so nothing bridges it diagonally
    out, _ = run(gap)
    assert np.array_equal(out, want) and np.array_equal(out, R.canny_hysteresis(gap[None])[0])
    tail = snake.copy()
    tail[path[-1]] = 2                                            # seeded at the other end: promotion runs against the scan order too
    assert np.array_equal(run(tail)[0], np.where(on_path, 255, 0).astype(np.uint8))
    diag = np.ones((H, W), np.uint8)
    idx = np.arange(H)
    diag[idx, idx + 30] = 0                                       # a diagonal-only chain, and an anti-diagonal one
    diag[idx, 159 - idx - 40] = 0
    diag[0, 30] = 2
    diag[95, 159 - 95 - 40] = 2
    out, _ = run(diag)
    assert np.array_equal(out, np.where(diag != 1, 255, 0).astype(np.uint8))
    none = snake.copy()
    none[::7, ::5] = 0                                            # candidates, no strong pixel: all zero, one sweep
    out, sweeps = run(none)
    assert not out.any() and sweeps == 1
    out, sweeps = run(np.full((H, W), 2, np.uint8))               # all strong
    assert (out == 255).all() and sweeps == 1


# ---- resize, convert("L") against PIL's bytes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("pair", RESIZE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_resize_against_fixture(gpu, pair, C):
    from unigen_amd.image import resize_u8
    (H, W), (h, w) = pair
    g = golden()
    src = g[f"in_{H}x{W}"][None, :, :, :C].contiguous().to(gpu)
    want = g[f"resize{C}_{H}x{W}_{h}x{w}"].reshape(1, h, w, C)
    got = resize_u8(src, h, w)
    assert torch.equal(got.cpu(), want)
    batch = torch.cat([src, src.flip(1), src.flip(2)], 0)         # B = 3 agrees with the reference, image by image
    assert np.array_equal(resize_u8(batch, h, w).cpu().numpy(), R.resize(batch.cpu().numpy(), h, w))
    wide = torch.zeros(1, H + 2, W + 3, C, dtype=torch.uint8, device=gpu)       # a strided view
    wide[:, 1:H + 1, 3:].copy_(src)
    assert torch.equal(resize_u8(wide[:, 1:H + 1, 3:], h, w).cpu(), want)


def test_resize_large_ratio_takes_the_unstaged_path(gpu):
    """A workgroup's 256 outputs read more input bytes than the staged span holds: 16 x 20000 x 3 -> 16 x 300."""
    from unigen_amd.image import resize_u8
    img = R.synth(1, 16, 20000, 3, seed=9)
    assert np.array_equal(resize_u8(torch.from_numpy(img).to(gpu), 16, 300).cpu().numpy(), R.resize(img, 16, 300))


def test_rgb_to_l_against_fixture(gpu):
    from unigen_amd import ops
    g = golden()
    for k in [k for k in g if k.startswith("in")]:
        assert torch.equal(ops.img_rgb_to_l(g[k][None].to(gpu)).cpu()[0, :, :, 0], g["l_" + k]), k
    grid = torch.from_numpy(np.stack(np.meshgrid(np.arange(0, 256, 3), np.arange(0, 256, 3), np.arange(0, 256, 5), indexing="ij"), -1)
                            .reshape(2, 86, -1, 3).astype(np.uint8))
    assert np.array_equal(ops.img_rgb_to_l(grid.to(gpu)).cpu().numpy(), R.rgb_to_l(grid.numpy()))


# ---- the converters ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("W", [1, 7, 64])
def test_u8_to_chw_all_values(gpu, W, dtype):
    from unigen_amd import ops
    H = 256 * 3 // W + 3
    v = (np.arange(H * W * 3) // 3 + np.arange(H * W * 3) % 3 * 85) % 256     # every byte value in every channel position, several times over
    img = v.astype(np.uint8).reshape(1, H, W, 3).repeat(2, 0)
    img[1] = 255 - img[1]
    for c in range(3):
        assert len(np.unique(img[0, :, :, c])) == 256
    x = torch.from_numpy(img).to(gpu)
    bits = lambda t: t.cpu().view(torch.int32 if t.dtype == F32 else torch.int16)
    for normalize in (True, False):
        assert torch.equal(bits(ops.img_u8_to_chw(x, normalize=normalize, dtype=dtype)), bits(R.u8_to_chw(img, normalize, dtype)))
    gray = x[..., :1].contiguous()
    assert torch.equal(bits(ops.img_u8_to_chw(gray, dtype=dtype)), bits(R.u8_to_chw(img[..., :1], True, dtype)))
    assert torch.equal(bits(ops.img_u8_to_chw(gray, dtype=dtype, replicate=True)), bits(R.u8_to_chw(img[..., :1], True, dtype, replicate=True)))


def test_chw_to_u8_all_bf16_patterns(gpu):
    from unigen_amd import ops
    x = all_bf16_non_nan()                                       # 65282 values, the infinities included
    n = x.numel()
    for C, H, W in ((1, 1, n), (3, 26, 837), (2, 127, 258), (4, 3, 5448)):   # W = 837, 258: the guarded path; 5448 = 8 * 681: the 16-byte path
        t = x.repeat(3)[: C * H * W].reshape(1, C, H, W).contiguous()
        assert C * H * W >= n
        assert np.array_equal(ops.img_chw_to_u8(t.to(gpu)).cpu().numpy(), R.chw_to_u8(t))
    t = x[: 64 * 1020].reshape(1, 1, 64, 1020)
    raw = lambda u: (u.float().clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(ops.img_chw_to_u8(t.to(gpu), denormalize=False).cpu(), raw(t))


def test_chw_to_u8_fp32_with_halfway_points(gpu):
    from unigen_amd import ops
    x = torch.cat([all_bf16_non_nan().float(), halfway_fp32(), torch.nextafter(halfway_fp32(), torch.tensor(2.0)),
                   torch.nextafter(halfway_fp32(), torch.tensor(-2.0))])
    n = x.numel()
    for C, H, W in ((1, 1, n), (3, 29, 761), (3, 5, 4404)):     # 761 odd; 4404 a multiple of 4 above one 1024-pixel segment
        t = x.repeat(3)[: C * H * W].reshape(1, C, H, W).contiguous()
        assert C * H * W >= n
        assert np.array_equal(ops.img_chw_to_u8(t.to(gpu)).cpu().numpy(), R.chw_to_u8(t))


# ---- VaeImageProcessor -----------------------------------------------------------------------------------------------------------------------------------
def test_processor_round_trip_resize_list_and_batch(gpu):
    from unigen_amd.image import VaeImageProcessor
    p = VaeImageProcessor(vae_scale_factor=16)
    img = R.synth(2, 64, 48, 3, seed=21)
    x = p.preprocess(img)
    assert x.dtype == F32 and x.is_cuda and tuple(x.shape) == (2, 3, 64, 48)
    assert torch.equal(x.cpu(), R.u8_to_chw(img))
    back = p.postprocess(x, output_type="u8")
    assert back.is_cuda and np.array_equal(back.cpu().numpy(), img)                    # unchanged size: the image comes back exactly
    assert np.array_equal(p.postprocess(x.to(BF), output_type="u8").cpu().numpy(), R.chw_to_u8(x.cpu().to(BF)))
    assert np.array_equal(p.postprocess(x, output_type="np"), ((x.cpu() * 0.5 + 0.5).clamp(0, 1)).permute(0, 2, 3, 1).numpy())
    odd = R.synth(2, 75, 53, 3, seed=22)
    assert torch.equal(p.preprocess(odd).cpu(), R.u8_to_chw(R.resize(odd, 64, 48)))    # default size rounded down to the factor
    assert torch.equal(p.preprocess(odd, height=40, width=100).cpu(), R.u8_to_chw(R.resize(odd, 32, 96)))
    as_list = p.preprocess([odd[0], torch.from_numpy(odd[1])])
    assert torch.equal(as_list, p.preprocess(odd)) and torch.equal(as_list[:1], p.preprocess(odd[0]))
    assert torch.equal(p.preprocess(torch.from_numpy(odd).to(gpu)), as_list)
    gray = VaeImageProcessor(vae_scale_factor=16, do_convert_grayscale=True).preprocess(odd)
    assert torch.equal(gray.cpu(), R.u8_to_chw(R.resize(R.rgb_to_l(odd), 64, 48)))
    rgb = VaeImageProcessor(vae_scale_factor=16, do_convert_rgb=True, do_normalize=False).preprocess(odd[..., :1])
    assert torch.equal(rgb.cpu(), R.u8_to_chw(R.resize(odd[..., :1], 64, 48), normalize=False, replicate=True))
    Image = pytest.importorskip("PIL.Image")
    pil = Image.fromarray(odd[0])
    assert torch.equal(p.preprocess(pil), as_list[:1])
    want = np.array(pil.resize((48, 64), Image.LANCZOS))
    out = p.postprocess(p.preprocess(pil), output_type="pil")
    assert len(out) == 1 and out[0].mode == "RGB" and np.array_equal(np.array(out[0]), want)


# ---- Condition and the pipeline ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny_pipe():
    from safetensors import safe_open
    from oracle import vae_ref as V
    from unigen_amd.image import VaeImageProcessor
    from unigen_amd.pipeline import UniGenFLUXPipeline
    from unigen_amd.vae import AutoencoderKL
    with safe_open(os.path.join(HERE, "golden", "vae_tiny.safetensors"), "pt") as f:
        meta = f.metadata()
    cfg_d, case = json.loads(meta["config"]), json.loads(meta["case"])
    cfg_d["block_out_channels"] = tuple(cfg_d["block_out_channels"])
    state = V.make_vae_state(V.VAEConfig(**cfg_d), seed=case["state_seed"])
    dev = torch.device("cuda:0")
    vae = AutoencoderKL.from_config(cfg_d, device=dev, dtype=BF)
    res = vae.load_state_dict({k: v.to(dev, BF) for k, v in state.items()})
    assert not res.missing_keys and not res.unexpected_keys
    scale = 2 ** (len(cfg_d["block_out_channels"]) - 1)
    return UniGenFLUXPipeline(vae=vae, vae_scale_factor=scale, image_processor=VaeImageProcessor(vae_scale_factor=2 * scale))


def test_condition_encode(gpu):
    from unigen_amd.condition import Condition
    from unigen_amd.image import canny
    from unigen_amd.pipeline import pack_latents
    pipe = tiny_pipe()
    img = R.synth(1, 35, 34, 3, seed=31)[0]                        # preprocess rounds to 32 x 32 (the VAE's mid-block attention wants 16 x 16 latents)
    cond = Condition("canny", raw_img=img)
    edges = R.canny(img[None])[0]
    assert np.array_equal(cond.condition, np.repeat(edges[..., None], 3, -1)) and cond.type_id == 1
    gen = lambda: torch.Generator(device=gpu).manual_seed(5)
    tokens, ids, type_id = cond.encode(pipe, generator=gen())
    C = pipe.vae.config.latent_channels
    assert tuple(tokens.shape) == (1, 16 * 16 // 4, 4 * C) and tuple(ids.shape) == (64, 3) and tuple(type_id.shape) == (64, 1)
    assert bool((type_id == 1).all())
    x = pipe.image_processor.preprocess(np.repeat(canny(img)[..., None], 3, -1))
    assert tuple(x.shape) == (1, 3, 32, 32)
    z = pipe.vae.encode_scaled(x.to(BF), generator=gen())
    assert torch.equal(tokens, pack_latents(z.contiguous()))
    want_ids = torch.zeros(8, 8, 3)
    want_ids[..., 1] += torch.arange(8)[:, None]
    want_ids[..., 2] += torch.arange(8)[None]
    assert torch.equal(ids.float().cpu(), want_ids.reshape(64, 3))
    s_tokens, s_ids, s_type = Condition("subject", raw_img=img).encode(pipe, generator=gen())
    assert torch.equal(s_ids[:, 2].float().cpu(), want_ids.reshape(64, 3)[:, 2] + 8) and torch.equal(s_ids[:, :2], ids[:, :2])
    assert bool((s_type == 4).all()) and tuple(s_tokens.shape) == tuple(tokens.shape)
    col = Condition("coloring", raw_img=img)
    assert np.array_equal(col.condition, np.repeat(R.rgb_to_l(img[None])[0], 3, -1))


def test_pipeline_prepare_image(gpu):
    from unigen_amd.pipeline import UniGenFLUXPipeline
    pipe = tiny_pipe()
    img = R.synth(1, 42, 37, 3, seed=33)[0]
    want = pipe.image_processor.preprocess(img, height=32, width=24)
    got = pipe.prepare_image(img, 24, 32, 3, 2, gpu, BF)
    assert tuple(got.shape) == (3, 3, 32, 24) and got.dtype == BF
    assert torch.equal(got, want.repeat_interleave(3, dim=0).to(BF))          # one image serves the whole batch
    two = pipe.prepare_image([img, img[::-1].copy()], 24, 32, 2, 2, gpu, F32)
    assert torch.equal(two, pipe.image_processor.preprocess([img, img[::-1].copy()], height=32, width=24).repeat_interleave(2, dim=0))
    with pytest.raises(NotImplementedError, match="no image processor is attached"):
        UniGenFLUXPipeline().prepare_image(img, 24, 32, 1, 1, gpu, BF)
