"""CPU checks of tests/image_ref.py, the numpy restatement that tests/test_image_gpu.py compares the image kernels with, and of the host logic of
unigen_amd/image.py and unigen_amd/condition.py that needs no GPU. Every comparison is equality.

Canny is restated from OpenCV's published source and no cv2 vectors exist here ("parity unpinned"), so its stages are checked
against independent implementations: Sobel against scipy.ndimage.correlate, hysteresis against scipy.ndimage.label, the channel choice and the NMS
rules against a naive per-pixel loop. The resampler and convert("L") are pinned against PIL itself and against the committed fixture.
"""
import os

import numpy as np
import pytest
import torch

from tests import image_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_tiny.safetensors")
RESIZE_PAIRS = [((64, 48), (32, 32)), ((33, 47), (64, 80)), ((100, 60), (37, 23)), ((48, 48), (48, 96)), ((1024, 16), (512, 16)), ((16, 1024), (16, 512))]


@pytest.fixture(scope="module")
def golden():
    from safetensors.torch import load_file
    return {k: v.numpy() for k, v in load_file(GOLDEN).items()}


# ---- Canny against independent implementations -------------------------------------------------------------------------------------------------------
def test_sobel_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    img = R.synth(2, 37, 53, 3, seed=1)
    dx, dy = R.sobel(img)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    for b in range(2):
        for c in range(3):
            plane = img[b, :, :, c].astype(np.int32)
            assert np.array_equal(dx[b, :, :, c], ndi.correlate(plane, kx, mode="nearest"))
            assert np.array_equal(dy[b, :, :, c], ndi.correlate(plane, kx.T, mode="nearest"))


def _naive_grad_nms(img, low, high):
    """Per-pixel Python: Sobel with clamped coordinates, the strongest channel (strict >), then cv::Canny's NMS rules."""
    H, W, C = img.shape
    px = lambda y, x, c: int(img[min(max(y, 0), H - 1), min(max(x, 0), W - 1), c])
    dx, dy, mag = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            best = None
            for c in range(C):
                gx = (px(y - 1, x + 1, c) + 2 * px(y, x + 1, c) + px(y + 1, x + 1, c)) - (px(y - 1, x - 1, c) + 2 * px(y, x - 1, c) + px(y + 1, x - 1, c))
                gy = (px(y + 1, x - 1, c) + 2 * px(y + 1, x, c) + px(y + 1, x + 1, c)) - (px(y - 1, x - 1, c) + 2 * px(y - 1, x, c) + px(y - 1, x + 1, c))
                m = abs(gx) + abs(gy)
                if best is None or m > best[2]:
                    best = (gx, gy, m)
            dx[y, x], dy[y, x], mag[y, x] = best
    mg = lambda y, x: int(mag[y, x]) if 0 <= y < H and 0 <= x < W else 0
    out = np.ones((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            m = mg(y, x)
            if not m > low:
                continue
            xs, ys = int(dx[y, x]), int(dy[y, x])
            ax, ay = abs(xs), abs(ys) << 15
            if ay < ax * 13573:
                keep = m > mg(y, x - 1) and m >= mg(y, x + 1)
            elif ay > ax * 13573 + (ax << 16):
                keep = m > mg(y - 1, x) and m >= mg(y + 1, x)
            else:
                s = -1 if (xs ^ ys) < 0 else 1
                keep = m > mg(y - 1, x - s) and m > mg(y + 1, x + s)
            if keep:
                out[y, x] = 2 if m > high else 0
    return dx, dy, mag, out


@pytest.mark.parametrize("levels", [None, 4])
def test_channel_choice_and_nms_against_naive_loop(levels):
    img = R.synth(1, 11, 9, 3, seed=3, levels=levels)
    dx, dy, mag = R.canny_grad(img)
    ndx, ndy, nmag, nmap = _naive_grad_nms(img[0], 100, 200)
    assert np.array_equal(dx[0], ndx) and np.array_equal(dy[0], ndy) and np.array_equal(mag[0], nmag)
    assert np.array_equal(R.canny_nms(dx, dy, mag, 100, 200)[0], nmap)
    assert np.array_equal(R.canny_nms(dx, dy, mag, 200, 100)[0], nmap)          # low > high swaps


@pytest.mark.parametrize("levels", [None, 4])
def test_hysteresis_against_scipy_label(levels):
    ndi = pytest.importorskip("scipy.ndimage")
    img = R.synth(2, 61, 83, 3, seed=5, levels=levels)
    emap = R.canny_nms(*R.canny_grad(img), 100, 200)
    got = R.canny_hysteresis(emap)
    for b in range(2):
        lab, n = ndi.label(emap[b] != 1, structure=np.ones((3, 3), int))
        keep = np.unique(lab[emap[b] == 2])
        want = np.where(np.isin(lab, keep[keep > 0]), 255, 0).astype(np.uint8)
        assert (emap[b] == 0).any() and (emap[b] == 2).any()
        assert np.array_equal(got[b], want)
    assert np.array_equal(R.canny(img), got)


def test_four_level_image_meets_the_edge_cases():
    """The properties the GPU test relies on, of the same image it uses."""
    img = R.synth(1, 97, 131, 3, seed=11, levels=4)
    props = canny_edge_case_counts(img, 100, 200)
    assert all(v > 0 for v in props.values()), props


def canny_edge_case_counts(img, low, high):
    dxc, dyc = R.sobel(img)
    magc = np.abs(dxc) + np.abs(dyc)
    top = magc.max(-1)
    dx, dy, mag = R.canny_grad(img)
    m = mag.astype(np.int64)
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    H, W = m.shape[1:]
    eq = np.zeros(m.shape, bool)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            if (oy, ox) != (0, 0):
                eq |= (p[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W] == m)
    return dict(nms_ties=int((eq & (m > low)).sum()), mag_eq_low=int((m == low).sum()), mag_eq_high=int((m == high).sum()),
                channel_ties=int((((magc == top[..., None]).sum(-1) > 1) & (top > 0)).sum()))


# ---- the resampler and convert("L") against PIL and the fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RESIZE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_resize_against_pil(pair):
    Image = pytest.importorskip("PIL.Image")
    (H, W), (h, w) = pair
    img = R.synth(1, H, W, 3, seed=41)
    assert np.array_equal(R.resize(img, h, w)[0], np.array(Image.fromarray(img[0]).resize((w, h), Image.LANCZOS)))
    gray = img[..., :1]
    assert np.array_equal(R.resize(gray, h, w)[0, :, :, 0], np.array(Image.fromarray(gray[0, :, :, 0], mode="L").resize((w, h), Image.LANCZOS)))


def test_resize_against_pil_large_ratio_and_tables_match_the_package():
    Image = pytest.importorskip("PIL.Image")
    from unigen_amd.image import resample_tables
    img = R.synth(1, 96, 200, 3, seed=43)
    for h, w in ((8, 8), (200, 96), (96, 199)):
        assert np.array_equal(R.resize(img, h, w)[0], np.array(Image.fromarray(img[0]).resize((w, h), Image.LANCZOS)))
    for a, b in ((200, 8), (96, 200), (1536, 1024), (47, 80), (16, 16)):
        for got, want in zip(resample_tables(a, b), R.resample_tables(a, b)):
            assert np.array_equal(got, want)


@pytest.mark.parametrize("pair", RESIZE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_resize_against_fixture(golden, pair):
    (H, W), (h, w) = pair
    img = golden[f"in_{H}x{W}"]
    assert np.array_equal(R.resize(img[None], h, w)[0], golden[f"resize3_{H}x{W}_{h}x{w}"])
    assert np.array_equal(R.resize(img[None, :, :, :1], h, w)[0, :, :, 0], golden[f"resize1_{H}x{W}_{h}x{w}"])


def test_rgb_to_l_against_fixture_and_pil(golden):
    names = [k for k in golden if k.startswith("in")]
    assert len(names) >= 7
    for k in names:
        assert np.array_equal(R.rgb_to_l(golden[k][None])[0, :, :, 0], golden["l_" + k]), k
    assert np.array_equal(R.resize(golden["in4_100x60"][None], 37, 23)[0], golden["resize3_in4_100x60_37x23"])
    Image = pytest.importorskip("PIL.Image")
    rgb = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij"), -1).reshape(1, -1, 52, 3).astype(np.uint8)
    assert np.array_equal(R.rgb_to_l(rgb)[0, :, :, 0], np.array(Image.fromarray(rgb[0]).convert("L")))


# ---- the converters against diffusers' torch / numpy formulas --------------------------------------------------------------------------------------------
def test_u8_to_chw_all_byte_values():
    img = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, -1)
    x = np.array(img[0]).astype(np.float32) / 255.0                     # pil_to_numpy
    t = torch.from_numpy(x[None].transpose(0, 3, 1, 2))                   # numpy_to_pt
    assert torch.equal(R.u8_to_chw(img, normalize=False), t)
    assert torch.equal(R.u8_to_chw(img, normalize=True), 2.0 * t - 1.0)   # normalize
    assert torch.equal(R.u8_to_chw(img, normalize=True, dtype=torch.bfloat16), (2.0 * t - 1.0).to(torch.bfloat16))
    assert torch.equal(R.u8_to_chw(img[..., :1], replicate=True), 2.0 * t - 1.0)


def all_bf16_non_nan():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16)
    return x[~torch.isnan(x.float())]


def halfway_fp32():
    """(k + 0.5) / 255 mapped back through 2 x - 1: where * 255 lands on (or next to) a rounding tie."""
    k = torch.arange(255, dtype=torch.float32)
    return 2.0 * ((k + 0.5) / 255.0) - 1.0


def test_chw_to_u8_all_bf16_patterns_and_halfway_points():
    x = all_bf16_non_nan()
    assert x.numel() == 65536 - 2 * 127 and torch.isinf(x.float()).sum() == 2
    for t in (x.reshape(1, 1, -1, 1), torch.cat([x.float(), halfway_fp32()]).reshape(1, 1, -1, 1)):
        want = (t * 0.5 + 0.5).clamp(0, 1)                                               # denormalize
        want = want.cpu().permute(0, 2, 3, 1).float().numpy()                             # pt_to_numpy
        want = (want * 255).round().astype("uint8")                                       # numpy_to_pil
        assert np.array_equal(R.chw_to_u8(t), want)


# ---- host logic of the package that needs no GPU ---------------------------------------------------------------------------------------------------------
def test_processor_sizes_and_argument_errors():
    from unigen_amd.image import VaeImageProcessor, _as_u8_batch
    p = VaeImageProcessor(vae_scale_factor=16)
    assert p.config["resample"] == "lanczos" and p.config["do_normalize"] and not p.config["do_convert_rgb"] and VaeImageProcessor().vae_scale_factor == 8
    img = np.zeros((37, 50, 3), np.uint8)
    assert p.get_default_height_width(img) == (32, 48)
    assert p.get_default_height_width(img[None]) == (32, 48)
    assert p.get_default_height_width(img, height=100, width=17) == (96, 16)
    assert p.get_default_height_width(torch.zeros(1, 3, 64, 80)) == (64, 80)
    with pytest.raises(ValueError):
        p.get_default_height_width(np.zeros((8, 50, 3), np.uint8))
    for bad in ("bilinear", "bicubic", "nearest"):
        with pytest.raises(NotImplementedError, match="LANCZOS"):
            VaeImageProcessor(resample=bad)
    with pytest.raises(ValueError):
        VaeImageProcessor(do_convert_rgb=True, do_convert_grayscale=True)
    with pytest.raises(TypeError):
        _as_u8_batch(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        _as_u8_batch(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(TypeError):
        _as_u8_batch("image.png")
    assert _as_u8_batch(np.zeros((4, 5), np.uint8)).shape == (1, 4, 5, 1)
    with pytest.raises(ValueError):
        p.postprocess(torch.zeros(1, 3, 8, 8), output_type="jpeg")
    z = torch.zeros(1, 3, 8, 8)
    assert p.postprocess(z, output_type="latent") is z
    f = torch.rand(2, 3, 8, 8)
    assert torch.equal(p.preprocess(f), 2.0 * f - 1.0) and torch.equal(p.preprocess(f - 0.5), f - 0.5)       # float tensors pass as diffusers passes them
    assert torch.equal(p.postprocess(f, output_type="pt"), (f * 0.5 + 0.5).clamp(0, 1))
    assert p.postprocess(f, output_type="np").shape == (2, 8, 8, 3)


def test_condition_host_logic():
    import src.condition as S
    from unigen_amd.condition import Condition, condition_dict
    assert S.Condition is Condition and S.condition_dict is condition_dict
    assert condition_dict == {"depth": 0, "canny": 1, "subject": 4, "coloring": 6, "deblurring": 7, "fill": 9}
    img = np.zeros((16, 16, 3), np.uint8)
    for name, tid in condition_dict.items():
        if name in ("subject", "fill"):
            c = Condition(name, raw_img=img)
            assert c.type_id == tid and np.array_equal(c.condition, img) and c.condition_ids is None
    assert Condition("canny", raw_img=img, no_process=True).type_id == 1
    assert Condition("fill", raw_img=img[..., 0]).condition.shape == (16, 16, 3)
    with pytest.raises(NotImplementedError, match="depth-estimation"):
        Condition("depth", raw_img=img)
    with pytest.raises(NotImplementedError, match="GaussianBlur"):
        Condition("deblurring", raw_img=img)
    with pytest.raises(AssertionError):
        Condition("canny")
    tok, ids = torch.zeros(1, 4, 8), torch.zeros(4, 3)
    c = Condition("depth", condition=tok, condition_ids=ids)
    t, i, tid = c.encode(None)
    assert t is tok and i is ids and tid.shape == (4, 1) and bool((tid == 0).all())
    with pytest.raises(NotImplementedError, match="image_processor"):
        Condition("fill", raw_img=img).encode(type("P", (), {"image_processor": None, "vae": None})())


def test_pipeline_errors_name_the_processor():
    from unigen_amd.pipeline import UniGenFLUXPipeline, UniGenSD3Pipeline
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="unigen_amd.image.VaeImageProcessor"):
        UniGenFLUXPipeline().prepare_image(img, 16, 16, 1, 1, "cpu", torch.float32)
    with pytest.raises(NotImplementedError, match="unigen_amd.image.VaeImageProcessor"):
        UniGenSD3Pipeline().prepare_image(img, 16, 16, 1, 1, "cpu", torch.float32)
