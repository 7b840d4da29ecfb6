"""GPU tests of the blur kernels (unigen_amd/csrc/image.hip: ug_img_box_blur_u8; unigen_amd/image.py box_blur, gaussian_blur, VaeImageProcessor.blur;
unigen_amd/condition.py deblurring_image) against PIL's bytes in tests/golden/blur_tiny.safetensors and against tests/blur_ref.py (pinned against PIL
by tests/test_blur_ref_cpu.py). Integer arithmetic: every comparison is equality, no element is exempt (docs/PARITY_TOLERANCES.md, "Image front end:
exact"). Every case runs with fuse=1 (all passes of an axis in one launch where the halo fits in LDS) and with fuse=0 (one launch per pass).
"""
import functools

import numpy as np
import pytest
import torch

from tests import blur_ref as R
from tests.image_ref import synth
from tests.test_blur_ref_cpu import consts_of, fixture_cases, ref_blur

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cases_of(H, W):
    """The fixture's cases of one size, read once."""
    return [c for c in fixture_cases() if c[1].shape[:2] == (H, W)]


def run_ops(x, kind, radius, fuse):
    from unigen_amd import ops
    (cx, cy), passes = consts_of(kind, radius)
    return ops.img_box_blur_u8(x, cx, cy, passes, fuse=fuse)


@pytest.mark.parametrize("H,W", R.SIZES, ids=lambda v: str(v))
def test_fixture_cases(gpu, H, W):
    """Every stored output, as RGB and with channel 0 as "L", through ops with fuse=1 and fuse=0 and through gaussian_blur / box_blur."""
    from unigen_amd.image import box_blur, gaussian_blur
    cases = cases_of(H, W)
    assert len(cases) == 2 * len(R.filters(H, W))
    for cid, img, kind, radius, want in cases:
        x = torch.from_numpy(img[None]).to(gpu)
        gray = x[..., :1].contiguous()
        for fuse in (True, False):
            assert np.array_equal(run_ops(x, kind, radius, fuse)[0].cpu().numpy(), want), (cid, fuse)
            assert np.array_equal(run_ops(gray, kind, radius, fuse)[0, :, :, 0].cpu().numpy(), want[..., 0]), (cid, "L", fuse)
        fn = gaussian_blur if kind == "gaussian" else box_blur
        assert np.array_equal(fn(img, radius), want), cid
        assert np.array_equal(fn(np.ascontiguousarray(img[..., 0]), radius), want[..., 0]), (cid, "L")


def test_batch_of_three_different_images(gpu):
    g = {c[0]: c for c in cases_of(40, 50)}
    a, b = g["g10_in_40x50"], g["g10_bw_40x50"]
    third = np.ascontiguousarray(a[1][::-1, ::-1])
    batch = np.stack([a[1], b[1], third])
    want = np.stack([a[4], b[4], np.ascontiguousarray(a[4][::-1, ::-1])])            # the blur commutes with a flip of both axes
    assert np.array_equal(ref_blur(batch, "gaussian", 10), want)
    x = torch.from_numpy(batch).to(gpu)
    for fuse in (True, False):
        assert np.array_equal(run_ops(x, "gaussian", 10, fuse).cpu().numpy(), want), fuse
        assert np.array_equal(run_ops(x[..., 1:2].contiguous(), "gaussian", 10, fuse).cpu().numpy(), want[..., 1:2]), fuse


@pytest.mark.parametrize("C", [1, 3])
def test_non_contiguous_rows(gpu, C):
    """A 37-wide crop of a 41-wide image: with C = 3 the row stride is 123 bytes and no row but the first starts on a dword; two samples, so the
    sample stride is not the crop's size either. The crop starts one row and three pixels in."""
    from unigen_amd.image import gaussian_blur
    img = synth(2, 33, 37, C, seed=50 + C)
    wide = torch.full((2, 35, 41, C), 77, dtype=torch.uint8, device=gpu)
    view = wide[:, 1:34, 3:40]
    view.copy_(torch.from_numpy(img))
    assert not view.is_contiguous() and view.stride(1) == 41 * C
    for kind, radius in (("gaussian", 10), ("box", 2), ("gaussian", (0, 3.7)), ("gaussian", (3.7, 0))):
        want = ref_blur(img, kind, radius)
        for fuse in (True, False):
            assert np.array_equal(run_ops(view, kind, radius, fuse).cpu().numpy(), want), (kind, radius, fuse)
    out = gaussian_blur(view, 10)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), ref_blur(img, "gaussian", 10))
    assert bool((wide[:, 0] == 77).all()) and bool((wide[:, :, :3] == 77).all()) and bool((wide[:, :, 40:] == 77).all())        # the source is only read


# The kernels' tiles: 256 pixels x 8 rows along rows; 128 bytes (128 gray or 42 2/3 RGB pixels) x 96 rows along columns. One less, exactly, one more.
TILE_EDGE_SIZES = [(95, 255), (96, 256), (97, 257), (7, 127), (8, 128), (9, 129), (193, 42), (17, 43), (192, 86)]


@functools.lru_cache(maxsize=None)
def tile_edge_case(H, W):
    img = synth(1, H, W, 3, seed=600 + H + W)
    return img, ref_blur(img, "gaussian", 10), ref_blur(img[..., :1], "gaussian", 10)


@pytest.mark.parametrize("H,W", TILE_EDGE_SIZES, ids=lambda v: str(v))
def test_sizes_at_the_tile_edges(gpu, H, W):
    img, want3, want1 = tile_edge_case(H, W)
    x = torch.from_numpy(img).to(gpu)
    for fuse in (True, False):
        assert np.array_equal(run_ops(x, "gaussian", 10, fuse).cpu().numpy(), want3), fuse
        assert np.array_equal(run_ops(x[..., :1].contiguous(), "gaussian", 10, fuse).cpu().numpy(), want1), fuse


def test_radii_whose_halo_does_not_fit(gpu):
    """GaussianBlur(25) (r = 24: three passes need 75 rows of halo, more than a column tile holds, so the columns run pass by pass), BoxBlur(60)
    (r + 1 = 61 rows: past the column tile, straight from memory; r + 1 > H) and BoxBlur(130) (past the row tile too, r + 1 > W)."""
    img = synth(2, 57, 131, 3, seed=70)
    x = torch.from_numpy(img).to(gpu)
    for kind, radius in (("gaussian", 25), ("box", 60), ("box", 130), ("box", (130.5, 0.5)), ("gaussian", (1, 40))):
        want = ref_blur(img, kind, radius)
        assert np.array_equal(want, ref_blur(img, kind, radius, R.line_running))
        for fuse in (True, False):
            assert np.array_equal(run_ops(x, kind, radius, fuse).cpu().numpy(), want), (kind, radius, fuse)
            assert np.array_equal(run_ops(x[..., 2:].contiguous(), kind, radius, fuse).cpu().numpy(), want[..., 2:]), (kind, radius, fuse)


def test_radius_zero_is_a_copy(gpu):
    from unigen_amd.image import box_blur, gaussian_blur
    img = synth(1, 21, 22, 3, seed=71)[0]
    x = torch.from_numpy(img).to(gpu)
    for out in (gaussian_blur(x, 0), gaussian_blur(x, (0, 0)), box_blur(x, 0)):
        assert out.data_ptr() != x.data_ptr() and torch.equal(out, x)


def test_image_kinds(gpu):
    """PIL in, PIL out; ndarray in, ndarray out; a CPU tensor comes back on the CPU; a GPU tensor stays on the GPU; [H, W], [H, W, C], [B, H, W, C]."""
    from unigen_amd.image import VaeImageProcessor, box_blur, gaussian_blur
    img = synth(2, 31, 29, 3, seed=72)
    want = ref_blur(img, "gaussian", 4)
    out = gaussian_blur(img, 4)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    assert np.array_equal(gaussian_blur(img[0], 4), want[0]) and np.array_equal(gaussian_blur(img[0, :, :, 1], 4), want[0, :, :, 1])
    t = torch.from_numpy(img)
    out = gaussian_blur(t, 4)
    assert isinstance(out, torch.Tensor) and not out.is_cuda and np.array_equal(out.numpy(), want)
    out = gaussian_blur(t.to(gpu), 4)
    assert out.is_cuda and out.device == t.to(gpu).device and np.array_equal(out.cpu().numpy(), want)
    out = VaeImageProcessor.blur(t[0].to(gpu))                                        # diffusers' default blur_factor = 4
    assert out.is_cuda and tuple(out.shape) == (31, 29, 3) and np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(VaeImageProcessor.blur(img[1], blur_factor=4), want[1])
    assert np.array_equal(box_blur(img, (2, 0.5)), ref_blur(img, "box", (2, 0.5)))
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    pil = Image.fromarray(img[0])
    out = VaeImageProcessor.blur(pil, 4)
    assert isinstance(out, Image.Image) and out.mode == "RGB" and np.array_equal(np.array(out), np.array(pil.filter(ImageFilter.GaussianBlur(4))))
    assert np.array_equal(np.array(out), want[0])
    gray = Image.fromarray(img[0, :, :, 0])
    out = box_blur(gray, 2)
    assert out.mode == "L" and np.array_equal(np.array(out), np.array(gray.filter(ImageFilter.BoxBlur(2))))


def test_deblurring_image_and_condition(gpu):
    from tests.test_image_gpu import tiny_pipe
    from unigen_amd.condition import Condition, deblurring_image
    from unigen_amd.pipeline import pack_latents
    g = {c[0]: c for c in cases_of(40, 50)}
    _, img, _, _, want = g["g10_in_40x50"]
    out = deblurring_image(img)
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    gray_want = np.repeat(want[..., :1], 3, -1)                                       # .convert("RGB") of a gray image, blurred
    assert np.array_equal(deblurring_image(np.ascontiguousarray(img[..., 0])), gray_want)
    out = deblurring_image(torch.from_numpy(img[..., :1].copy()).to(gpu))
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), gray_want)
    pipe = tiny_pipe()
    raw = synth(1, 35, 34, 3, seed=31)[0]                                             # preprocess rounds to 32 x 32, as in test_condition_encode
    blurred = deblurring_image(raw)
    assert np.array_equal(blurred, ref_blur(raw[None], "gaussian", 10)[0])
    cond = Condition("deblurring", raw_img=blurred, no_process=True)
    assert cond.type_id == 7 and np.array_equal(cond.condition, blurred)
    gen = lambda: torch.Generator(device=gpu).manual_seed(5)
    tokens, ids, type_id = cond.encode(pipe, generator=gen())
    C = pipe.vae.config.latent_channels
    assert tuple(tokens.shape) == (1, 64, 4 * C) and tuple(ids.shape) == (64, 3) and tuple(type_id.shape) == (64, 1) and bool((type_id == 7).all())
    z = pipe.vae.encode_scaled(pipe.image_processor.preprocess(blurred).to(torch.bfloat16), generator=gen())
    assert torch.equal(tokens, pack_latents(z.contiguous()))


def test_bad_arguments_raise(gpu):
    import ctypes as C
    from unigen_amd import lib as L
    from unigen_amd import ops
    from unigen_amd.image import gaussian_blur
    H, W = 12, 16
    x = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=gpu)
    out = torch.empty_like(x)
    lib = L.load()
    need = int(lib.ug_img_blur_workspace_bytes(1, H, W, 3))
    assert need >= 2 * H * W * 3 and int(lib.ug_img_blur_workspace_bytes(1, 0, W, 3)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    good = dict(src=x.data_ptr(), dst=out.data_ptr(), C=3, cx=(9, 840963, 399459), cy=(9, 840963, 399459), passes=3, fuse=1, ws_bytes=need)

    def call(**kw):
        a = {**good, **kw}
        return lib.ug_img_box_blur_u8(a["src"], H * W * a["C"], W * a["C"], 1, H, W, a["C"], a["dst"], H * W * a["C"], W * a["C"], *a["cx"], *a["cy"], a["passes"],
                                      a["fuse"], ws.data_ptr(), a["ws_bytes"], torch.cuda.current_stream().cuda_stream)

    assert call() == L.UG_OK
    for kw in (dict(C=2), dict(C=4), dict(passes=0), dict(passes=-3), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(cx=(-1, 840963, 399459)),
               dict(cy=(-2, 0, 0)), dict(cx=(9, 1 << 24, 0)), dict(cy=(0, -1, 0)), dict(fuse=2), dict(dst=x.data_ptr())):
        with pytest.raises(L.UniGenHipError, match="ug_img_box_blur_u8"):
            L.check(call(**kw), "ug_img_box_blur_u8")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="channels"):
        ops.img_box_blur_u8(torch.zeros(1, H, W, 2, dtype=torch.uint8, device=gpu), (0, 1 << 23, 1 << 22), (0, 1 << 23, 1 << 22))
    with pytest.raises(L.UniGenHipError):
        ops.img_box_blur_u8(x.cpu(), (0, 1 << 23, 1 << 22), (0, 1 << 23, 1 << 22))
    with pytest.raises(TypeError):
        gaussian_blur(torch.zeros(H, W, 3), 2)                                        # blur on float images is out of scope
    with pytest.raises(ValueError, match="non-negative"):
        gaussian_blur(x, -2)
