"""CPU checks of tests/blur_ref.py, the numpy restatement of PIL's BoxBlur / GaussianBlur that tests/test_blur_gpu.py compares the blur kernels with,
and of the host constants of unigen_amd/image.py (box_blur_constants, gaussian_box_radius). Every comparison is equality, no element is exempt.

The two forms of the reference (the clamped window the kernels compute, PIL's running accumulator) must agree with each other, with PIL's bytes in
tests/golden/blur_tiny.safetensors and, where Pillow is installed, with PIL itself. The constants always come from unigen_amd/image.py, so the float32
rounding points of the radius formula are pinned here as well: on a grid of 400 radii per filter no radius differs from PIL.
"""
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import blur_ref as R
from tests.image_ref import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blur_tiny.safetensors")


@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return {k: v.numpy() for k, v in load_file(GOLDEN).items()}


def consts_of(kind, radius):
    """-> (((rx, wwx, fwx), (ry, wwy, fwy)), passes) as unigen_amd/image.py hands them to the kernels."""
    from unigen_amd.image import _xy, box_blur_constants, gaussian_box_radius
    rx, ry = _xy(radius)
    if kind == "gaussian":
        return (box_blur_constants(gaussian_box_radius(rx)), box_blur_constants(gaussian_box_radius(ry))), 3
    return (box_blur_constants(rx), box_blur_constants(ry)), 1


def ref_blur(img, kind, radius, line=R.line_window):
    """The reference on img uint8 [B, H, W, C]; the constants of radius 0 skip their axis, as PIL does."""
    consts, passes = consts_of(kind, radius)
    return R.box_blur(img, tuple(None if c == (0, 1 << 24, 0) else c for c in consts), passes, line)


def fixture_cases():
    """(id, input [H, W, 3], kind, radius, PIL's bytes [H, W, 3]) of every stored output."""
    g = golden()
    for H, W in R.SIZES:
        bw = R.bw_image(H, W)
        assert hashlib.sha256(bw.tobytes()).digest() == g[f"sha_bw_{H}x{W}"].tobytes(), "the seeded 0 / 255 image is not the one the fixture was made from"
        for name, img in ((f"in_{H}x{W}", g[f"in_{H}x{W}"]), (f"bw_{H}x{W}", bw)):
            for key, (kind, radius) in R.filters(H, W).items():
                yield f"{key}_{name}", img, kind, radius, g[f"{key}_{name}"]


def test_fixture_is_complete():
    cases = list(fixture_cases())
    assert len(cases) == 2 * (len(R.SIZES) + 10 * len(R.MORE_ON)) and len(golden()) == len(cases) + 2 * len(R.SIZES) + 1
    assert bytes(golden()["pil_version"]).decode().split(".")[0].isdigit()
    for _, img, _, _, want in cases:
        assert want.shape == img.shape and want.dtype == np.uint8
    assert all(set(np.unique(R.bw_image(H, W))) <= {0, 255} for H, W in R.SIZES)
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_both_forms_equal_the_fixture():
    """RGB, and channel 0 alone as PIL's mode "L" (PIL filters each band on its own: the maker asserts that the "L" result is channel 0 of the RGB one)."""
    for cid, img, kind, radius, want in fixture_cases():
        for line in (R.line_window, R.line_running):
            assert np.array_equal(ref_blur(img[None], kind, radius, line)[0], want), (cid, line.__name__)
            assert np.array_equal(ref_blur(img[None, :, :, :1], kind, radius, line)[0, :, :, 0], want[..., 0]), (cid, "L", line.__name__)


def _pil(arr, kind, radius):
    from PIL import Image, ImageFilter
    f = ImageFilter.GaussianBlur(radius) if kind == "gaussian" else ImageFilter.BoxBlur(radius)
    return np.array(Image.fromarray(arr).filter(f))


def test_both_forms_equal_live_pil():
    pytest.importorskip("PIL.ImageFilter")
    for cid, img, kind, radius, want in fixture_cases():
        assert np.array_equal(_pil(img, kind, radius), want), cid                    # the installed Pillow still makes the fixture's bytes
        gray = np.ascontiguousarray(img[..., 0])
        for line in (R.line_window, R.line_running):
            assert np.array_equal(ref_blur(img[None], kind, radius, line)[0], _pil(img, kind, radius)), (cid, line.__name__)
            assert np.array_equal(ref_blur(gray[None, :, :, None], kind, radius, line)[0, :, :, 0], _pil(gray, kind, radius)), (cid, "L", line.__name__)


def test_constants():
    from unigen_amd.image import box_blur_constants, gaussian_box_radius
    R10 = gaussian_box_radius(10)
    assert R10.dtype == np.float32 and abs(float(R10) - 9.475) < 2e-6              # within two float32 steps (9.5e-7 each) of 9.475
    assert box_blur_constants(R10) == (9, 840963, 399459)
    assert box_blur_constants(0) == (0, 1 << 24, 0) and box_blur_constants(gaussian_box_radius(0)) == (0, 1 << 24, 0)      # radius 0: the identity, skipped
    assert box_blur_constants(0.5) == (0, 1 << 23, 1 << 22)
    for k in range(0, 4000, 7):                                                      # the weights of a pass never sum to more than 2^24
        r, ww, fw = box_blur_constants(k / 10)
        assert r == int(np.float32(k / 10)) and ww >= 0 and fw >= 0 and (2 * r + 1) * ww + 2 * fw <= 1 << 24
    for bad in (-1, float("nan"), 1 << 24):
        with pytest.raises(ValueError):
            box_blur_constants(bad)


def test_radius_grid_against_live_pil():
    """image.py's own constants through the reference on 400 radii per filter: BoxBlur all equal; GaussianBlur may differ on at most 2 radii, none of
    them an integer radius - with every assignment of _gaussian_blur_radius rounded to float32 as in C, none differs."""
    pytest.importorskip("PIL.ImageFilter")
    img = synth(1, 24, 31, 3, seed=5)
    box_bad = [k / 10 for k in range(1, 401) if not np.array_equal(ref_blur(img, "box", k / 10)[0], _pil(img[0], "box", k / 10))]
    assert box_bad == []
    gauss_bad = [k / 10 for k in range(1, 401) if not np.array_equal(ref_blur(img, "gaussian", k / 10)[0], _pil(img[0], "gaussian", k / 10))]
    print("GaussianBlur radii that differ from PIL:", gauss_bad)
    assert len(gauss_bad) <= 2 and not any(float(v).is_integer() for v in gauss_bad)
    assert gauss_bad == []                                                           # docs/PARITY_TOLERANCES.md lists none


def test_host_refusals_need_no_gpu():
    from unigen_amd.image import VaeImageProcessor, box_blur, gaussian_blur
    assert callable(VaeImageProcessor.blur)
    img = np.zeros((4, 4, 3), np.uint8)
    for fn in (box_blur, gaussian_blur):
        with pytest.raises(ValueError, match="non-negative"):
            fn(img, -1)
        with pytest.raises(ValueError, match="non-negative"):
            fn(img, (2, -3))
    import src.condition as S
    from unigen_amd.condition import Condition, deblurring_image
    assert S.deblurring_image is deblurring_image
    with pytest.raises(NotImplementedError, match=r"GaussianBlur\(10\).*deblurring_image\(img\), no_process=True"):
        Condition("deblurring", raw_img=img)
