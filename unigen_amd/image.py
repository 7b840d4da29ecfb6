"""Image front end on the HIP library: diffusers' VaeImageProcessor surface and cv2.Canny, neither package needed.

The reference passes PIL images to `pipe(control_image=...)`, saves `pipe(...).images` as PIL images (infer.py) and builds its canny condition with
`cv2.Canny(img, 100, 200)` (src/condition.py:63-67); every image goes through `VaeImageProcessor.preprocess` / `.postprocess`. Here an image is
uploaded once as uint8 and everything after that runs in csrc/image.hip: PIL's Lanczos resampler, convert("L"), the uint8 <-> [-1, 1] converters, the
three stages of Canny and PIL's BoxBlur / GaussianBlur (the reference's "deblurring" condition, src/condition.py:72-78). All of it is integer or
exactly specified fp32 arithmetic (docs/PARITY_TOLERANCES.md, "Image front end: exact").

PIL is imported lazily: only PIL-typed inputs and `output_type="pil"` need it.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2          # PIL Resample.c: 8 bits of the pixel, 2 bits of head room for the sum of |coefficients|


def _is_pil(x) -> bool:
    return type(x).__module__.split(".")[0] == "PIL"


# ---- PIL's coefficient tables (Resample.c precompute_coeffs, normalize_coeffs_8bpc), float64 on the host as in C ---------------------------------
def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x: float) -> float:
    a = -0.5                                         # PIL's BICUBIC (torch's bicubic interpolation has a = -0.75)
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}      # name -> (kernel, support) of Resample.c


@lru_cache(maxsize=64)
def resample_tables(in_size: int, out_size: int, filter: str = "lanczos") -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (bounds int32 [out, 2] = (first input coordinate, taps), coef int32 [out, ksize] 22-bit fixed point, ksize) of one pass of PIL's
    "lanczos" (a = 3) or "bicubic" (a = -0.5) filter."""
    if filter not in _FILTERS:
        raise NotImplementedError(f"filter={filter!r}: one of {sorted(_FILTERS)}")
    kernel, support = _FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx, 0], bounds[xx, 1] = xmin, xmax
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coef[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)      # C's (int): round half away from zero
    return bounds, coef, ksize


_device_tables = {}


def _tables_on(device: torch.device, in_size: int, out_size: int, filter: str = "lanczos"):
    key = (str(device), in_size, out_size, filter)
    if key not in _device_tables:
        if len(_device_tables) >= 64:
            _device_tables.clear()
        b, c, k = resample_tables(in_size, out_size, filter)
        _device_tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), k)
    return _device_tables[key]


# ---- uint8 image batches ---------------------------------------------------------------------------------------------------------------------------
def _as_u8_batch(image) -> Union[np.ndarray, torch.Tensor]:
    """One image-like (PIL image, uint8 ndarray / tensor [H, W], [H, W, C] or [B, H, W, C]) -> [B, H, W, C] uint8, still on its side of the bus."""
    if _is_pil(image):
        if image.mode not in ("L", "RGB"):
            image = image.convert("RGB")
        image = np.array(image)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError(f"image arrays must be uint8 (got {image.dtype}); float images go in as [B, C, H, W] tensors")
    elif isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8:
            raise TypeError(f"image tensors must be uint8 [.., H, W, C] or float [B, C, H, W] (got {image.dtype})")
    else:
        raise TypeError(f"unsupported image type {type(image).__name__}: a PIL image, a uint8 ndarray / tensor or a list of these")
    if image.ndim == 2:
        image = image[None, :, :, None]
    elif image.ndim == 3:
        image = image[None]
    elif image.ndim != 4:
        raise ValueError(f"image must be [H, W], [H, W, C] or [B, H, W, C], got {tuple(image.shape)}")
    if image.shape[-1] not in (1, 3):
        raise ValueError(f"images have 1 or 3 channels in the last dimension, got {tuple(image.shape)}")
    return image


def to_device_u8(image, device) -> torch.Tensor:
    """Image-like or a list of them -> ONE uint8 [B, H, W, C] tensor on `device` (one host-to-device copy of the bytes)."""
    if isinstance(image, (list, tuple)):
        parts = [_as_u8_batch(im) for im in image]
        if not parts:
            raise ValueError("empty image list")
        if any(p.shape[1:] != parts[0].shape[1:] for p in parts):
            raise ValueError("images of one list must share height, width and channels")
        if all(isinstance(p, torch.Tensor) and p.is_cuda for p in parts):
            return torch.cat(parts, 0)
        image = np.concatenate([p.cpu().numpy() if isinstance(p, torch.Tensor) else p for p in parts], 0)
    else:
        image = _as_u8_batch(image)
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    return image.to(device)


def _default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def canny(image, low: int = 100, high: int = 200, return_sweeps: bool = False):
    """cv2.Canny(image, low, high): uint8 [H, W], [H, W, C] or [B, H, W, C] (C = 1 or 3) -> uint8 edge map [H, W] or [B, H, W], 255 on edges.
    A tensor comes back as a tensor on its device, an ndarray (or PIL image) as an ndarray."""
    from . import ops
    as_numpy = not isinstance(image, torch.Tensor)
    batched = getattr(image, "ndim", 3) == 4
    dev = image.device if isinstance(image, torch.Tensor) and image.is_cuda else _default_device()
    x = to_device_u8(image, dev)
    out, sweeps = ops.canny_u8(x, int(low), int(high))
    out = out if batched else out[0]
    out = out.cpu().numpy() if as_numpy else (out if image.is_cuda else out.cpu())
    return (out, sweeps) if return_sweeps else out


# ---- PIL's BoxBlur / GaussianBlur (BoxBlur.c): the constants of a pass, on the host with C's float roundings ---------------------------------------
_f32 = np.float32


def box_blur_constants(R) -> Tuple[int, int, int]:
    """(r, ww, fw) of one box-blur pass of float radius R: r = (int)R, ww = (uint32)(2^24 / (R * 2 + 1)) divided in float32, fw the weight of the
    two pixels just outside the window. A pass is (ww * window + fw * (in[x-r-1] + in[x+r+1]) + 2^23) >> 24."""
    R = _f32(R)
    if not 0 <= R < (1 << 24):                       # also refuses a NaN
        raise ValueError(f"blur radius must be in [0, 2^24), got {R}")
    r = int(R)
    ww = int(_f32(1 << 24) / (R * _f32(2) + _f32(1)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def gaussian_box_radius(radius, passes: int = 3) -> np.float32:
    """BoxBlur.c _gaussian_blur_radius: the float box radius whose `passes` repetitions approximate a Gaussian of standard deviation `radius`.
    Every variable is a C float, so every product, sum and quotient rounds to float32; only sqrt and floor see doubles (their literals are doubles)."""
    radius, one = _f32(radius), _f32(1)
    sigma2 = radius * radius / _f32(passes)
    L = _f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = _f32(math.floor((float(L) - 1.0) / 2.0))
    a = (_f32(2) * l + one) * (l * (l + one) - _f32(3) * sigma2)
    a = a / (_f32(6) * (sigma2 - (l + one) * (l + one)))
    return l + a


def _xy(radius) -> Tuple[float, float]:
    rx, ry = radius if isinstance(radius, (tuple, list)) else (radius, radius)
    if not (rx >= 0 and ry >= 0):
        raise ValueError(f"blur radius must be non-negative, got {radius!r}")
    return rx, ry


def _blur(image, Rx, Ry, passes: int):
    """`passes` box passes of float radius Rx along rows, then of Ry along columns; the result in the kind of `image`."""
    from . import ops
    pil, as_numpy = _is_pil(image), not isinstance(image, torch.Tensor)
    ndim = 3 if pil else image.ndim
    dev = image.device if isinstance(image, torch.Tensor) and image.is_cuda else _default_device()
    x = to_device_u8(image, dev)
    out = ops.img_box_blur_u8(x, box_blur_constants(Rx), box_blur_constants(Ry), passes)
    out = out if ndim == 4 else (out[0, :, :, 0] if ndim == 2 or (pil and x.shape[-1] == 1) else out[0])
    if pil:
        from PIL import Image
        return Image.fromarray(out.cpu().numpy())
    return out.cpu().numpy() if as_numpy else (out if image.is_cuda else out.cpu())


def box_blur(image, radius):
    """PIL's `image.filter(ImageFilter.BoxBlur(radius))`, bit for bit: uint8 [H, W], [H, W, C] or [B, H, W, C] (C = 1 or 3), a PIL image, ndarray or
    tensor, returned in the kind it came in (a GPU tensor stays on the GPU). `radius` is a number or an (x, y) pair."""
    rx, ry = _xy(radius)
    return _blur(image, rx, ry, 1)


def gaussian_blur(image, radius=2):
    """PIL's `image.filter(ImageFilter.GaussianBlur(radius))`, bit for bit: three box passes per axis of radius `gaussian_box_radius(radius)`.
    Image kinds and `radius` as for `box_blur`."""
    rx, ry = _xy(radius)
    return _blur(image, gaussian_box_radius(rx, 3), gaussian_box_radius(ry, 3), 3)


class VaeImageProcessor:
    """diffusers.image_processor.VaeImageProcessor for the pipelines of this package: same constructor names and defaults, `preprocess` and
    `postprocess`; the arithmetic runs in csrc/image.hip. Attach it like the text encoders:
        pipe.image_processor = VaeImageProcessor(vae_scale_factor=2 * pipe.vae_scale_factor)"""

    def __init__(self, do_resize: bool = True, vae_scale_factor: int = 8, vae_latent_channels: int = 4, resample: str = "lanczos", do_normalize: bool = True,
                 do_binarize: bool = False, do_convert_rgb: bool = False, do_convert_grayscale: bool = False, device=None):
        if resample != "lanczos":
            raise NotImplementedError(f"resample={resample!r}: only PIL's LANCZOS filter is implemented (docs/NEXT_ROWS.md)")
        if do_binarize:
            raise NotImplementedError("do_binarize is not implemented (no pipeline of this package uses it)")
        if do_convert_rgb and do_convert_grayscale:
            raise ValueError("`do_convert_rgb` and `do_convert_grayscale` can not both be set to `True`")
        if vae_scale_factor < 1:
            raise ValueError("vae_scale_factor must be >= 1")
        self.config = dict(do_resize=do_resize, vae_scale_factor=vae_scale_factor, vae_latent_channels=vae_latent_channels, resample=resample,
                           do_normalize=do_normalize, do_binarize=do_binarize, do_convert_rgb=do_convert_rgb, do_convert_grayscale=do_convert_grayscale)
        self.do_resize, self.vae_scale_factor, self.do_normalize = do_resize, int(vae_scale_factor), do_normalize
        self.do_convert_rgb, self.do_convert_grayscale = do_convert_rgb, do_convert_grayscale
        self.device = None if device is None else torch.device(device)

    @staticmethod
    def blur(image, blur_factor: int = 4):
        """diffusers' `image.filter(ImageFilter.GaussianBlur(blur_factor))`."""
        return gaussian_blur(image, blur_factor)

    # ---------------------------------------------------------------- sizes --------------------------------------------------------------------
    def get_default_height_width(self, image, height: Optional[int] = None, width: Optional[int] = None) -> Tuple[int, int]:
        """The image's own size unless given; in every case rounded DOWN to a multiple of vae_scale_factor."""
        if height is None or width is None:
            if _is_pil(image):
                h, w = image.height, image.width
            elif isinstance(image, torch.Tensor) and image.is_floating_point():
                h, w = image.shape[2], image.shape[3]                       # [B, C, H, W]
            else:
                h, w = (image.shape[0], image.shape[1]) if image.ndim in (2, 3) else (image.shape[1], image.shape[2])
            height = h if height is None else height
            width = w if width is None else width
        f = self.vae_scale_factor
        height, width = (int(height) // f) * f, (int(width) // f) * f
        if height < 1 or width < 1:
            raise ValueError(f"height and width must be at least vae_scale_factor = {f}")
        return height, width

    # ---------------------------------------------------------------- in ------------------------------------------------------------------------
    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        """-> fp32 [B, 3 or 1, H, W] on the GPU, in [-1, 1] (do_normalize) or [0, 1]."""
        from . import ops
        if isinstance(image, torch.Tensor) and image.is_floating_point():
            # diffusers passes a [B, C, H, W] float tensor through: no resize on this path here, normalised only when it looks like [0, 1] data
            if image.ndim == 3:
                image = image[None]
            if image.ndim != 4:
                raise ValueError(f"a float image tensor must be [B, C, H, W], got {tuple(image.shape)}")
            if self.do_normalize and float(image.min()) >= 0:
                image = 2.0 * image - 1.0
            return image
        first = image[0] if isinstance(image, (list, tuple)) and image else image
        dev = self.device or (first.device if isinstance(first, torch.Tensor) and first.is_cuda else _default_device())
        x = to_device_u8(image, dev)                                         # the one upload
        if self.do_convert_grayscale and x.shape[-1] == 3:
            x = ops.img_rgb_to_l(x)
        if self.do_resize:
            height, width = self.get_default_height_width(x, height, width)
            x = resize_u8(x, height, width)
        replicate = self.do_convert_rgb and x.shape[-1] == 1
        return ops.img_u8_to_chw(x, normalize=self.do_normalize, dtype=torch.float32, replicate=replicate)

    # ---------------------------------------------------------------- out -----------------------------------------------------------------------
    def postprocess(self, image: torch.Tensor, output_type: str = "pil", do_denormalize: Optional[List[bool]] = None):
        """"latent": untouched; "pt": the denormalised tensor; "np": float32 NHWC in [0, 1]; "pil": a list of PIL images; "u8" (ours): the uint8 NHWC
        tensor of the "pil" bytes, still on the GPU."""
        from . import ops
        if not isinstance(image, torch.Tensor):
            raise ValueError(f"Input for postprocessing is in incorrect format: {type(image)}. We only support pytorch tensor")
        if output_type not in ("latent", "pt", "np", "pil", "u8"):
            raise ValueError(f"output_type={output_type!r}: one of 'latent', 'pt', 'np', 'pil', 'u8'")
        if output_type == "latent":
            return image
        if do_denormalize is not None and not all(do_denormalize):
            raise NotImplementedError("per-image do_denormalize=False is not implemented")
        if output_type in ("pt", "np"):
            pt = (image * 0.5 + 0.5).clamp(0, 1) if self.do_normalize else image
            return pt if output_type == "pt" else pt.detach().cpu().permute(0, 2, 3, 1).float().numpy()
        u8 = ops.img_chw_to_u8(image, denormalize=self.do_normalize)
        if output_type == "u8":
            return u8
        from PIL import Image
        arr = u8.cpu().numpy()
        return [Image.fromarray(a[..., 0], mode="L") if a.shape[-1] == 1 else Image.fromarray(a) for a in arr]


def resize_u8(x: torch.Tensor, height: int, width: int, filter: str = "lanczos") -> torch.Tensor:
    """PIL's `Image.resize((width, height), LANCZOS)` (or BICUBIC with filter="bicubic") of a uint8 [B, H, W, C] GPU tensor, bit for bit."""
    from . import ops
    B, H, W, Cc = x.shape
    if (H, W) == (height, width):
        return x
    xt = _tables_on(x.device, W, width, filter) if W != width else None
    yt = _tables_on(x.device, H, height, filter) if H != height else None
    return ops.img_resize_u8(x, height, width, xt, yt)
