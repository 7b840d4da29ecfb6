"""`Condition` of the reference (src/condition.py) on this package's pipeline objects: the condition image is made by the HIP image front end
(unigen_amd/image.py) and encoded by the native VAE.

    Condition("canny", raw_img=img).encode(pipe) -> (tokens [B, N, 4C], ids [N, 3], type_id [N, 1])
    Condition("deblurring", raw_img=deblurring_image(img), no_process=True).encode(pipe)
    Condition("depth", raw_img=depth_image(img, model), no_process=True).encode(pipe)        model: unigen_amd.depth.DepthAnythingForDepthEstimation

`pipe` needs `image_processor` (unigen_amd.image.VaeImageProcessor) and `vae` (unigen_amd.vae.AutoencoderKL). Images are PIL images, uint8 ndarrays
or uint8 tensors [H, W, C]; a condition image comes back in the kind it went in as (PIL in, PIL out).
"""
from __future__ import annotations

from typing import Any, Optional, Tuple

import numpy as np
import torch

from . import image as I
from .pipeline import pack_latents, prepare_latent_image_ids

condition_dict = {
    "depth": 0,
    "canny": 1,
    "subject": 4,
    "coloring": 6,
    "deblurring": 7,
    "fill": 9,
}


def _like(src, arr: np.ndarray):
    """A uint8 [H, W, 3] result in the kind of `src`: PIL image, tensor (on its device) or ndarray."""
    if I._is_pil(src):
        from PIL import Image
        return Image.fromarray(arr)
    if isinstance(src, torch.Tensor):
        return torch.from_numpy(arr).to(src.device)
    return arr


def _rgb(img):
    """`img.convert("RGB")` for the three image kinds (a gray image is replicated)."""
    if I._is_pil(img):
        return img.convert("RGB")
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[-1] == 1:
        img = img.expand(*img.shape[:-1], 3) if isinstance(img, torch.Tensor) else np.repeat(img, 3, axis=-1)
    return img


def deblurring_image(raw_img):
    """The reference's "deblurring" condition image (src/condition.py:72-78), `raw_img.convert("RGB").filter(ImageFilter.GaussianBlur(10)).convert("RGB")`,
    in the kind of `raw_img` (PIL image, uint8 ndarray or tensor [H, W] / [H, W, C]); the blur runs in csrc/image.hip, bit for bit PIL's."""
    rgb = _rgb(raw_img)
    return I.gaussian_blur(rgb.contiguous() if isinstance(rgb, torch.Tensor) else rgb, 10)      # a replicated gray tensor is a stride-0 view


def depth_image(raw_img, model, processor=None):
    """The reference's "depth" condition image (src/condition.py:52-62), `depth_pipe(raw_img.convert("RGB"))["depth"].convert("RGB")`, in the kind of
    `raw_img`; `model` is a unigen_amd.depth.DepthAnythingForDepthEstimation, `processor` a DepthImageProcessor (default: depth-anything's settings).
    A GPU tensor stays on the GPU and nothing synchronises with the host."""
    from .depth import _estimate
    if not I._is_pil(raw_img) and raw_img.ndim not in (2, 3):
        raise ValueError(f"depth_image takes one image [H, W] or [H, W, C], got {tuple(raw_img.shape)}")
    _, u8 = _estimate(model, raw_img, processor, 3)                       # a gray image is replicated by the patch kernel: convert("RGB")
    out = u8[0]
    if I._is_pil(raw_img):
        from PIL import Image
        return Image.fromarray(out.cpu().numpy())
    if isinstance(raw_img, torch.Tensor):
        return out if raw_img.is_cuda else out.to(raw_img.device)
    return out.cpu().numpy()


class Condition(object):
    def __init__(self, condition_type: str, raw_img=None, no_process: bool = False, condition=None, condition_ids=None, mask=None) -> None:
        self.condition_type = condition_type
        assert raw_img is not None or condition is not None
        if raw_img is not None:
            self.condition = _rgb(raw_img) if no_process else self.get_condition(condition_type, raw_img)
            self.condition_ids = None
        else:
            self.condition = condition
            self.condition_ids = condition_ids
        assert mask is None, "Mask not supported yet"

    def get_condition(self, condition_type: str, raw_img):
        """Returns the condition image (src/condition.py:46-81)."""
        if condition_type == "depth":
            raise NotImplementedError("condition type 'depth' needs a depth-estimation model (the reference runs transformers' depth-anything pipeline); "
                                      "`depth_image` of this module runs one on the GPU (unigen_amd.depth) - pass Condition(\"depth\", "
                                      "raw_img=depth_image(img, model), no_process=True) (docs/NEXT_ROWS.md: why this branch still refuses)")
        if condition_type == "canny":
            src = np.array(raw_img) if I._is_pil(raw_img) else raw_img
            edges = I.canny(src, 100, 200)                                   # cv2.Canny(img, 100, 200)
            edges = edges.cpu().numpy() if isinstance(edges, torch.Tensor) else edges
            return _like(raw_img, np.repeat(edges[..., None], 3, axis=-1))   # .convert("RGB")
        if condition_type == "subject":
            return raw_img
        if condition_type == "coloring":
            from . import ops
            x = I.to_device_u8(_rgb(raw_img), raw_img.device if isinstance(raw_img, torch.Tensor) and raw_img.is_cuda else I._default_device())
            gray = ops.img_rgb_to_l(x)[0].cpu().numpy()                      # .convert("L").convert("RGB")
            return _like(raw_img, np.repeat(gray, 3, axis=-1))
        if condition_type == "deblurring":
            raise NotImplementedError("condition type 'deblurring' is PIL's GaussianBlur(10); `deblurring_image` of this module computes it on the GPU, "
                                      "bit for bit - pass Condition(\"deblurring\", raw_img=deblurring_image(img), no_process=True) "
                                      "(docs/NEXT_ROWS.md: why this branch still refuses)")
        if condition_type == "fill":
            return _rgb(raw_img)
        return self.condition

    @property
    def type_id(self) -> int:
        """Returns the type id of the condition."""
        return condition_dict[self.condition_type]

    def _encode_image(self, pipe, cond_img, generator: Optional[torch.Generator] = None) -> Tuple[Any, Any]:
        """Encodes an image condition into tokens using the pipeline (src/condition.py:90-111)."""
        if getattr(pipe, "image_processor", None) is None or getattr(pipe, "vae", None) is None:
            raise NotImplementedError("Condition.encode needs `pipe.image_processor` (unigen_amd.image.VaeImageProcessor) and `pipe.vae` "
                                      "(unigen_amd.vae.AutoencoderKL)")
        vae = pipe.vae
        x = pipe.image_processor.preprocess(cond_img)
        x = x.to(device=vae.device, dtype=vae.dtype)
        z = vae.encode_scaled(x, generator=generator)
        cond_tokens = pack_latents(z.contiguous())
        cond_ids = prepare_latent_image_ids(z.shape[2] // 2, z.shape[3] // 2, z.device, z.dtype)
        if self.condition_type == "subject":
            cond_ids[:, 2] += z.shape[2] // 2
        return cond_tokens, cond_ids

    def encode(self, pipe, generator: Optional[torch.Generator] = None) -> Tuple[Any, Any, torch.Tensor]:
        """Encodes the condition into tokens, ids and type_id."""
        if self.condition_ids is not None:
            tokens, ids = self.condition, self.condition_ids
        elif self.condition_type in condition_dict:
            tokens, ids = self._encode_image(pipe, self.condition, generator)
        else:
            raise NotImplementedError(
                "There are two ways to use it: \n"
                "(1) Give the condition tensor to the 'self.condition' and the condition_ids to the 'self.condition_ids' manually.\n"
                "(2) Give the raw_image to the 'self.raw_img' and process the rest operations with a pipeline automatically.\n")
        type_id = torch.ones_like(ids[:, :1]) * self.type_id     # the type_id is not used so far
        return tokens, ids, type_id
