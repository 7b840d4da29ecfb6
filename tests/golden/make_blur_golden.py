"""Writes tests/golden/blur_tiny.safetensors: seeded uint8 images and PIL's GaussianBlur / BoxBlur of them (needs Pillow; the tests need only the file).

    python tests/golden/make_blur_golden.py

  in_{H}x{W}            uint8 [H, W, 3]: tests/image_ref.py synth
  sha_bw_{H}x{W}        SHA-256 of tests/blur_ref.py bw_image(H, W), the seeded image of 0 / 255 bytes (integers of a seeded generator: rebuilt by the
                        tests, and checked against this digest, rather than stored)
  {filter}_{name}       PIL's image.filter(...) of the RGB input `name` (in_.. or bw_..); `filter` is a key of tests/blur_ref.py filters(H, W), e.g.
                        g10 = GaussianBlur(10), g10x0 = GaussianBlur((10, 0)), b9.475 = BoxBlur(9.475)
  pil_version           the Pillow release that wrote the file, as bytes
PIL filters every band on its own, so what it makes of channel 0 as an "L" image is channel 0 of the RGB result: main() asserts that for every case
and the file stores the RGB result alone (it stays under 512 KB that way); the "L" cases of the tests compare with that channel.
"""
import hashlib
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageFilter, __version__ as PIL_VERSION
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.blur_ref import SIZES, bw_image, filters  # noqa: E402
from tests.image_ref import synth  # noqa: E402


def pil_filter(arr, kind, radius):
    """arr uint8 [H, W, 3] or [H, W] -> PIL's filtered bytes"""
    f = ImageFilter.GaussianBlur(radius) if kind == "gaussian" else ImageFilter.BoxBlur(radius)
    return np.array(Image.fromarray(arr).filter(f))


def main():
    out = {}
    for i, (H, W) in enumerate(SIZES):
        img, bw = synth(1, H, W, 3, seed=300 + i)[0], bw_image(H, W)
        out[f"in_{H}x{W}"] = torch.from_numpy(img)
        out[f"sha_bw_{H}x{W}"] = torch.tensor(list(hashlib.sha256(bw.tobytes()).digest()), dtype=torch.uint8)
        for name, arr in ((f"in_{H}x{W}", img), (f"bw_{H}x{W}", bw)):
            for key, (kind, radius) in filters(H, W).items():
                rgb = pil_filter(arr, kind, radius)
                assert np.array_equal(pil_filter(np.ascontiguousarray(arr[..., 0]), kind, radius), rgb[..., 0]), (name, key)
                out[f"{key}_{name}"] = torch.from_numpy(rgb)
    out["pil_version"] = torch.tensor(list(PIL_VERSION.encode()), dtype=torch.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blur_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL_VERSION)
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
