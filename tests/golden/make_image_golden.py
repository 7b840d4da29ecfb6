"""Writes tests/golden/image_tiny.safetensors: seeded synthetic uint8 images and what PIL makes of them (needs Pillow; the tests need only the file).

    python tests/golden/make_image_golden.py

  in_{H}x{W}            uint8 [H, W, 3]: smooth blobs + hard edges + noise (tests/image_ref.py synth); the one-channel cases use channel 0 of it
  in4_100x60            the same recipe quantised to 4 grey levels (plateaus)
  resize{C}_{H}x{W}_{h}x{w}   PIL Image.resize((w, h), LANCZOS) of the C-channel input
  l_{name}              PIL convert("L") of the input
  pil_version           the Pillow release that wrote the file, as bytes
"""
import os
import sys

import numpy as np
import torch
from PIL import Image, __version__ as PIL_VERSION
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.image_ref import synth  # noqa: E402

# (H, W) -> (h, w): down, up, odd sizes, one pass skipped each way, more than one workgroup along each axis
RESIZE_PAIRS = [((64, 48), (32, 32)), ((33, 47), (64, 80)), ((100, 60), (37, 23)), ((48, 48), (48, 96)), ((1024, 16), (512, 16)), ((16, 1024), (16, 512))]


def main():
    out = {}
    for i, ((H, W), (h, w)) in enumerate(RESIZE_PAIRS):
        img = synth(1, H, W, 3, seed=100 + i)[0]
        out[f"in_{H}x{W}"] = torch.from_numpy(img)
        out[f"resize3_{H}x{W}_{h}x{w}"] = torch.from_numpy(np.array(Image.fromarray(img).resize((w, h), Image.LANCZOS)))
        out[f"resize1_{H}x{W}_{h}x{w}"] = torch.from_numpy(np.array(Image.fromarray(img[..., 0], mode="L").resize((w, h), Image.LANCZOS)))
        out[f"l_in_{H}x{W}"] = torch.from_numpy(np.array(Image.fromarray(img).convert("L")))
    img4 = synth(1, 100, 60, 3, seed=7, levels=4)[0]
    out["in4_100x60"] = torch.from_numpy(img4)
    out["l_in4_100x60"] = torch.from_numpy(np.array(Image.fromarray(img4).convert("L")))
    out["resize3_in4_100x60_37x23"] = torch.from_numpy(np.array(Image.fromarray(img4).resize((23, 37), Image.LANCZOS)))
    out["pil_version"] = torch.tensor(list(PIL_VERSION.encode()), dtype=torch.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL_VERSION)


if __name__ == "__main__":
    main()
