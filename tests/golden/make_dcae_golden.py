"""Writes tests/golden/dcae_tiny.safetensors from tests/dcae_ref.py: inputs and float64 outputs of the tiny AutoencoderDC, and what pins its weights.

    python tests/golden/make_dcae_golden.py

Configuration "a" of tests/dcae_ref.py TINY (three stages ResBlock, EfficientViTBlock, EfficientViTBlock; widths 64, 128, 128; one layer each;
multiscales (), (5,), (); 8 latent channels; "Conv" / "interpolate"), 1.78 M parameters. At one byte per weight that is 1.7 MiB, above the size limit
for a committed file, so the weights are NOT stored: they come from the seeded integer generator of dcae_ref.tiny_quantised, as the second
configuration's do, and the fixture pins that generator instead:
  keys                                 the state-dict keys in order, newline-joined, as bytes
  fingerprint                          int64 [keys, 2]: the sum and the sum of squares of every tensor's 8-bit grid values
  run{r}.x, run{r}.z                   inputs of TINY_RUNS[r] (r = 0, 1): the image [2, 3, H, W] and latents of their own [2, 8, H / 4, W / 4], bf16
  run{r}.latent, run{r}.sample         float64 encode(x) [2, 8, H / 4, W / 4] and decode(z) [2, 3, H, W]
Configuration "b" is evaluated by the tests themselves. Configuration "w" (the published attention widths 512 and 1024, 66 M values) has one run, 24 x 40,
whose float64 evaluation takes longer than everything else tests/test_dcae_gpu.py does with it, so its float64 pair is stored as well:
  fingerprint.w                        as `fingerprint`, of configuration "w"
  run4.x, run4.z, run4.latent, run4.sample
"""
import os
import sys

import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import dcae_ref as R  # noqa: E402

RUNS = (0, 1, R.RUN_W)
LIMIT = 1 << 20                  # the repository's size limit for a committed file


def main():
    out = {"keys": torch.tensor(list("\n".join(R.tiny_quantised("a")).encode()), dtype=torch.uint8), "fingerprint": R.fingerprint("a"),
           "fingerprint.w": R.fingerprint("w")}
    for r in RUNS:
        assert R.TINY_RUNS[r][0] in ("a", "w")
        i = R.tiny_inputs(r)
        out[f"run{r}.x"], out[f"run{r}.z"] = i["x"], i["z"]
        out[f"run{r}.latent"], out[f"run{r}.sample"] = R.evaluate(r)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dcae_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(os.path.dirname(path), "sana_tiny.safetensors")) < LIMIT


if __name__ == "__main__":
    main()
