"""Writes tests/golden/sana_tiny.safetensors from tests/sana_ref.py: weights, inputs and float64 outputs of the tiny Sana block and model.

    python tests/golden/make_sana_golden.py

Configuration "a" of tests/sana_ref.py TINY (dim 128: 4 heads of 32, cross heads of 48, 2 layers, caption_channels 64), 668 k parameters:
  q.<key>, e.<key>      the state dict on its 8-bit grid: int8 values and the exponent (int32 scalar); weight = q * 2^e (sana_ref.dequantise), exact in
                        bf16 - one byte per weight keeps the file under the size limit for a committed file
  run{r}.x / enc / t / mask                       inputs of TINY_RUNS[r] (r = 0, 1: the runs of configuration "a"; mask only with a prefix mask)
  run{r}.out                                      float64 model output [2, 8, H, W]
  blk{r}.h / enc / t                              inputs of block 0 alone (hidden [2, N, 128], text [2, T, 128], timestep [2, 768]; the run's mask)
  blk{r}.out                                      float64 block output [2, N, 128]
Configuration "b" (dim 320, 3.9 M parameters) does not fit: its weights come from the same seeded integer generator and the tests evaluate the
float64 reference themselves.
"""
import os
import sys

import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import sana_ref as R  # noqa: E402

F64 = torch.float64
RUNS = (0, 1)


def evaluate(run, sd=None):
    """-> (model output, block-0 output) of a run in float64"""
    name, H, W, T, _ = R.TINY_RUNS[run]
    sd = sd if sd is not None else R.tiny_state_dict(name)
    with torch.no_grad():
        m = R.build_ref(name, sd, F64)
        i = R.tiny_inputs(run)
        out = m(i["x"].to(F64), i["enc"].to(F64), i["t"].to(F64), i["mask"])
        b = R.block_inputs(run)
        blk = m.transformer_blocks[0](b["h"].to(F64), None, b["enc"].to(F64), b["mask"], b["t"].to(F64), H, W)
    return out, blk


def main():
    out = {}
    for k, (q, e) in R.tiny_quantised("a").items():
        out["q." + k], out["e." + k] = q, torch.tensor(e, dtype=torch.int32)
    for r in RUNS:
        assert R.TINY_RUNS[r][0] == "a"
        i, b = R.tiny_inputs(r), R.block_inputs(r)
        for n in ("x", "enc", "t"):
            out[f"run{r}.{n}"] = i[n]
        if i["mask"] is not None:
            out[f"run{r}.mask"] = i["mask"]
        for n in ("h", "enc", "t"):
            out[f"blk{r}.{n}"] = b[n]
        out[f"run{r}.out"], out[f"blk{r}.out"] = evaluate(r)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sana_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
