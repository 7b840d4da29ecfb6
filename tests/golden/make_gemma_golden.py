"""Writes tests/golden/gemma_tiny.safetensors: token ids, masks and the outputs of the installed transformers' Gemma2Model (float64, eager attention,
stored as fp32) on the two tiny models of tests/gemma_ref.py. The 2.4 M weights of the two models do not fit a committed fixture; they are an exact
integer function of their names (gemma_ref.tiny_state), and the fixture records their float64 sums beside the outputs that pin them.
Needs transformers; no download (HF_HUB_OFFLINE=1).

    python tests/golden/make_gemma_golden.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from tests import gemma_ref as R  # noqa: E402


def main():
    from safetensors.torch import save_file
    ids, mask = R.tiny_inputs()
    out = {"ids": ids.to(torch.int32), "mask": mask.to(torch.int32)}
    with torch.no_grad():
        for tag, (cfg, std, seed) in R.TINY.items():
            sd = R.tiny_state(cfg, std, seed)
            out[f"{tag}.weight_sum"] = torch.stack([v.double().sum() for _, v in sorted(sd.items())]).sum().view(1)
            out[f"{tag}.out.mask"] = R.hf_model(cfg, sd)(input_ids=ids, attention_mask=mask)[0].float()
            out[f"{tag}.out.nomask"] = R.hf_model(cfg, sd)(input_ids=ids)[0].float()
            if tag == "b":          # the same weights without the cap, and with a window that hides nothing: what the cap and the window move
                out["b.out.nocap"] = R.hf_model(dict(cfg, attn_logit_softcapping=None), sd)(input_ids=ids, attention_mask=mask)[0].float()
                out["b.out.nowindow"] = R.hf_model(dict(cfg, sliding_window=4096), sd)(input_ids=ids, attention_mask=mask)[0].float()
    path = os.path.join(HERE, "gemma_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
