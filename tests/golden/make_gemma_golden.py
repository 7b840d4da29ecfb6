"""Writes tests/golden/gemma_tiny.safetensors: token ids, masks and the outputs of the installed transformers' Gemma2Model (float64, eager attention,
stored as fp32) on the two tiny models of tests/gemma_ref.py. The 2.4 M weights of the two models do not fit a committed fixture; they are an exact
integer function of their names (gemma_ref.tiny_state), and the fixture records their float64 sums beside the outputs that pin them.
Needs transformers; no download (HF_HUB_OFFLINE=1).

    python tests/golden/make_gemma_golden.py

With the argument `window` it writes tests/golden/gemma_tiny_window.safetensors instead and leaves the first file alone: the same for
gemma_ref.TINY_WINDOW (sliding window 40) on 100 tokens, the second sample with 37 live ones. There the padded rows 76 .. 99 of the second sample have
no live key in a sliding layer. The module in float64 turns them into NaN (its additive mask is -inf once the softmax casts it to fp32), and through
0 x NaN in P.V every row of that sample with them; rows 0 .. 75 depend on none of them (the mask is causal), so their truth is the module's output on
the first 76 tokens of that sample alone, and the fixture keeps NaN in rows 76 .. 99, where gemma_ref and the kernels define zero attention instead.

    python tests/golden/make_gemma_golden.py window
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


def window_outputs(cfg, sd, ids, mask):
    """-> (masked [2, L, hidden], unmasked) float64: the module's outputs on the window fixture's inputs, the second sample's masked rows as the header says"""
    dead = R.window_dead_rows(cfg, mask)
    assert not bool(dead[0].any()) and bool(dead[1].any())
    n = int((~dead[1]).sum())                                           # the rows before the first one without a live key
    assert not bool(dead[1, :n].any()) and bool(dead[1, n:].all())
    with torch.no_grad():
        m = R.hf_model(cfg, sd)
        full, nomask = m(input_ids=ids, attention_mask=mask)[0], m(input_ids=ids)[0]
        head = m(input_ids=ids[1:, :n], attention_mask=mask[1:, :n])[0]
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(head).all()) and bool(torch.isfinite(nomask).all())
    assert bool(torch.isnan(full[1, n:]).all()), "the module gives the rows without a live key a value now: compare them too"
    out = full.clone()
    out[1, :n] = head[0]
    return out, nomask


def main_window():
    from safetensors.torch import save_file
    cfg, std, seed = R.TINY_WINDOW
    ids, mask = R.window_inputs()
    sd = R.tiny_state(cfg, std, seed)
    masked, nomask = window_outputs(cfg, sd, ids, mask)
    out = {"ids": ids.to(torch.int32), "mask": mask.to(torch.int32), "c.out.mask": masked.float(), "c.out.nomask": nomask.float(),
           "c.weight_sum": torch.stack([v.double().sum() for _, v in sorted(sd.items())]).sum().view(1)}
    path = os.path.join(HERE, "gemma_tiny_window.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main_window() if sys.argv[1:] == ["window"] else main()
