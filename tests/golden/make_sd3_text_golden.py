"""Writes the fixtures of SD3's prompt encoding: the tiny models of tests/sd3_text_ref.py (weights, token ids) and the outputs of the installed
transformers library on them in float64, stored as fp32. Needs transformers; no download (random weights, HF_HUB_OFFLINE=1).

    tests/golden/sd3_text_tiny.safetensors      the two projected CLIPs (clip_a.*, clip_b.*): text_embeds, last_hidden_state, hidden_states[-2] and [-3]
    tests/golden/sd3_text_tiny_t5.safetensors   the 256-wide T5 encoder (t5.*): last_hidden_state
(two files: together the weights and the stored outputs pass the size limit of one committed file)

    python tests/golden/make_sd3_text_golden.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from tests import sd3_text_ref as S  # noqa: E402
from tests import text_ref as R  # noqa: E402

CLIP_FILE, T5_FILE = "sd3_text_tiny.safetensors", "sd3_text_tiny_t5.safetensors"
CLIP_OUTPUTS = ("text_embeds", "last_hidden_state", "hidden_m2", "hidden_m3")


def hf_clip_proj(cfg, sd):
    import transformers
    m = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**cfg, attention_dropout=0.0, bos_token_id=1, pad_token_id=0)).eval()
    have = m.state_dict()
    pre = "text_model." if any(k.startswith("text_model.") for k in have) else ""
    missing, unexpected = m.load_state_dict({(k if k.startswith("text_projection.") else pre + k): v for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m.double()


def hf_t5(cfg, sd):
    import transformers
    m = transformers.T5EncoderModel(transformers.T5Config(**cfg, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)).eval()
    missing, unexpected = m.load_state_dict({**sd, "encoder.embed_tokens.weight": sd["shared.weight"]}, strict=False)
    assert not unexpected and all("embed_tokens" in k for k in missing), (missing, unexpected)
    return m.double()


def tensors():
    """-> (the CLIP file's tensors, the T5 file's)"""
    ids_a, ids_b, ids_t5 = S.tiny_ids()
    clips = {"clip_a.ids": ids_a.to(torch.int32), "clip_b.ids": ids_b.to(torch.int32)}
    with torch.no_grad():
        for name, cfg, seed, ids in (("clip_a", S.CLIP_A, 31, ids_a), ("clip_b", S.CLIP_B, 32, ids_b)):
            clips.update({f"{name}.w." + k: v for k, v in R.random_state(S.clip_proj_keys(cfg), seed).items()})
            c = hf_clip_proj(cfg, R.decode_state(clips, f"{name}.w."))(input_ids=ids.long(), output_hidden_states=True)
            assert len(c.hidden_states) == cfg["num_hidden_layers"] + 1
            for key, t in zip(CLIP_OUTPUTS, (c.text_embeds, c.last_hidden_state, c.hidden_states[-2], c.hidden_states[-3])):
                clips[f"{name}.out.{key}"] = t.float()
        t5 = {"t5.ids": ids_t5.to(torch.int32)}
        t5.update({"t5.w." + k: v for k, v in R.random_state(R.t5_keys(S.T5_SD3), 33).items()})
        t5["t5.out.last_hidden_state"] = hf_t5(S.T5_SD3, R.decode_state(t5, "t5.w."))(input_ids=ids_t5.long())[0].float()
    return ({k: v.contiguous() for k, v in clips.items()}, {k: v.contiguous() for k, v in t5.items()})


def main():
    from safetensors.torch import save_file
    for name, out in zip((CLIP_FILE, T5_FILE), tensors()):
        path = os.path.join(HERE, name)
        save_file(out, path)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
