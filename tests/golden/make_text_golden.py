"""Writes tests/golden/text_tiny.safetensors: the tiny T5 encoder and CLIP text model of tests/text_ref.py (weights, token ids) and the outputs of
the installed transformers library on them in float64, stored as fp32. Needs transformers; no download (random weights, HF_HUB_OFFLINE=1).

    python tests/golden/make_text_golden.py
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import text_ref as R  # noqa: E402


def hf_t5(cfg, sd):
    import transformers
    m = transformers.T5EncoderModel(transformers.T5Config(**cfg, dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)).eval()
    missing, unexpected = m.load_state_dict({**sd, "encoder.embed_tokens.weight": sd["shared.weight"]}, strict=False)
    assert not unexpected and all("embed_tokens" in k for k in missing), (missing, unexpected)
    return m.double()


def hf_clip(cfg, sd):
    import transformers
    m = transformers.CLIPTextModel(transformers.CLIPTextConfig(**cfg, attention_dropout=0.0, bos_token_id=1, pad_token_id=0)).eval()
    have = m.state_dict()
    pre = "text_model." if any(k.startswith("text_model.") for k in have) else ""
    missing, unexpected = m.load_state_dict({pre + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m.double()


def main():
    from safetensors.torch import save_file
    t5_ids, clip_ids = R.tiny_ids()
    out = {"t5.ids": t5_ids.to(torch.int32), "clip.ids": clip_ids.to(torch.int32)}
    st5, sclip = R.random_state(R.t5_keys(R.T5_TINY), 11), R.random_state(R.clip_keys(R.CLIP_TINY), 12)
    out.update({"t5.w." + k: v for k, v in st5.items()})
    out.update({"clip.w." + k: v for k, v in sclip.items()})
    with torch.no_grad():
        y = hf_t5(R.T5_TINY, R.decode_state(out, "t5.w."))(input_ids=t5_ids.long())[0]
        out["t5.out.last_hidden_state"] = y.float()
        c = hf_clip(R.CLIP_TINY, R.decode_state(out, "clip.w."))(input_ids=clip_ids.long(), output_hidden_states=True)
        out["clip.out.last_hidden_state"] = c.last_hidden_state.float()
        out["clip.out.pooler_output"] = c.pooler_output.float()
        out["clip.out.hidden_m2"] = c.hidden_states[-2].float()
    path = os.path.join(HERE, "text_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
