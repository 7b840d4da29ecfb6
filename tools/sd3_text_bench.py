"""Time one SD3.5 prompt encode at the real geometries with random weights: CLIP-L (12 layers, 768 wide), OpenCLIP bigG (32 layers, 1280 wide, 20 heads,
erf GELU) and T5-XXL (24 layers, d_model 4096), 8 prompts plus 8 negatives (two calls of B = 8 per encoder, as encode_prompt_sd3 makes them), 77 / 77 /
256 tokens. Prints one JSON line per encoder (HIP events over `--iters` encodes after `--warmup`) and one for the whole encode_prompt_sd3 call.

    python tools/sd3_text_bench.py [--iters 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from text_bench import CLIP_L, T5_XXL, fill, timed  # noqa: E402
from unigen_amd.text import CLIPTextModelWithProjection, T5EncoderModel, encode_prompt_sd3  # noqa: E402

CLIP_L_PROJ = dict(CLIP_L, projection_dim=768)
CLIP_G = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, max_position_embeddings=77,
              hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2, projection_dim=1280)
B = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    encoders, ids, neg = [], [], []
    for name, cls, cfg, Lq in (("clip_l", CLIPTextModelWithProjection, CLIP_L_PROJ, 77), ("clip_g", CLIPTextModelWithProjection, CLIP_G, 77),
                               ("t5_xxl", T5EncoderModel, T5_XXL, 256)):
        model = cls.from_config(cfg, device=dev, dtype=torch.bfloat16)
        fill(model, 1)
        pos, ng = (torch.randint(3, 1000, (B, Lq), device=dev) for _ in range(2))
        if name != "t5_xxl":
            pos[:, -1] = ng[:, -1] = 49407
        kw = dict(output_hidden_states=True) if name != "t5_xxl" else {}
        ms = timed(lambda: (model(pos, **kw), model(ng, **kw)), a.iters, a.warmup)
        print(json.dumps(dict(case=name, B=f"{B}+{B}", L=Lq, ms_per_encode=round(ms, 3))), flush=True)
        encoders.append(model); ids.append(pos); neg.append(ng)
    ms = timed(lambda: encode_prompt_sd3(encoders, [None] * 3, None, max_sequence_length=256, device=dev, text_input_ids_list=ids, negative_text_input_ids_list=neg),
               a.iters, a.warmup)
    print(json.dumps(dict(case="encode_prompt_sd3", B=f"{B}+{B}", L="77/77/256", ms_per_encode=round(ms, 3))), flush=True)


if __name__ == "__main__":
    main()
