"""The grid of the attention regimes sweep: tests/test_fuzz_attention_gpu.py runs every case on the GPU, tests/test_attn_regimes_cpu.py checks on the
host what each case's regime promises. Shapes and scales only; the operands come from bwd_ref.attention_regime."""
import random

import torch

from tests.bwd_ref import REGIMES, attention_regime, regime_fits
from tests.test_fuzz_backward_gpu import LENGTHS

SWEEP_VARIANTS = ("dh128", "dh64_buf", "dh64_ptr")           # head width 128 | 64 with the buffer-form K / V DMAs | 64 with the pointer form
SWEEP_SCALES = ("dh^-0.5", 0.05, 0.25)
SWEEP_SEEDS = (0, 1)
SWEEP_LQ = (33, 100, 300)
SWEEP_LKV = tuple(n for n in LENGTHS if n > 64)              # the backward sweep's lengths with more than one key tile
SWEEP_CAP = 2_000_000                                         # B H Lq Lkv: the float64 reference of one case stays well under a second


def sweep_ids():
    return [f"{r}-{v}-s{si}-{seed}" for r in REGIMES for v in SWEEP_VARIANTS for si in range(len(SWEEP_SCALES)) for seed in SWEEP_SEEDS]


def sweep_spec(case_id):
    """shape and scale of one case of the regimes sweep (no data)"""
    regime, variant, si, seed = case_id.rsplit("-", 3)
    rng = random.Random(case_id)
    dh = 128 if variant == "dh128" else 64
    scale = SWEEP_SCALES[int(si[1:])]
    B, H = rng.choice([1, 2]), rng.choice([1, 2, 3])
    Lq = rng.choice([n for n in SWEEP_LQ if regime_fits(regime, n, max(LENGTHS))])
    Lkv = rng.choice([n for n in SWEEP_LKV if regime_fits(regime, Lq, n)])
    if B * H * Lq * Lkv > SWEEP_CAP:
        B = 1
    return dict(id=case_id, regime=regime, variant=variant, dh=dh, scale=dh ** -0.5 if scale == "dh^-0.5" else scale, seed=int(seed), B=B, H=H,
                Lq=Lq, Lkv=Lkv)


def sweep_data(spec):
    """the operands of a sweep case: attention_regime's dict"""
    g = torch.Generator().manual_seed(31000 + sweep_ids().index(spec["id"]))
    return attention_regime(g, spec["regime"], spec["dh"], spec["B"], spec["H"], spec["Lq"], spec["Lkv"], spec["scale"])
