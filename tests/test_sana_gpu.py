"""unigen_amd.sana on the GPU: SanaTransformerBlock and SanaTransformer2DModel against the plain-torch reference of tests/sana_ref.py and the committed
fixture tests/golden/sana_tiny.safetensors (weights, inputs and float64 outputs of configuration "a"; configuration "b" does not fit into a committed
file: same seeded weights, float64 reference evaluated here).

Bounds (docs/PARITY_TOLERANCES.md, "Sana kernels and block"; those of tests/test_vae_gpu.py for whole-model paths): the fp32 path within rel-L2 1e-3
of the float64 reference; the bf16 path no further from it than 1.25 x the reference's own bf16 evaluation (e_hip <= 1.25 e_ref)."""
import os

import pytest
import torch

from tests import sana_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
F32_BOUND, RATIO = 1e-3, 1.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sana_tiny.safetensors")
BLOCK_KW = ("num_attention_heads", "attention_head_dim", "num_cross_attention_heads", "cross_attention_head_dim", "cross_attention_dim", "attention_bias",
            "norm_eps", "mlp_ratio")

_CACHE = {}


def _golden():
    if "golden" not in _CACHE:
        from safetensors.torch import load_file
        _CACHE["golden"] = load_file(GOLDEN)
    return _CACHE["golden"]


def _weights(name):
    """configuration "a": from the fixture; "b": the seeded generator"""
    if name not in _CACHE:
        if name == "a":
            t = _golden()
            _CACHE[name] = {k[2:]: R.dequantise(k[2:], t[k], int(t["e." + k[2:]])) for k in t if k.startswith("q.")}
        else:
            _CACHE[name] = R.tiny_state_dict(name)
    return _CACHE[name]


def _reference(run):
    """-> dict(out, blk: float64 truths; out16, blk16: the reference's own bf16 evaluation), computed once per process"""
    key = ("ref", run)
    if key not in _CACHE:
        name, H, W, T, _ = R.TINY_RUNS[run]
        sd, i, b = _weights(name), R.tiny_inputs(run), R.block_inputs(run)
        with torch.no_grad():
            if name == "a":
                out, blk = _golden()[f"run{run}.out"], _golden()[f"blk{run}.out"]
            else:
                m = R.build_ref(name, sd, F64)
                out = m(i["x"].to(F64), i["enc"].to(F64), i["t"].to(F64), i["mask"])
                blk = m.transformer_blocks[0](b["h"].to(F64), None, b["enc"].to(F64), b["mask"], b["t"].to(F64), H, W)
            m = R.build_ref(name, sd, BF)
            out16 = m(i["x"], i["enc"], i["t"], i["mask"])
            blk16 = m.transformer_blocks[0](b["h"], None, b["enc"], b["mask"], b["t"], H, W)
        _CACHE[key] = dict(out=out, blk=blk, out16=out16, blk16=blk16)
    return _CACHE[key]


def _model(name, dtype, dev):
    from unigen_amd.sana import SanaTransformer2DModel
    m = SanaTransformer2DModel(R.TINY[name], device=dev, dtype=dtype)
    m.load_state_dict(_weights(name))
    return m


def _block(name, dtype, dev):
    from unigen_amd.sana import SanaTransformerBlock
    c = R.TINY[name]
    b = SanaTransformerBlock(c["num_attention_heads"] * 32, **{k: c[k] for k in BLOCK_KW}, device=dev, dtype=dtype)
    b.load_state_dict({k[len("transformer_blocks.0."):]: v for k, v in _weights(name).items() if k.startswith("transformer_blocks.0.")})
    return b


@pytest.mark.parametrize("run", range(len(R.TINY_RUNS)))
def test_block_against_the_reference(gpu, run):
    name, H, W, T, _ = R.TINY_RUNS[run]
    ref, b = _reference(run), R.block_inputs(run)
    mask = None if b["mask"] is None else b["mask"].to(gpu)
    got = {}
    for dtype in (F32, BF):
        blk = _block(name, dtype, gpu)
        args = (b["h"].to(gpu, dtype), None, b["enc"].to(gpu, dtype), mask, b["t"].to(gpu, dtype), H, W)
        got[dtype] = blk(*args)
        torch.cuda.synchronize()
        assert torch.equal(blk(*args), got[dtype]), "two forwards differ"
    e32 = rel_l2(got[F32], ref["blk"])
    e_hip, e_ref = rel_l2(got[BF], ref["blk"]), rel_l2(ref["blk16"], ref["blk"])
    print(f"block run {run} ({name}, {H}x{W}, T={T}): fp32 {e32:.3e} (bound {F32_BOUND:.0e}); bf16 e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, ratio {e_hip / e_ref:.3f}")
    assert bool(torch.isfinite(got[BF]).all()) and e32 <= F32_BOUND, e32
    assert e_hip <= RATIO * e_ref, (e_hip, e_ref)


@pytest.mark.parametrize("run", range(len(R.TINY_RUNS)))
def test_model_against_the_reference(gpu, run):
    name, H, W, T, _ = R.TINY_RUNS[run]
    ref, i = _reference(run), R.tiny_inputs(run)
    mask = None if i["mask"] is None else i["mask"].to(gpu)
    got = {}
    for dtype in (F32, BF):
        m = _model(name, dtype, gpu)
        args = (i["x"].to(gpu, dtype), i["enc"].to(gpu, dtype), i["t"].to(gpu), mask)
        got[dtype] = m(*args)
        torch.cuda.synchronize()
        assert got[dtype].shape == ref["out"].shape and torch.equal(m(*args), got[dtype]), "shape, or two forwards differ"
    e32 = rel_l2(got[F32], ref["out"])
    e_hip, e_ref = rel_l2(got[BF], ref["out"]), rel_l2(ref["out16"], ref["out"])
    print(f"model run {run} ({name}, {H}x{W}, T={T}): fp32 {e32:.3e} (bound {F32_BOUND:.0e}); bf16 e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, ratio {e_hip / e_ref:.3f}")
    assert bool(torch.isfinite(got[BF]).all()) and e32 <= F32_BOUND, e32
    assert e_hip <= RATIO * e_ref, (e_hip, e_ref)


def test_all_ones_mask_is_no_mask(gpu):
    run = 0
    name, H, W, T, _ = R.TINY_RUNS[run]
    i = R.tiny_inputs(run)
    m = _model(name, BF, gpu)
    args = (i["x"].to(gpu), i["enc"].to(gpu), i["t"].to(gpu))
    assert torch.equal(m(*args), m(*args, encoder_attention_mask=torch.ones(2, T, dtype=torch.int64, device=gpu)))


def test_a_fresh_mask_per_call_is_read_every_time(gpu):
    """one new mask per prompt, each freed before the next is built (so that the allocator may hand out the same address): the result is that of a
    mask that is kept alive"""
    run = 1
    name, H, W, T, _ = R.TINY_RUNS[run]
    i = R.tiny_inputs(run)
    m = _model(name, BF, gpu)
    args = (i["x"].to(gpu), i["enc"].to(gpu), i["t"].to(gpu))
    lengths = [(12, 1), (3, 12), (12, 12), (1, 5)]
    kept = [(torch.arange(T)[None, :] < torch.tensor(n)[:, None]).to(torch.int64) for n in lengths]
    want = [m(*args, encoder_attention_mask=k).clone() for k in kept]
    assert not torch.equal(want[0], want[1]) and torch.equal(want[2], m(*args))
    for where in ("cpu", gpu):
        for n, w in zip(lengths, want):
            fresh = (torch.arange(T)[None, :] < torch.tensor(n)[:, None]).to(torch.int64).to(where)
            assert torch.equal(m(*args, encoder_attention_mask=fresh), w), (where, n)
            del fresh


def test_state_dict_round_trip_is_bit_exact(gpu):
    from unigen_amd.sana import SanaTransformer2DModel
    m = _model("a", BF, gpu)
    sd = m.state_dict()
    assert set(sd) == set(_weights("a")) and all(torch.equal(sd[k].cpu(), v) for k, v in _weights("a").items())
    m2 = SanaTransformer2DModel(R.TINY["a"], device=gpu, dtype=BF)
    m2.load_state_dict(sd)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    i = R.tiny_inputs(1)
    args = (i["x"].to(gpu), i["enc"].to(gpu), i["t"].to(gpu), i["mask"].to(gpu))
    assert torch.equal(m(*args), m2(*args))
    blk = _block("a", BF, gpu)
    assert all(torch.equal(v, sd["transformer_blocks.0." + k]) for k, v in blk.state_dict().items())
    with pytest.raises(KeyError, match="missing"):
        m2.load_state_dict({k: v for k, v in sd.items() if k != "caption_norm.weight"})


def test_refusals(gpu):
    from unigen_amd.sana import SanaTransformer2DModel, SanaTransformerBlock
    kw = dict(dim=128, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2, cross_attention_head_dim=48, cross_attention_dim=128)
    with pytest.raises(NotImplementedError, match="qk_norm.*follow-up"):
        SanaTransformerBlock(**kw, qk_norm="rms_norm_across_heads")
    with pytest.raises(NotImplementedError, match="dropout.*follow-up"):
        SanaTransformerBlock(**kw, dropout=0.1)
    with pytest.raises(NotImplementedError, match="head width 32"):
        SanaTransformerBlock(**dict(kw, num_attention_heads=2, attention_head_dim=64))
    with pytest.raises(NotImplementedError, match="guidance_embeds.*follow-up"):
        SanaTransformer2DModel(dict(R.TINY["a"], guidance_embeds=True))
    with pytest.raises(NotImplementedError, match="use_rope.*follow-up"):
        SanaTransformer2DModel(dict(R.TINY["a"], use_rope=True))
    run = 1
    name, H, W, T, _ = R.TINY_RUNS[run]
    b, blk = R.block_inputs(run), _block(name, BF, gpu)
    h, enc, t = b["h"].to(gpu), b["enc"].to(gpu), b["t"].to(gpu)
    with pytest.raises(NotImplementedError, match="attention_mask.*follow-up"):
        blk(h, torch.ones(2, H * W, device=gpu), enc, None, t, H, W)
    holes = torch.ones(2, T, dtype=torch.int64)
    holes[0, 3] = 0
    with pytest.raises(NotImplementedError, match="prefix.*follow-up"):
        blk(h, None, enc, holes, t, H, W)
    with pytest.raises(NotImplementedError, match="follow-up"):
        blk(h, None, enc, torch.zeros(2, 1, T), t, H, W)
    with pytest.raises(RuntimeError, match="inference only"):
        blk(h.clone().requires_grad_(True), None, enc, None, t, H, W)
    with torch.no_grad():
        blk(h.clone().requires_grad_(True), None, enc, None, t, H, W)           # recording off: allowed
    m = _model(name, BF, gpu)
    i = R.tiny_inputs(run)
    with pytest.raises(NotImplementedError, match="attention_mask.*follow-up"):
        m(i["x"].to(gpu), i["enc"].to(gpu), i["t"].to(gpu), None, torch.ones(2, H * W, device=gpu))
    with pytest.raises(TypeError, match="bfloat16"):
        m(i["x"].to(gpu, F32), i["enc"].to(gpu), i["t"].to(gpu))


def test_sana_600m_widths_run_finite_and_deterministic(gpu):
    """dim 1152 (36 heads of 32), 16 cross heads of 72 packed into 128-wide slots, mlp_ratio 2.5 (C = 2880), 2 layers, 32 x 32 tokens, 300 text tokens"""
    from unigen_amd.sana import SanaTransformer2DModel
    cfg = dict(in_channels=32, out_channels=32, num_attention_heads=36, attention_head_dim=32, num_layers=2, num_cross_attention_heads=16,
               cross_attention_head_dim=72, cross_attention_dim=1152, caption_channels=2304, mlp_ratio=2.5, attention_bias=False, sample_size=32, patch_size=1,
               norm_eps=1e-6, interpolation_scale=None)
    m = SanaTransformer2DModel(cfg, device=gpu, dtype=BF).init_synthetic_(3)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 32, 32, 32, generator=g).to(gpu, BF)
    enc = torch.randn(1, 300, 2304, generator=g).to(gpu, BF)
    t = torch.tensor([500.0], device=gpu)
    mask = (torch.arange(300)[None] < 77).to(torch.int64)
    a = m(x, enc, t, mask)
    torch.cuda.synchronize()
    assert a.shape == (1, 32, 32, 32) and bool(torch.isfinite(a).all()) and float(a.float().std()) > 0
    assert torch.equal(m(x, enc, t, mask), a)
    assert not torch.equal(m(x, enc, t), a), "the prefix mask must matter"
