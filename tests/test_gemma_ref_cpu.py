"""tests/gemma_ref.py against the installed transformers (live, float64) and against tests/golden/gemma_tiny.safetensors; the visibility of the cap and
the window in the fixture; the new ABI symbols; the host logic of unigen_amd/gemma.py that needs no GPU (refusals, key handling, default layer types,
encode_prompt_sana's index selection)."""
import os

import pytest
import torch

from tests import gemma_ref as R

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemma_tiny.safetensors")


@pytest.fixture(scope="module")
def golden():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


def FP32_OPS(layers: int) -> float:
    """What a float64 run of the module may differ from exact float64 by: Gemma2RMSNorm computes in fp32 whatever the model's dtype (`x.float()`), and
    eager_attention_forward takes its softmax in fp32; that is five fp32 tensors per layer and the final norm, 2^-23 relative each."""
    return (5 * layers + 1) * 2.0 ** -23


# ---- the reference against transformers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (None, 50.0, 4.0))
@pytest.mark.parametrize("window", (4096, 8))
@pytest.mark.parametrize("masked", (False, True))
def test_ref_matches_transformers_live(masked, window, cap):
    pytest.importorskip("transformers")
    cfg = dict(R.TINY_B, attn_logit_softcapping=cap, sliding_window=window, num_hidden_layers=2, layer_types=["sliding_attention", "full_attention"])
    sd = {k: v.double() for k, v in R.tiny_state(cfg, R.STD_B, 3).items()}
    ids, mask = R.tiny_inputs()
    mask = mask if masked else None
    with torch.no_grad():
        want = R.hf_model(cfg, sd)(input_ids=ids, attention_mask=mask)[0]
    got = R.model(sd, cfg, ids, mask)
    assert R.rel_l2(got, want) <= FP32_OPS(2), R.rel_l2(got, want)


def test_default_layer_types_are_the_library_s():
    transformers = pytest.importorskip("transformers")
    from unigen_amd.gemma import default_layer_types
    for n in (1, 4, 26):
        assert default_layer_types(n) == list(transformers.Gemma2Config(num_hidden_layers=n).layer_types) == R.layer_types(dict(num_hidden_layers=n))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("L", (1, 24, 300))
def test_rope_table_is_the_module_s_bit_for_bit(L, dtype):
    transformers = pytest.importorskip("transformers")
    from transformers.models.gemma2.modeling_gemma2 import Gemma2RotaryEmbedding
    from unigen_amd.gemma import rope_table
    conf = transformers.Gemma2Config(head_dim=256, hidden_size=128, num_attention_heads=2, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cos, sin = Gemma2RotaryEmbedding(conf)(torch.zeros(1, L, 128, dtype=dtype), torch.arange(L)[None])
    mine = rope_table(L, 256, 10000.0, dtype)
    ref = R.rope_table(L, 256, 10000.0)
    for want, a, b in ((cos, mine[0], ref[0]), (sin, mine[1], ref[1])):
        assert torch.equal(want[0, :, :128], want[0, :, 128:])          # the module's two halves are one table
        assert torch.equal(a, want[0, :, :128]) and torch.equal(b.to(dtype), want[0, :, :128])


def test_ref_matches_the_fixture(golden):
    ids, mask = R.tiny_inputs()
    assert torch.equal(golden["ids"].long(), ids) and torch.equal(golden["mask"].long(), mask)
    for tag, (cfg, std, seed) in R.TINY.items():
        sd = R.tiny_state(cfg, std, seed)
        total = torch.stack([v.double().sum() for _, v in sorted(sd.items())]).sum()
        assert float(total) == float(golden[f"{tag}.weight_sum"]), "the weights are not the ones the fixture was made with"
        for key, m in (("mask", mask), ("nomask", None)):
            e = R.rel_l2(R.model(sd, cfg, ids, m), golden[f"{tag}.out.{key}"])
            assert e <= FP32_OPS(cfg["num_hidden_layers"]) + 2.0 ** -24, (tag, key, e)          # the fixture stores the float64 outputs as fp32


def test_the_fixture_sees_the_cap_the_window_and_the_mask(golden):
    """Config B exists because a test that cannot see the cap or the window shows nothing: on the float64 truth each moves the output by more than
    10 x the bf16 bound of the model test (1.5 x the error of the bf16-rounded run). The mask moves the padded rows and no other."""
    cfg, std, seed = R.TINY["b"]
    ids, mask = R.tiny_inputs()
    truth = golden["b.out.mask"].double()
    bound = 1.5 * R.rel_l2(R.model(R.tiny_state(cfg, std, seed), cfg, ids, mask, R.bf), truth)
    cap, window = R.rel_l2(truth, golden["b.out.nocap"]), R.rel_l2(truth, golden["b.out.nowindow"])
    print(f"config B: bf16 bound {bound:.3e}; the cap moves the output by {cap:.3f}, the window by {window:.3f}")
    assert cap >= 10 * bound and window >= 10 * bound
    for tag in ("a", "b"):
        d = (golden[f"{tag}.out.mask"] - golden[f"{tag}.out.nomask"]).abs()
        assert float(d[0].max()) == 0 and float(d[1, :R.TINY_LIVE].max()) == 0 and float(d[1, R.TINY_LIVE:].max()) > 0.5


GOLDEN_WINDOW = os.path.join(os.path.dirname(GOLDEN), "gemma_tiny_window.safetensors")


def _window_case_errors(masked_want, nomask_want, storage: float):
    """gemma_ref against the module's outputs for TINY_WINDOW (sliding window 40, 100 tokens, the second sample with 37 live ones): every row with a
    live key in the sliding layers under the rule of the other fixture; the 24 rows without one are where the module (float64, eager) has NaN and
    the reference its defined zero attention - finite, and not compared against NaN."""
    cfg, std, seed = R.TINY_WINDOW
    sd = R.tiny_state(cfg, std, seed)
    ids, mask = R.window_inputs()
    dead = R.window_dead_rows(cfg, mask)
    assert dead.sum(1).tolist() == [0, R.WINDOW_L - R.WINDOW_LIVE - cfg["sliding_window"] + 1]
    assert torch.equal(torch.isnan(masked_want).any(-1), dead) and bool(torch.isfinite(nomask_want).all())
    got, got0 = R.model(sd, cfg, ids, mask), R.model(sd, cfg, ids, None)
    assert bool(torch.isfinite(got).all())
    bound = FP32_OPS(cfg["num_hidden_layers"]) + storage
    for b in range(R.WINDOW_B):                                         # each sample on its own: the short one must not hide behind the long one
        e = R.rel_l2(got[b][~dead[b]], masked_want[b][~dead[b]])
        print(f"TINY_WINDOW sample {b}: {int((~dead[b]).sum())} rows, rel-L2 {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (b, e)
    e0 = R.rel_l2(got0, nomask_want)
    assert e0 <= bound, e0
    assert float((got[1, :R.WINDOW_LIVE] - got0[1, :R.WINDOW_LIVE]).abs().max()) == 0 and float((got[1, R.WINDOW_LIVE:] - got0[1, R.WINDOW_LIVE:]).abs().max()) > 0.5
    return sd, cfg, ids, mask, got


def test_window_case_matches_transformers_live():
    pytest.importorskip("transformers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_gemma_golden", os.path.join(os.path.dirname(GOLDEN), "make_gemma_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cfg, std, seed = R.TINY_WINDOW
    ids, mask = R.window_inputs()
    masked, nomask = gen.window_outputs(cfg, {k: v.double() for k, v in R.tiny_state(cfg, std, seed).items()}, ids, mask)
    _window_case_errors(masked, nomask, 0.0)


def test_window_case_matches_the_fixture():
    from safetensors.torch import load_file
    g = load_file(GOLDEN_WINDOW)
    ids, mask = R.window_inputs()
    assert torch.equal(g["ids"].long(), ids) and torch.equal(g["mask"].long(), mask)
    sd, cfg, _, _, got = _window_case_errors(g["c.out.mask"].double(), g["c.out.nomask"].double(), 2.0 ** -24)
    total = torch.stack([v.double().sum() for _, v in sorted(sd.items())]).sum()
    assert float(total) == float(g["c.weight_sum"]), "the weights are not the ones the fixture was made with"
    # the window is visible: without it the float64 output moves by several times the bf16 bound of the model test (a model that ignored the
    # window would miss that bound by the same factor)
    bound = 1.5 * R.rel_l2(R.model(sd, cfg, ids, mask, R.bf), got)
    moved = R.rel_l2(R.model(sd, dict(cfg, sliding_window=4096), ids, mask), got)
    print(f"TINY_WINDOW: bf16 bound {bound:.3e}; the window moves the output by {moved:.3f}")
    assert moved >= 5 * bound


def test_attention_reference_properties():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 20, h, 16, generator=g, dtype=F64) for h in (4, 2, 2))
    full = R.attention(q, k, v, 0.25, 3.0, 0, None)
    assert torch.equal(R.attention(q, k, v, 0.25, 3.0, 20, [20, 20]), full)                  # a window of L and full lengths hide nothing
    rep = R.attention(q, k.repeat_interleave(2, 2), v.repeat_interleave(2, 2), 0.25, 3.0)      # grouped heads are repeated heads
    assert torch.equal(rep, full)
    assert torch.equal(R.attention(q, k, v, 0.25, 3.0, 4, [20, 7])[1, 12:], torch.zeros(8, 4, 16, dtype=F64))      # no live key: zeros
    rows = torch.tensor([0, 5, 19])
    assert torch.allclose(R.attention(q[:, rows], k, v, 0.25, 3.0, 4, [20, 7], qrows=rows), R.attention(q, k, v, 0.25, 3.0, 4, [20, 7])[:, rows], atol=1e-15)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols():
    from unigen_amd import lib
    names = ("ug_flash_attn_fwd_softcap", "ug_rope_half", "ug_gemma_rmsnorm_rows", "ug_gather_rows_scaled")
    cdll = lib.load()
    for n in names:
        assert n in lib.SIGNATURES and lib.F32_TWIN_OF[n] == n + "_f32" and lib.SIGNATURES[n] == lib.SIGNATURES[n + "_f32"]
        assert hasattr(cdll, n) and hasattr(cdll, n + "_f32")
    assert len(lib.SIGNATURES["ug_flash_attn_fwd_softcap"][1]) == 22


# ---- host logic -------------------------------------------------------------------------------------------------------------------
def test_config_refusals_name_the_field():
    from unigen_amd.gemma import Gemma2Model
    for field, value in (("head_dim", 128), ("hidden_activation", "gelu"), ("rope_parameters", {"rope_type": "linear", "factor": 2.0}),
                         ("attention_bias", True), ("use_bidirectional_attention", True)):
        with pytest.raises(NotImplementedError, match="rope_type" if field == "rope_parameters" else field):
            Gemma2Model(dict(R.TINY_A, **{field: value}))
    with pytest.raises(NotImplementedError, match="rope_type"):
        Gemma2Model(dict(R.TINY_A, rope_scaling={"type": "dynamic", "factor": 2.0}))
    with pytest.raises(ValueError, match="num_key_value_heads"):
        Gemma2Model(dict(R.TINY_A, num_attention_heads=3, num_key_value_heads=2))


def test_call_refusals():
    from unigen_amd.gemma import Gemma2Model
    m = Gemma2Model(dict(R.TINY_A, num_hidden_layers=1, layer_types=None))
    ids, mask = R.tiny_inputs()
    for kw in (dict(position_ids=torch.arange(24)[None]), dict(past_key_values=object()), dict(inputs_embeds=torch.zeros(2, 24, 128)),
               dict(cache_position=torch.arange(24)), dict(use_cache=True)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            m(ids, **kw)
    left, hole, empty, soft = mask.flip(1), mask.clone(), mask.clone(), mask.float() * 0.5
    hole[0, 5] = 0
    empty[1] = 0
    for bad, exc in ((left, NotImplementedError), (hole, NotImplementedError), (soft, NotImplementedError), (empty, ValueError), (mask[:, :5], ValueError)):
        with pytest.raises(exc, match="attention_mask"):
            m(ids, attention_mask=bad)
    with pytest.raises(Exception, match="HIP device only"):          # a good call on a CPU model gets as far as the device check
        m(ids, attention_mask=mask)


def test_prefix_lengths():
    from unigen_amd.gemma import prefix_lengths
    _, mask = R.tiny_inputs()
    n = prefix_lengths(mask, 2, 24)
    assert n.dtype == torch.int32 and n.tolist() == [24, 17]
    assert prefix_lengths(mask.bool(), 2, 24).tolist() == [24, 17]


def test_config_fields_and_keys():
    from unigen_amd.gemma import Gemma2Model
    m = Gemma2Model(dict(R.TINY_B, layer_types=None, rope_parameters={"rope_type": "default", "rope_theta": 5000.0}, attn_logit_softcapping=None))
    assert m.config["layer_types"] == ["sliding_attention", "full_attention"] * 2 and m.config["rope_theta"] == 5000.0
    assert Gemma2Model(dict(R.TINY_B, rope_theta=777.0)).config["rope_theta"] == 777.0 and Gemma2Model(R.TINY_B).config["rope_theta"] == 10000.0
    assert set(m.state_dict()) == set(R.keys(R.TINY_B))
    cfg, std, seed = R.TINY["b"]
    sd = R.tiny_state(cfg, std, seed)
    m.load_state_dict(sd)
    m2 = Gemma2Model(cfg)
    m2.load_state_dict({**{"model." + k: v for k, v in sd.items()}, "lm_head.weight": sd["embed_tokens.weight"]})          # the causal-LM checkpoint
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]) and torch.equal(v.float(), sd[k]), k
    H, KV, dh = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    qkv = m.layers[1]["qkv"]
    assert tuple(qkv.shape) == ((H + 2 * KV) * dh, 128) and torch.equal(qkv[H * dh:(H + KV) * dh].float(), sd["layers.1.self_attn.k_proj.weight"])
    assert torch.equal(m.layers[2]["gate_up"][256:].float(), sd["layers.2.mlp.up_proj.weight"])
    with pytest.raises(KeyError):
        m2.load_state_dict({**sd, "layers.0.self_attn.q_norm.weight": torch.zeros(256)})
    with pytest.raises(KeyError):
        m2.load_state_dict({k: v for k, v in sd.items() if k != "norm.weight"})


def test_from_pretrained_reads_a_local_directory(tmp_path):
    import json
    from safetensors.torch import save_file
    from unigen_amd.gemma import Gemma2Model
    cfg, std, seed = R.TINY["a"]
    sd = R.tiny_state(cfg, std, seed)
    os.makedirs(tmp_path / "text_encoder")
    with open(tmp_path / "text_encoder" / "config.json", "w") as f:
        json.dump(dict(cfg, architectures=["Gemma2Model"], model_type="gemma2", torch_dtype="bfloat16"), f)
    save_file({k: v.to(torch.bfloat16) for k, v in sd.items()}, str(tmp_path / "text_encoder" / "model.safetensors"))
    m = Gemma2Model.from_pretrained(str(tmp_path), subfolder="text_encoder")
    assert m.dtype == torch.bfloat16 and all(torch.equal(v.float(), sd[k]) for k, v in m.state_dict().items())


class _StubTokenizer:
    """words -> ids by position in a tiny vocabulary; <bos> first, padding (id 0) on the right; records what it was asked"""

    def __init__(self):
        self.calls = []

    def encode(self, text):
        return [2] + [3 + (sum(map(ord, w)) % 100) for w in text.split()]

    def __call__(self, prompts, padding, max_length, truncation, add_special_tokens, return_tensors):
        self.calls.append(dict(prompts=list(prompts), padding=padding, max_length=max_length, truncation=truncation))
        ids = torch.zeros(len(prompts), max_length, dtype=torch.int64)
        mask = torch.zeros_like(ids)
        for i, p in enumerate(prompts):
            e = self.encode(p)[:max_length]
            ids[i, :len(e)] = torch.tensor(e)
            mask[i, :len(e)] = 1
        return type("Enc", (), dict(input_ids=ids, attention_mask=mask))()


class _StubEncoder:
    """row t of the output is the token's id and its position: what was selected is readable from the result"""
    dtype, device = torch.float32, torch.device("cpu")

    def __call__(self, ids, attention_mask=None):
        self.seen = (ids, attention_mask)
        return (torch.stack([ids.float(), torch.arange(ids.shape[1]).expand_as(ids).float()], -1),)


def test_encode_prompt_sana_selection():
    from unigen_amd.gemma import encode_prompt_sana
    tok, enc = _StubTokenizer(), _StubEncoder()
    embeds, mask = encode_prompt_sana(enc, tok, ["  A Red Fox ", "two words"], max_sequence_length=6)
    assert tok.calls[-1] == dict(prompts=["a red fox", "two words"], padding="max_length", max_length=6, truncation=True)
    assert embeds[0, :, 1].tolist() == [0, 1, 2, 3, 4, 5] and mask.tolist() == [[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0]]
    chi = ["Line one of it:", "line two", "Prompt: "]
    embeds, mask = encode_prompt_sana(enc, tok, "  A Red Fox ", max_sequence_length=6, complex_human_instruction=chi, num_images_per_prompt=2)
    joined = "\n".join(chi)
    n = len(tok.encode(joined)) + 6 - 2
    assert tok.calls[-1]["prompts"] == [joined + "a red fox"] and tok.calls[-1]["max_length"] == n and enc.seen[0].shape == (1, n)
    assert tuple(embeds.shape) == (2, 6, 2) and embeds[0, :, 1].tolist() == [0] + list(range(n - 5, n)) and torch.equal(embeds[0], embeds[1])
    assert torch.equal(mask[0], enc.seen[1][0, [0] + list(range(n - 5, n))]) and torch.equal(mask[0], mask[1])
    ids, m = R.tiny_inputs()
    e, mm = encode_prompt_sana(enc, None, None, max_sequence_length=10, text_input_ids=ids, attention_mask=m)
    assert e[1, :, 1].tolist() == [0] + list(range(15, 24)) and torch.equal(mm, m[:, [0] + list(range(15, 24))])
    with pytest.raises(ValueError, match="tokenizer"):
        encode_prompt_sana(enc, None, "a prompt")
