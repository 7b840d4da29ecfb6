"""CPU tests of the text encoders' references and host side: tests/text_ref.py against the installed transformers library (tiny random configs,
no download) and against the committed fixture, the delta table against transformers' [H, L, L] bias bit for bit, the state-dict key handling,
encode_prompt's shapes with stub encoders, the pipeline's `_encode` behaviours and the new ABI symbols."""
import os
import re

import pytest
import torch

from tests import text_ref as R
from tests.util import rel_l2

os.environ.setdefault("HF_HUB_OFFLINE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_tiny.safetensors")


def golden():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


def _maker():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_text_golden", os.path.join(ROOT, "tests", "golden", "make_text_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_references_match_the_fixture():
    g = golden()
    assert os.path.getsize(GOLDEN) < (1 << 20)
    y = R.t5_encoder(R.decode_state(g, "t5.w."), R.T5_TINY, g["t5.ids"])
    assert rel_l2(y, g["t5.out.last_hidden_state"]) <= 2e-6          # transformers' own fp32 variance (6e-7) and the fp32 storage
    c = R.clip_text(R.decode_state(g, "clip.w."), R.CLIP_TINY, g["clip.ids"])
    assert rel_l2(c["last_hidden_state"], g["clip.out.last_hidden_state"]) <= 1e-7     # fp32 storage of float64 outputs
    assert rel_l2(c["pooler_output"], g["clip.out.pooler_output"]) <= 1e-7
    assert rel_l2(c["hidden_states"][-2], g["clip.out.hidden_m2"]) <= 1e-7
    assert R.clip_pool_index(g["clip.ids"], 5).tolist() == [9, 30] and len(c["hidden_states"]) == 4


def test_references_match_transformers():
    pytest.importorskip("transformers")
    g, mk = golden(), _maker()
    sd = R.decode_state(g, "t5.w.")
    with torch.no_grad():
        y = mk.hf_t5(R.T5_TINY, sd)(input_ids=g["t5.ids"].long())[0]
    assert rel_l2(R.t5_encoder(sd, R.T5_TINY, g["t5.ids"]), y) <= 2e-6
    sd = R.decode_state(g, "clip.w.")
    for eos, ids in ((5, g["clip.ids"]), (2, g["clip.ids"])):       # the first-EOS branch and the legacy argmax branch
        cfg = dict(R.CLIP_TINY, eos_token_id=eos)
        with torch.no_grad():
            h = mk.hf_clip(cfg, sd)(input_ids=ids.long(), output_hidden_states=True)
        c = R.clip_text(sd, cfg, ids)
        assert rel_l2(c["last_hidden_state"], h.last_hidden_state) <= 1e-13 and rel_l2(c["pooler_output"], h.pooler_output) <= 1e-13
        assert rel_l2(c["hidden_states"][-2], h.hidden_states[-2]) <= 1e-13 and len(h.hidden_states) == len(c["hidden_states"])


@pytest.mark.parametrize("L", (1, 77, 200, 512))
def test_delta_table_equals_transformers_bias(L):
    pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention, T5Config
    att = T5Attention(T5Config(**R.T5_TINY), has_relative_attention_bias=True)
    with torch.no_grad():
        bias = att.compute_bias(L, L)[0]                             # [H, L, L] fp32
    table = R.t5_rel_table(att.relative_attention_bias.weight.detach(), L, 32, 128)
    assert table.dtype == torch.float32 and torch.equal(R.bias_from_table(table, L, L), bias)


def test_bucket_function_shape():
    b = R.t5_bucket(torch.arange(-200, 201), 32, 128)
    assert b[200] == 0 and b[201] == 17 and b[199] == 1 and b[200 + 7] == 16 + 7 and b[0] == 15 and b[-1] == 31 and b[200 - 128] == 15
    assert (b[:200].flip(0)[1:] >= b[:200].flip(0)[:-1]).all()       # monotone in the distance


def test_attention_reference_modes():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, 5, 2, 64, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(2, 9, generator=g, dtype=torch.float64)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125 + R.bias_from_table(table, 5, 5)[None]
    s = s.masked_fill(torch.triu(torch.ones(5, 5, dtype=torch.bool), 1), float("-inf"))
    want = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)
    assert rel_l2(R.attention(q, k, v, 0.125, table, True), want) <= 1e-14
    assert R.bias_from_table(table, 5, 5)[1, 3, 1] == table[1, (1 - 3) + 4]


def test_norms_and_activations_match_torch():
    x = torch.randn(7, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w, b = torch.rand(128, dtype=torch.float64) + 0.5, torch.rand(128, dtype=torch.float64)
    assert rel_l2(R.layernorm(x, w, b, 1e-5), torch.nn.functional.layer_norm(x, (128,), w, b, 1e-5)) <= 1e-14
    assert rel_l2(R.rmsnorm(x, w, 1e-6), w * x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6)) <= 1e-14
    assert rel_l2(R.gelu_new(x), torch.nn.functional.gelu(x, approximate="tanh")) <= 1e-13
    assert rel_l2(R.quick_gelu(x), x * torch.sigmoid(1.702 * x)) <= 1e-14
    ab = torch.cat([x, x.flip(0)], -1)
    assert torch.equal(R.gated_gelu(ab), R.gelu_new(x) * x.flip(0))


def test_state_dict_key_handling():
    from unigen_amd.text import CLIPTextModel, T5EncoderModel
    g = golden()
    sd = R.decode_state(g, "clip.w.")
    a, b = CLIPTextModel.from_config(R.CLIP_TINY, dtype=torch.float32), CLIPTextModel.from_config(R.CLIP_TINY, dtype=torch.float32)
    a.load_state_dict(sd)
    b.load_state_dict({**{"text_model." + k: v for k, v in sd.items()}, "text_model.embeddings.position_ids": torch.arange(77)[None]})
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict()) and all(k.startswith("text_model.") for k in a.state_dict())
    p = "encoder.layers.1.self_attn."
    assert torch.equal(a.layers[1]["qkv"], torch.cat([sd[p + f"{n}_proj.weight"] for n in "qkv"]))              # one packed weight
    assert a.state_dict()["text_model." + p + "k_proj.weight"].data_ptr() == a.layers[1]["qkv"][128:].data_ptr()    # the named parameter is a view of it
    with pytest.raises(KeyError):
        a.load_state_dict({k: v for k, v in sd.items() if "fc1" not in k})
    sd = R.decode_state(g, "t5.w.")
    t, u = T5EncoderModel.from_config(R.T5_TINY, dtype=torch.float32), T5EncoderModel.from_config(R.T5_TINY, dtype=torch.float32)
    t.load_state_dict(sd)
    alias = {("encoder.embed_tokens.weight" if k == "shared.weight" else k): v for k, v in sd.items()}
    u.load_state_dict(alias)
    u.load_state_dict({**sd, "encoder.embed_tokens.weight": sd["shared.weight"]})
    assert all(torch.equal(t.state_dict()[k], u.state_dict()[k]) for k in t.state_dict()) and set(t.state_dict()) == set(sd)
    p = "encoder.block.1.layer.1.DenseReluDense."
    assert torch.equal(t.layers[1]["wi"], torch.cat([sd[p + "wi_0.weight"], sd[p + "wi_1.weight"]]))
    assert t.dtype == torch.float32 and t.device.type == "cpu"
    with pytest.raises(NotImplementedError, match="gated-gelu"):
        T5EncoderModel.from_config(dict(R.T5_TINY, feed_forward_proj="relu"))
    with pytest.raises(NotImplementedError, match="hidden_act"):
        CLIPTextModel.from_config(dict(R.CLIP_TINY, hidden_act="gelu"))
    from unigen_amd import lib
    with pytest.raises(lib.UniGenHipError):                          # no CPU path
        t(g["t5.ids"])


def test_from_pretrained_reads_config_and_safetensors(tmp_path):
    import json
    from safetensors.torch import save_file
    from unigen_amd.text import CLIPTextModel, T5EncoderModel
    g = golden()
    for sub, cfg, pre, cls, disk_pre in (("text_encoder", R.CLIP_TINY, "clip.w.", CLIPTextModel, "text_model."), ("text_encoder_2", R.T5_TINY, "t5.w.", T5EncoderModel, "")):
        d = tmp_path / sub
        d.mkdir()
        (d / "config.json").write_text(json.dumps(cfg))
        sd = R.decode_state(g, pre)
        names = sorted(sd)
        save_file({disk_pre + k: sd[k].contiguous() for k in names[::2]}, str(d / "model-00001-of-00002.safetensors"))
        save_file({disk_pre + k: sd[k].contiguous() for k in names[1::2]}, str(d / "model-00002-of-00002.safetensors"))
        m = cls.from_pretrained(str(tmp_path), subfolder=sub, dtype=torch.float32)
        have = m.state_dict()
        assert all(torch.equal(have[disk_pre + k], sd[k]) for k in names)


class _Stub:
    dtype, device = torch.bfloat16, torch.device("cpu")

    def __init__(self, width):
        self.width, self.calls = width, []

    def __call__(self, ids, output_hidden_states=False):
        from unigen_amd.text import TextEncoderOutput
        self.calls.append(ids)
        last = ids[..., None].to(torch.bfloat16).expand(*ids.shape, self.width).contiguous()
        return TextEncoderOutput(last, last[:, 0])


def test_encode_prompt_shapes_with_stub_encoders():
    from src.text_encoder import encode_prompt
    clip, t5 = _Stub(8), _Stub(16)
    cid, tid = torch.arange(2 * 77).view(2, 77) % 50, torch.arange(2 * 12).view(2, 12)
    e, p, t = encode_prompt([clip, t5], [None, None], None, 12, num_images_per_prompt=3, text_input_ids_list=[cid, tid])
    assert tuple(e.shape) == (6, 12, 16) and tuple(p.shape) == (6, 8) and tuple(t.shape) == (12, 3) and not t.any() and t.dtype == torch.bfloat16
    assert torch.equal(e[:, 0, 0].float(), torch.tensor([0, 0, 0, 12, 12, 12.0])) and torch.equal(p[:, 0].float(), torch.tensor([0, 27, 0, 27, 0, 27.0]))
    assert tuple(encode_prompt([clip], [None], None, 12, text_input_ids_list=[cid]).shape) == (2, 8)
    tok = lambda prompt, max_length=None, **kw: type("T", (), {"input_ids": torch.ones(len(prompt), max_length, dtype=torch.long)})()
    e, p, t = encode_prompt([clip, t5], [tok, tok], "one prompt", 20)
    assert tuple(e.shape) == (1, 20, 16) and tuple(clip.calls[-1].shape) == (1, 77)
    with pytest.raises(ValueError, match="text_input_ids"):
        encode_prompt([clip, t5], [None, None], "x", 12)


def test_pipeline_encode_behaviours():
    from unigen_amd.pipeline import UniGenFLUXPipeline
    pipe = UniGenFLUXPipeline()
    a, b = torch.zeros(1, 4, 16), torch.zeros(1, 8)
    assert pipe._encode("prompt", None, None, a, b, "cpu", 1, 12) == (a, b)                            # embeds pass through
    with pytest.raises(NotImplementedError, match="encode_prompt"):                                   # nothing attached
        pipe._encode("prompt", "text", None, None, None, "cpu", 1, 12)
    pipe.text_encoder, pipe.text_encoder_2 = _Stub(8), _Stub(16)
    ids = (torch.ones(1, 77, dtype=torch.long), torch.ones(1, 12, dtype=torch.long))
    e, p = pipe._encode("prompt", ids, None, None, None, None, 2, 12)                                   # the new path, on ids
    assert tuple(e.shape) == (2, 12, 16) and tuple(p.shape) == (2, 8)
    with pytest.raises(TypeError, match="token ids"):
        pipe._encode("prompt", "text", None, None, None, None, 1, 12)
    tok = lambda prompt, max_length=None, **kw: type("T", (), {"input_ids": torch.ones(len(prompt), max_length, dtype=torch.long)})()
    pipe.tokenizer, pipe.tokenizer_2 = tok, tok
    assert tuple(pipe._encode("prompt", ["a", "b"], None, None, None, None, 1, 12)[0].shape) == (2, 12, 16)   # through attached tokenizers
    pipe.encode_prompt = lambda **kw: ("E", "P", None)                                                # an attached callable wins
    assert pipe._encode("prompt", ids, None, None, None, None, 1, 12) == ("E", "P")
    assert len(pipe.text_encoder.calls) == 2


def test_new_abi_symbols():
    from unigen_amd import build, lib
    hdr = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    declared = set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", hdr))
    new = {"ug_flash_attn_fwd_bias", "ug_t5_rel_table", "ug_rmsnorm_rows", "ug_layernorm_rows", "ug_gated_gelu", "ug_quick_gelu"}
    new |= {n + "_f32" for n in new}
    assert new <= declared and new <= set(lib.SIGNATURES) and "text.hip" in build.SOURCES
    cdll = lib.load()
    assert cdll.ug_version() >= 210
    # argument validation happens before any launch
    assert cdll.ug_flash_attn_fwd_bias(16, 64, 64, 16, 64, 64, 16, 64, 64, 16, 64, 64, 1, 1, 8, 8, 128, 1.0, None, 0, 1, None) == lib.UG_ERR_UNSUPPORTED
    assert cdll.ug_flash_attn_fwd_bias(16, 64, 64, 16, 64, 64, 16, 64, 64, 16, 64, 64, 1, 1, 8, 8, 64, 1.0, 16, 4, 0, None) == lib.UG_ERR_BAD_SHAPE
    assert b"rel_len" in cdll.ug_last_error()
    assert cdll.ug_rmsnorm_rows(16, 12, 16, 16, 12, 1, 12, 1e-6, None) == lib.UG_ERR_UNSUPPORTED
    assert cdll.ug_quick_gelu(16, 16, 12, None) == lib.UG_ERR_UNSUPPORTED and cdll.ug_gated_gelu(16, 8, 16, 8, 1, 8, None) == lib.UG_ERR_BAD_SHAPE


# ---- the sweep's references, cases and bounds (tests/test_fuzz_text_gpu.py) ------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lkv", ((5, 77), (200, 33), (129, 128)))
def test_bias_at_unequal_lengths_equals_transformers(Lq, Lkv):
    """a table longer than the launch needs: the extra entries do not matter"""
    pytest.importorskip("transformers")
    from transformers.models.t5.modeling_t5 import T5Attention, T5Config
    att = T5Attention(T5Config(**R.T5_TINY), has_relative_attention_bias=True)
    with torch.no_grad():
        bias = att.compute_bias(Lq, Lkv)[0]                          # [H, Lq, Lkv] fp32
    w = att.relative_attention_bias.weight.detach()
    for rel_len in (max(Lq, Lkv), max(Lq, Lkv) + 37):
        assert torch.equal(R.bias_from_table(R.t5_rel_table(w, rel_len, 32, 128), Lq, Lkv), bias)


def _sweep_and_fixed():
    return [R.attn_sweep_spec(i) for i in range(R.N_ATTN_SWEEP)] + list(R.ATTN_FIXED.values())


def _case(spec):
    return R.attn_fixed_case(spec["id"]) if spec["id"] in R.ATTN_FIXED else R.attn_sweep_case(spec["i"])


def test_attention_sweep_grid():
    specs = [R.attn_sweep_spec(i) for i in range(R.N_ATTN_SWEEP)]
    assert {s["B"] for s in specs} == {1, 2, 3} and {s["H"] for s in specs} == {1, 3, 5, 12}
    assert {(s["mode"], s["regime"]) for s in specs} == set(R.ATTN_COMBOS) and len(R.ATTN_COMBOS) == 14
    assert {s["rel_len"] - max(s["Lq"], s["Lkv"]) for s in specs if s["bias"]} == {0, 1, 37}
    assert all(s["Lq"] in R.ATTN_LENGTHS and s["Lkv"] in R.ATTN_LENGTHS and s["B"] * s["H"] * s["Lq"] * s["Lkv"] <= R.ATTN_CAP for s in specs)
    assert any(s["Lq"] != s["Lkv"] and s["rel_len"] > max(s["Lq"], s["Lkv"]) for s in specs)
    lays = [s["layout"] for s in specs]
    assert {l["shared"] for l in lays} == {True, False} and {l["o"]["off"] for l in lays} == {0, 4}
    assert any(l["o"]["colpad"] % 8 == 4 for l in lays) and all(l["o"]["colpad"] % 4 == 0 and l[n]["colpad"] % 8 == 0 for l in lays for n in "qkv")
    assert len({s["id"] for s in specs}) == len(specs)
    f = R.ATTN_FIXED
    assert (f["rel4096"]["rel_len"], f["rel4096"]["H"]) == (4096, 3) and R.attn_fixed_case("rel4096")["table"].shape == (3, 8191)
    assert [(f[n]["Lq"], f[n]["Lkv"], f[n]["mode"]) for n in ("q1_kv520", "q520_kv1", "causal_129x33", "causal_33x257")] == \
        [(1, 520, "bias"), (520, 1, "bias"), (129, 33, "causal"), (33, 257, "causal")]


def test_attention_layout_round_trip():
    """the buffers hold the case where the strides say, NaN elsewhere; the output reader finds the region and a touched sentinel"""
    for i in (0, 2):
        c = R.attn_sweep_case(i)
        bufs = R.attn_buffers(c, torch.bfloat16)
        for n, L in (("q", c["Lq"]), ("k", c["Lkv"]), ("v", c["Lkv"])):
            t = bufs[n]
            got = torch.as_strided(t["buf"], (c["B"], L, t["width"]), (t["bs"], t["rs"], 1), t["off"])
            assert torch.equal(got.double().view(c["B"], L, c["H"], 64), c[n]) and t["rs"] % 8 == 0 and t["bs"] % 8 == 0
            held = c["B"] * (c["Lq"] + 2 * c["Lkv"]) * t["width"] if c["layout"]["shared"] else got.numel()
            assert int(torch.isnan(t["buf"]).sum()) == t["buf"].numel() - held
        o = bufs["o"]
        assert o["rs"] % 4 == 0 and o["bs"] % 4 == 0 and (o["off"] - R.GUARD) == c["layout"]["o"]["off"]
        got, intact = R.attn_read_output(c, o, o["buf"])
        assert intact and bool((got == R.SENT_O).all())
        o["buf"][o["off"] + c["H"] * 64] = 1.0                     # the first pad column of row 0, or the next row's first element without a pad
        assert R.attn_read_output(c, o, o["buf"])[1] == (c["layout"]["o"]["colpad"] == 0 and c["Lq"] > 1)


@pytest.mark.parametrize("slip", list(R.ATTN_SLIPS))
def test_every_attention_slip_misses_the_gpu_bound(slip):
    """A kernel that commits the slip, rounding where the product path rounds, misses the bound that tests/test_fuzz_text_gpu.py applies (the same
    judge), on at least one case of a mode in which the slip can happen; the right reference, rounded the same way, passes it."""
    caught = []
    for spec in _sweep_and_fixed():
        if spec["mode"] not in R.ATTN_SLIPS[slip]:
            continue
        c = _case(spec)
        truth, variant = R.attn_refs(c)
        wrong = R.attention(c["q"], c["k"], c["v"], c["scale"], c["table"], c["causal"], rnd=R.bf, slip=slip)
        ratio = R.attn_judge(wrong, truth, variant, True)[0]
        assert R.attn_judge(variant, truth, variant, True)[0] <= 1.0
        if not ratio <= 1.0:
            caught.append((spec["id"], ratio))
        if len(caught) >= 2:
            break
    print(f"TEXT slip {slip}: caught by {caught}")
    assert caught, f"no case tells {slip} from the right kernel"


def test_attention_regimes_do_what_they_claim():
    seen = set()
    for i in range(R.N_ATTN_SWEEP):
        spec = R.attn_sweep_spec(i)
        if spec["regime"] == "gaussian" or (spec["regime"], spec["mode"]) in seen:
            continue
        seen.add((spec["regime"], spec["mode"]))
        c = R.attn_sweep_case(i)
        Lq, Lkv = c["Lq"], c["Lkv"]
        s = torch.einsum("bqhd,bkhd->bhqk", c["q"], c["k"]) * c["scale"]
        if c["bias"]:
            s = s + R.bias_from_table(c["table"].double(), Lq, Lkv)[None]
        qpos, kpos = torch.arange(Lq)[:, None], torch.arange(Lkv)[None, :]
        if c["causal"]:
            s = s.masked_fill(kpos > qpos, float("-inf"))
        assert torch.isfinite(s.amax(-1)).all() and float(s[torch.isfinite(s)].abs().max()) < 1e4        # every score finite in fp32, by far
        p = torch.softmax(s, -1)
        if c["regime"] in ("rising", "falling"):
            nt = (Lkv + 63) // 64
            pad = torch.full((*s.shape[:-1], nt * 64 - Lkv), float("-inf"), dtype=s.dtype)
            tiles = torch.cat([s, pad], -1).view(*s.shape[:-1], nt, 64)[:, :, c["rows"]]               # [B, H, rows, tiles, 64]
            tmax, full = tiles.amax(-1), torch.isfinite(tiles).sum(-1) >= 16                           # a tile counts where the row sees 16 of its keys
            up = tmax[..., 1:] > tmax[..., :-1] if c["regime"] == "rising" else tmax[..., 1:] < tmax[..., :-1]
            vis = full[..., 1:] & full[..., :-1]
            run3 = (up[..., 1:] & up[..., :-1] & vis[..., 1:] & vis[..., :-1]).any(-1)                   # three consecutive tiles, each above the last
            have3 = (vis.sum(-1) >= 2)
            assert len(c["rows"]) * 2 >= Lq and bool(have3.any()) and float(run3[have3].double().mean()) >= 0.99, spec["id"]
            if c["regime"] == "rising":
                assert float((up & vis).sum()) >= 0.95 * float(vis.sum()), spec["id"]      # and nearly every tile raises a chosen row's maximum
        elif c["regime"] == "spike_tail":
            key = c["spike_key"]
            assert Lkv % 64 and Lkv // 64 * 64 <= key < Lkv and len(c["rows"]) > 0
            assert float(p[:, :, c["rows"], key].min()) > 0.5, spec["id"]
            assert abs(len(c["rows"]) - (Lq + 3) // 4) <= (0 if not c["causal"] else Lq)
        elif c["regime"] == "far_bias":
            near = ((kpos - qpos).abs() <= 16).to(p.dtype)
            assert float((p * near).sum(-1).min()) >= 0.5, spec["id"]
            assert float(c["table"][:, (torch.arange(c["table"].shape[1]) - (c["rel_len"] - 1)).abs() == 40].min()) < -55       # (the other side may be an entry that no launch reads)
    assert len(seen) == 11


def test_constant_and_zero_rows_have_zero_variance():
    kinds = set()
    for c in R.norm_sweep_cases():
        x, w, b = R.norm_data(c)
        for r, kind in enumerate(R.norm_row_kinds(c)):
            kinds.add((kind, c["D"] > 4608))
            if kind in ("constant", "zero"):
                mu = x[r].mean()
                assert float(((x[r] - mu) ** 2).mean()) == 0.0 and torch.equal(R.layernorm(x[r:r + 1], w, b, 1e-5)[0], b)
                assert torch.equal(R.layernorm_bound(x[r:r + 1], w, b, 1e-5, True)[0][0], b)
                if kind == "zero":
                    assert not R.rmsnorm(x[r:r + 1], w, 1e-6).any()
            if kind == "big_mean" and c["D"] >= 512:                 # (eight such values all round to the mean)
                assert 300 < float(x[r].mean().abs() / x[r].std()) < 3000
    assert kinds == {(k, wide) for k in R.NORM_KINDS for wide in (False, True)}          # each kind on both sides of the register-resident limit
    cases = R.norm_sweep_cases()
    assert {(c["D"], c["rows"]) for c in cases} == {(D, r) for D in R.NORM_D for r in R.NORM_ROWS}
    assert {(c["ldx"] - c["D"], c["ldo"] - c["D"]) for c in cases} == {(a, b) for a in R.NORM_PADS for b in R.NORM_PADS}
    acts = R.act_sweep_cases()
    assert {(c["M"], c["F"]) for c in acts} == {(m, f) for m in R.ACT_M for f in R.ACT_F}
    assert {(c["ld"] - 2 * c["F"], c["ldo"] - c["F"]) for c in acts} == {(a, b) for a in R.ACT_PADS for b in R.ACT_PADS}
    x = R.all_finite_bf16()
    assert torch.equal(R.bf(x), x) and x.unique().numel() == 65279 and int((x == 0).sum()) == 2        # +0 and -0 are one value, two patterns


def test_elementwise_excess_handles_overflow_only_where_the_truth_overflows():
    truth = torch.tensor([1e39, -1e39, 1.0, 1e39, 1.0], dtype=torch.float64)
    got = torch.tensor([float("inf"), float("-inf"), 1.0, float("-inf"), float("inf")], dtype=torch.float64)
    bound = torch.full_like(truth, 1e-3)
    assert R.elementwise_excess(got[:3], truth[:3], bound[:3], True) == 0.0
    assert R.elementwise_excess(got[3:4], truth[3:4], bound[3:4], True) == float("inf")
    assert R.elementwise_excess(got[4:], truth[4:], bound[4:], False) == float("inf")
    assert R.elementwise_excess(torch.tensor([float("nan")], dtype=torch.float64), truth[2:3], bound[2:3], True) == float("inf")
