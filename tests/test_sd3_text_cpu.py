"""CPU tests of SD3's prompt encoding: the references of tests/sd3_text_ref.py against the installed transformers library and against the committed
fixtures, the new ABI symbols, CLIPTextModelWithProjection's state-dict handling, encode_prompt_sd3 / encode_condition_prompt_sd3 on stub encoders of
known widths, and UniGenSD3Pipeline's prompt handling on stubs."""
import importlib.util
import inspect
import json
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import sd3_text_ref as S
from tests import text_ref as R
from tests.util import rel_l2

os.environ.setdefault("HF_HUB_OFFLINE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
F32, F64 = torch.float32, torch.float64


def golden():
    from safetensors.torch import load_file
    return {**load_file(os.path.join(GOLDEN_DIR, "sd3_text_tiny.safetensors")), **load_file(os.path.join(GOLDEN_DIR, "sd3_text_tiny_t5.safetensors"))}


def _maker():
    spec = importlib.util.spec_from_file_location("make_sd3_text_golden", os.path.join(GOLDEN_DIR, "make_sd3_text_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- fixture and restatement ------------------------------------------------------------------------------------------------------------------------
def test_fixture_regenerates_bit_identically():
    pytest.importorskip("transformers")
    from safetensors.torch import load_file
    mk = _maker()
    for name, fresh in zip((mk.CLIP_FILE, mk.T5_FILE), mk.tensors()):
        path = os.path.join(GOLDEN_DIR, name)
        assert os.path.getsize(path) < (1 << 20)
        stored = load_file(path)
        assert set(stored) == set(fresh)
        for k in fresh:
            assert stored[k].dtype == fresh[k].dtype and torch.equal(stored[k], fresh[k]), k


def test_references_match_the_fixture():
    g = golden()
    for name, cfg, where in (("clip_a", S.CLIP_A, [9, 30]), ("clip_b", S.CLIP_B, [12, 40])):
        c = S.clip_text_proj(R.decode_state(g, f"{name}.w."), cfg, g[f"{name}.ids"])
        assert len(c["hidden_states"]) == cfg["num_hidden_layers"] + 1 and tuple(c["text_embeds"].shape) == (2, cfg["projection_dim"])
        got = dict(text_embeds=c["text_embeds"], last_hidden_state=c["last_hidden_state"], hidden_m2=c["hidden_states"][-2], hidden_m3=c["hidden_states"][-3])
        for key, t in got.items():
            assert rel_l2(t, g[f"{name}.out.{key}"]) <= S.FIXTURE_MARGIN, (name, key)
        assert R.clip_pool_index(g[f"{name}.ids"], cfg["eos_token_id"]).tolist() == where
    y = R.t5_encoder(R.decode_state(g, "t5.w."), S.T5_SD3, g["t5.ids"])
    assert tuple(y.shape) == (2, S.T5_LEN, 256) and rel_l2(y, g["t5.out.last_hidden_state"]) <= 2e-6     # transformers' own fp32 variance, as for text_tiny


def test_references_match_transformers():
    """and what the restatement assumes of the installed transformers: the output fields, the erf GELU behind "gelu", the legacy argmax pooling"""
    pytest.importorskip("transformers")
    from transformers.activations import GELUActivation
    g, mk = golden(), _maker()
    for name, cfg in (("clip_a", S.CLIP_A), ("clip_b", S.CLIP_B)):
        sd, ids = R.decode_state(g, f"{name}.w."), g[f"{name}.ids"]
        m = mk.hf_clip_proj(cfg, sd)
        with torch.no_grad():
            h = m(input_ids=ids.long(), output_hidden_states=True)
        assert list(h.keys()) == ["text_embeds", "last_hidden_state", "hidden_states"] and h[0] is h.text_embeds
        c = S.clip_text_proj(sd, cfg, ids)
        assert rel_l2(c["text_embeds"], h.text_embeds) <= S.HF_MARGIN and rel_l2(c["last_hidden_state"], h.last_hidden_state) <= S.HF_MARGIN
        assert len(h.hidden_states) == len(c["hidden_states"])
        assert all(rel_l2(a, b) <= S.HF_MARGIN for a, b in zip(c["hidden_states"], h.hidden_states))
        if cfg["hidden_act"] == "gelu":
            acts = [mod for mod in m.modules() if isinstance(mod, GELUActivation)]
            assert len(acts) == cfg["num_hidden_layers"]
            x = torch.linspace(-6, 6, 97, dtype=F64)
            assert rel_l2(S.gelu_erf(x), acts[0](x)) <= 1e-15 and rel_l2(S.gelu_erf(x), torch.nn.functional.gelu(x)) <= 1e-15
            # eos_token_id = 2: the pooled row is the one at the argmax of the ids, wherever a token 2 may stand
            moved = ids.clone()
            moved[0, 3] = 2
            with torch.no_grad():
                o = m(input_ids=moved.long())
            w = sd["text_projection.weight"].double()
            assert rel_l2(o.text_embeds[0], o.last_hidden_state[0, 12] @ w.t()) <= S.HF_MARGIN < 1e-2 < rel_l2(o.text_embeds[0], o.last_hidden_state[0, 3] @ w.t())
            assert rel_l2(S.clip_text_proj(sd, cfg, moved)["text_embeds"], o.text_embeds) <= S.HF_MARGIN


def test_gelu_erf_bound_leaves_room_for_the_device():
    """an fp32 evaluation of either formulation (plain erf; erfc for negative x) stays at 0.09 of the bound over every finite bf16 input"""
    x = R.all_finite_bf16()
    truth, bound = S.gelu_erf_bound(x, False)
    xf = x.float()
    u = xf * 0.70710678118654752
    plain = 0.5 * xf * (1 + torch.special.erf(u))
    tail = torch.where(xf < 0, 0.5 * xf * torch.special.erfc(-u), plain)
    for y in (plain, tail):
        worst = R.elementwise_excess(y, truth, bound, False)
        print(f"SD3TEXT gelu_erf fp32 on the host: worst |err| / bound = {worst:.4f}")
        assert worst <= 0.1
    assert torch.equal(truth[x == 0], torch.zeros(2, dtype=F64)) and float(truth[x == 1.0]) == pytest.approx(0.8413447460685429, abs=1e-15)


# ---- header and bindings ----------------------------------------------------------------------------------------------------------------------------
def test_new_abi_symbols():
    from unigen_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "unigen_hip.h")).read()
    declared = set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", hdr))
    new = {"ug_gelu_erf", "ug_gelu_erf_f32"}
    assert new <= declared and new <= set(lib.SIGNATURES) and declared == set(lib.SIGNATURES)
    assert lib.SIGNATURES["ug_gelu_erf"] == lib.SIGNATURES["ug_quick_gelu"] == lib.SIGNATURES["ug_gelu_erf_f32"] and callable(ops.gelu_erf)
    cdll = lib.load()                                    # raises if the library lacks a declared symbol
    assert cdll.ug_version() >= 220
    # argument validation happens before any launch, with ug_quick_gelu's codes
    for fn, twin in ((cdll.ug_gelu_erf, cdll.ug_quick_gelu), (cdll.ug_gelu_erf_f32, cdll.ug_quick_gelu_f32)):
        assert fn(16, 16, 12, None) == twin(16, 16, 12, None) == lib.UG_ERR_UNSUPPORTED
        assert b"multiple of 8" in cdll.ug_last_error()
        assert fn(None, 16, 8, None) == twin(None, 16, 8, None) == lib.UG_ERR_BAD_SHAPE
        assert fn(16, 16, -8, None) == twin(16, 16, -8, None) == lib.UG_ERR_BAD_SHAPE
        assert fn(16, 24, 8, None) == twin(16, 24, 8, None) == lib.UG_ERR_BAD_ALIGN
        assert fn(None, None, 0, None) == twin(None, None, 0, None) == lib.UG_OK


# ---- the model class --------------------------------------------------------------------------------------------------------------------------------
def test_projected_clip_state_dict_handling():
    from unigen_amd import CLIPTextModelWithProjection as exported
    from unigen_amd.text import CLIPTextModel, CLIPTextModelWithProjection
    assert exported is CLIPTextModelWithProjection and issubclass(CLIPTextModelWithProjection, CLIPTextModel)
    g = golden()
    sd = R.decode_state(g, "clip_b.w.")
    a, b = (CLIPTextModelWithProjection.from_config(S.CLIP_B, dtype=F32) for _ in range(2))
    a.load_state_dict(sd)
    b.load_state_dict({**{("text_model." + k if k != "text_projection.weight" else k): v for k, v in sd.items()},
                       "text_model.embeddings.position_ids": torch.arange(77)[None]})
    have = a.state_dict()
    assert set(have) == {("text_model." + k if k != "text_projection.weight" else k) for k in S.clip_proj_keys(S.CLIP_B)}      # the on-disk names
    assert all(torch.equal(have[k], b.state_dict()[k]) for k in have)
    assert torch.equal(have["text_projection.weight"], sd["text_projection.weight"]) and tuple(a.proj.shape) == (96, 128)
    assert have["text_projection.weight"].data_ptr() == a.proj.data_ptr()                         # the named parameter is a view of its pack
    with pytest.raises(KeyError):
        a.load_state_dict({k: v for k, v in sd.items() if k != "text_projection.weight"})
    with pytest.raises(KeyError):                                                                 # it does not live under text_model. on disk
        a.load_state_dict({**sd, "text_model.text_projection.weight": sd["text_projection.weight"]})
    assert CLIPTextModelWithProjection.from_config({k: v for k, v in S.CLIP_B.items() if k != "projection_dim"}).config["projection_dim"] == 512
    # the erf GELU is the subclass's; the plain text model goes on refusing it, and takes no projection
    assert "gelu" in CLIPTextModelWithProjection.ACTS and "gelu" not in CLIPTextModel.ACTS and set(CLIPTextModel.ACTS) < set(CLIPTextModelWithProjection.ACTS)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        CLIPTextModel.from_config(S.CLIP_B)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        CLIPTextModelWithProjection.from_config(dict(S.CLIP_B, hidden_act="relu"))
    with pytest.raises(KeyError):
        CLIPTextModel.from_config(S.CLIP_A, dtype=F32).load_state_dict(R.decode_state(g, "clip_a.w."))
    from unigen_amd import lib
    with pytest.raises(lib.UniGenHipError):                                                       # no CPU path
        a(g["clip_b.ids"])


def test_projected_clip_from_pretrained_keeps_the_projection(tmp_path):
    from safetensors.torch import save_file
    from unigen_amd.text import CLIPTextModel, CLIPTextModelWithProjection
    g = golden()
    for sub, cfg, pre in (("text_encoder", S.CLIP_A, "clip_a.w."), ("text_encoder_2", S.CLIP_B, "clip_b.w.")):
        d = tmp_path / sub
        d.mkdir()
        (d / "config.json").write_text(json.dumps(cfg))
        sd = R.decode_state(g, pre)
        disk = {("text_model." + k if k != "text_projection.weight" else k): v.contiguous() for k, v in sd.items()}
        disk.update({"logit_scale": torch.tensor(4.6), "vision_model.embeddings.class_embedding": torch.zeros(8), "visual_projection.weight": torch.zeros(4, 8)})
        names = sorted(disk)
        save_file({k: disk[k] for k in names[::2]}, str(d / "model-00001-of-00002.safetensors"))
        save_file({k: disk[k] for k in names[1::2]}, str(d / "model-00002-of-00002.safetensors"))
        m = CLIPTextModelWithProjection.from_pretrained(str(tmp_path), subfolder=sub, dtype=F32)
        have = m.state_dict()
        assert isinstance(m, CLIPTextModelWithProjection) and m.config["projection_dim"] == cfg["projection_dim"]
        assert set(have) == {k for k in disk if k.startswith(("text_model.", "text_projection."))} and all(torch.equal(have[k], disk[k]) for k in have)
    plain = CLIPTextModel.from_pretrained(str(tmp_path), subfolder="text_encoder", dtype=F32)      # unchanged: the plain model leaves the projection out
    assert "text_projection.weight" not in plain.state_dict() and not hasattr(plain, "proj")


# ---- the encode functions on stub encoders ----------------------------------------------------------------------------------------------------------
class _Clip:
    """hidden_states[k][b, l, :] = ids[b, l] + 1000 k + tag; text_embeds[b, :] = ids[b, 0] + tag"""
    dtype, device = F32, torch.device("cpu")

    def __init__(self, width, proj, tag):
        self.width, self.proj, self.tag, self.calls = width, proj, tag, []

    def __call__(self, ids, output_hidden_states=False):
        from unigen_amd.text import CLIPTextModelOutput
        self.calls.append((ids, output_hidden_states))
        base = ids[..., None].to(F32).expand(*ids.shape, self.width)
        hs = tuple(base + 1000.0 * k + self.tag for k in range(4))
        return CLIPTextModelOutput(ids[:, :1].to(F32).expand(-1, self.proj) + self.tag, hs[-1] + 0.5, hs if output_hidden_states else None)


class _T5:
    dtype, device = F32, torch.device("cpu")

    def __init__(self, width):
        self.width, self.calls = width, []

    def __call__(self, ids, **kw):
        from unigen_amd.text import TextEncoderOutput
        self.calls.append(ids)
        return TextEncoderOutput(-ids[..., None].to(F32).expand(*ids.shape, self.width).contiguous())


def _ids(seed=0, L3=12):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, 60, (2, 77), generator=g), torch.randint(1, 60, (2, 77), generator=g), torch.randint(1, 60, (2, L3), generator=g)]


def test_encode_prompt_sd3_on_stub_encoders():
    from unigen_amd import encode_condition_prompt_sd3 as cond_exported
    from unigen_amd.text import encode_condition_prompt_sd3, encode_prompt_sd3
    assert cond_exported is encode_condition_prompt_sd3
    cl, cg, t5 = _Clip(8, 4, 0.25), _Clip(16, 6, 0.5), _T5(32)
    ids, neg = _ids(0), _ids(1)
    e, ne, p, npool = encode_prompt_sd3([cl, cg, t5], [None] * 3, None, num_images_per_prompt=3, text_input_ids_list=ids, negative_text_input_ids_list=neg,
                                        max_sequence_length=12)
    assert tuple(e.shape) == tuple(ne.shape) == (6, 77 + 12, 32) and tuple(p.shape) == tuple(npool.shape) == (6, 4 + 6) and e.dtype == F32
    assert all(c[1] is True for c in cl.calls + cg.calls) and len(cl.calls) == len(cg.calls) == len(t5.calls) == 2
    seq_rows, pool_rows = [0, 0, 0, 1, 1, 1], [0, 1, 0, 1, 0, 1]                       # diffusers' two repeat orders
    for got, pooled, src in ((e, p, ids), (ne, npool, neg)):
        assert torch.equal(got[:, :77, :8], (src[0].float() + 2000.25)[seq_rows][..., None].expand(-1, -1, 8))          # hidden_states[-2] of the first CLIP
        assert torch.equal(got[:, :77, 8:24], (src[1].float() + 2000.5)[seq_rows][..., None].expand(-1, -1, 16))
        assert not got[:, :77, 24:].any()                                                                               # the pad is exactly zero
        assert torch.equal(got[:, 77:], -src[2].float()[seq_rows][..., None].expand(-1, -1, 32))                        # the T5 rows behind them
        assert torch.equal(pooled[:, :4], (src[0][:, :1].float() + 0.25)[pool_rows].expand(-1, 4))
        assert torch.equal(pooled[:, 4:], (src[1][:, :1].float() + 0.5)[pool_rows].expand(-1, 6))
    # clip_skip = 1: hidden_states[-3], for the prompt only (the negatives keep [-2]); no guidance: no negatives
    e1, ne1, p1, _ = encode_prompt_sd3([cl, cg, t5], [None] * 3, None, clip_skip=1, text_input_ids_list=ids, negative_text_input_ids_list=neg, max_sequence_length=12)
    assert torch.equal(e1[:, :77, :8], (ids[0].float() + 1000.25)[..., None].expand(-1, -1, 8)) and torch.equal(ne1, ne[[0, 3]]) and torch.equal(p1, p[:2])
    e0, none_e, p0, none_p = encode_prompt_sd3([cl, cg, t5], [None] * 3, None, do_classifier_free_guidance=False, text_input_ids_list=ids, max_sequence_length=12)
    assert none_e is None and none_p is None and torch.equal(e0, e[[0, 3]]) and torch.equal(p0, p[:2])
    ce, cp = encode_condition_prompt_sd3([cl, cg, t5], [None] * 3, None, num_images_per_prompt=3, text_input_ids_list=ids, max_sequence_length=12)
    assert torch.equal(ce, e) and torch.equal(cp, p)
    # no third encoder: zeros of the stated shape
    z, _, zp, _ = encode_prompt_sd3([cl, cg, None], [None] * 3, None, do_classifier_free_guidance=False, num_images_per_prompt=3, text_input_ids_list=ids[:2] + [None],
                                    max_sequence_length=10, joint_attention_dim=32)
    assert tuple(z.shape) == (6, 77 + 10, 32) and not z[:, 77:].any() and torch.equal(z[:, :77], e[:, :77]) and torch.equal(zp, p)
    assert tuple(encode_prompt_sd3([cl, cg, None], [None] * 3, None, do_classifier_free_guidance=False, text_input_ids_list=ids[:2] + [None],
                                   joint_attention_dim=32)[0].shape) == (2, 77 + 256, 32)                               # max_sequence_length defaults to 256
    with pytest.raises(ValueError, match="joint_attention_dim"):
        encode_prompt_sd3([cl, cg, None], [None] * 3, None, do_classifier_free_guidance=False, text_input_ids_list=ids[:2] + [None])
    with pytest.raises(ValueError, match="text_input_ids"):
        encode_prompt_sd3([cl, cg, t5], [None] * 3, "a prompt", do_classifier_free_guidance=False)
    with pytest.raises(ValueError, match="negative_text_input_ids_list"):
        encode_prompt_sd3([cl, cg, t5], [None] * 3, None, text_input_ids_list=ids)


def test_encode_prompt_sd3_through_tokenizers():
    from unigen_amd.text import encode_prompt_sd3
    seen = []

    def tok(tag):
        def call(prompt, max_length=None, **kw):
            seen.append((tag, list(prompt), max_length))
            return SimpleNamespace(input_ids=torch.full((len(prompt), max_length), 1 + len(prompt[0]), dtype=torch.long))
        return call
    cl, cg, t5 = _Clip(8, 4, 0.0), _Clip(16, 6, 0.0), _T5(32)
    e, ne, p, npool = encode_prompt_sd3([cl, cg, t5], [tok("l"), tok("g"), tok("t5")], ["ab", "ab"], prompt_3=["abcd", "abcd"], negative_prompt_2=["x", "x"],
                                        max_sequence_length=20)
    assert tuple(e.shape) == tuple(ne.shape) == (2, 97, 32) and tuple(p.shape) == (2, 10)
    assert seen[:3] == [("l", ["ab", "ab"], 77), ("g", ["ab", "ab"], 77), ("t5", ["abcd", "abcd"], 20)]      # prompt_2 defaults to prompt; T5 takes prompt_3
    assert seen[3:] == [("l", ["", ""], 77), ("g", ["x", "x"], 77), ("t5", ["", ""], 20)]                    # the negatives default to "" per prompt
    assert tuple(encode_prompt_sd3([cl, cg, t5], [tok("l"), tok("g"), tok("t5")], "one prompt")[0].shape) == (1, 77 + 256, 32)


# ---- the pipeline on stubs --------------------------------------------------------------------------------------------------------------------------
def _pipe(monkeypatch, **kw):
    from unigen_amd import pipeline as P
    seen = {}

    def loop(tr, **args):
        seen.update(args)
        return args["latents"]
    monkeypatch.setattr(P, "sd3_denoise_loop", loop)
    tr = SimpleNamespace(device=torch.device("cpu"), dtype=F32, config=SimpleNamespace(joint_attention_dim=32, in_channels=4, patch_size=2))
    return P.UniGenSD3Pipeline(transformer=tr, **kw), seen


def test_sd3_pipeline_prompt_precedence_and_cfg(monkeypatch):
    from unigen_amd.pipeline import UniGenSD3Pipeline
    from unigen_amd.text import encode_condition_prompt_sd3, encode_prompt_sd3
    params = list(inspect.signature(UniGenSD3Pipeline.__init__).parameters)
    assert params[:7] == ["self", "transformer", "scheduler_config", "vae_scale_factor", "encode_prompt", "vae", "image_processor"]       # the positional order stays
    assert params[7:] == ["text_encoder", "text_encoder_2", "text_encoder_3", "tokenizer", "tokenizer_2", "tokenizer_3"]
    call = inspect.signature(UniGenSD3Pipeline.__call__).parameters
    assert call["max_sequence_length"].default == 256 and all(call[k].default is None for k in ("prompt_2", "prompt_3", "negative_prompt", "negative_prompt_2",
                                                                                               "negative_prompt_3", "clip_skip"))
    cl, cg, t5 = _Clip(8, 4, 0.25), _Clip(16, 6, 0.5), _T5(32)
    got = UniGenSD3Pipeline.from_pretrained(None, transformer=None, text_encoder=cl, text_encoder_2=cg, text_encoder_3=t5, tokenizer="a", tokenizer_2="b",
                                            tokenizer_3="c", encode_prompt="d", vae="e", image_processor="f")
    assert (got.text_encoder, got.text_encoder_2, got.text_encoder_3, got.tokenizer, got.tokenizer_2, got.tokenizer_3) == (cl, cg, t5, "a", "b", "c")
    assert (got.encode_prompt, got.vae, got.image_processor) == ("d", "e", "f")

    pipe, seen = _pipe(monkeypatch, text_encoder=cl, text_encoder_2=cg, text_encoder_3=t5)
    ids, neg, cond = _ids(0), _ids(1), _ids(2)
    kw = dict(control_image=torch.zeros(2, 4, 8, 8), latents=torch.zeros(2, 4, 8, 8), num_inference_steps=1, max_sequence_length=12, return_dict=False)
    pipe(prompt=ids, condition_prompt=cond, negative_prompt=neg, guidance_scale=7.0, **kw)
    enc = [cl, cg, t5]
    e, ne, p, npool = encode_prompt_sd3(enc, [None] * 3, None, text_input_ids_list=ids, negative_text_input_ids_list=neg, max_sequence_length=12)
    cp = encode_condition_prompt_sd3(enc, [None] * 3, None, text_input_ids_list=cond, max_sequence_length=12)[1]
    assert torch.equal(seen["prompt_embeds"], torch.cat([ne, e])) and torch.equal(seen["pooled_prompt_embeds"], torch.cat([npool, p]))      # negatives first
    assert torch.equal(seen["condition_pooled_prompt_embeds"], torch.cat([cp, cp]))                                                        # doubled
    # without guidance: no negatives wanted, nothing doubled; clip_skip and num_images_per_prompt reach the encoders
    pipe(prompt=ids, condition_prompt=cond, guidance_scale=1.0, clip_skip=1, **kw)
    e1 = encode_prompt_sd3(enc, [None] * 3, None, do_classifier_free_guidance=False, clip_skip=1, text_input_ids_list=ids, max_sequence_length=12)[0]
    assert torch.equal(seen["prompt_embeds"], e1) and torch.equal(seen["pooled_prompt_embeds"], p) and torch.equal(seen["condition_pooled_prompt_embeds"], cp)
    with pytest.raises(ValueError, match="negative_text_input_ids_list"):
        pipe(prompt=ids, condition_prompt=cond, guidance_scale=7.0, **kw)
    for bad in (dict(prompt="a photo", condition_prompt=cond), dict(prompt=ids, condition_prompt="depth", negative_prompt=neg), dict(prompt=ids, condition_prompt=cond, negative_prompt="")):
        with pytest.raises(TypeError, match="token ids"):
            pipe(guidance_scale=7.0, **bad, **kw)
    # embeds that are passed in win over the encoders
    n_calls = len(cl.calls)
    E, PP = torch.ones(2, 5, 32), torch.ones(2, 10)
    pipe(prompt=ids, condition_prompt=cond, prompt_embeds=E, pooled_prompt_embeds=PP, condition_pooled_prompt_embeds=2 * PP, guidance_scale=1.0, **kw)
    assert len(cl.calls) == n_calls and torch.equal(seen["prompt_embeds"], E) and torch.equal(seen["condition_pooled_prompt_embeds"], 2 * PP)
    # an attached callable wins over the native encoders
    asked = []

    def hook(**args):
        asked.append(args)
        return 3 * E, 4 * E, 3 * PP, 4 * PP
    pipe.encode_prompt = hook
    pipe(prompt=ids, condition_prompt=cond, guidance_scale=7.0, **kw)
    assert len(cl.calls) == n_calls and len(asked) == 2 and asked[0]["do_classifier_free_guidance"] is True and asked[1]["do_classifier_free_guidance"] is False
    assert torch.equal(seen["prompt_embeds"], torch.cat([4 * E, 3 * E])) and torch.equal(seen["condition_pooled_prompt_embeds"], torch.cat([3 * PP, 3 * PP]))
    # nothing attached: the error names both ways out
    pipe.encode_prompt, pipe.text_encoder_2 = None, None
    with pytest.raises(NotImplementedError, match="encode_prompt") as err:
        pipe(prompt=ids, condition_prompt=cond, guidance_scale=1.0, **kw)
    assert all(name in str(err.value) for name in ("text_encoder`", "text_encoder_2", "text_encoder_3"))


def test_sd3_pipeline_through_tokenizers(monkeypatch):
    tok = lambda prompt, max_length=None, **kw: SimpleNamespace(input_ids=torch.full((len(prompt), max_length), 1 + len(prompt[0]), dtype=torch.long))
    cl, cg = _Clip(8, 4, 0.25), _Clip(16, 6, 0.5)
    pipe, seen = _pipe(monkeypatch, text_encoder=cl, text_encoder_2=cg, tokenizer=tok, tokenizer_2=tok)          # no T5: zeros of the transformer's width
    pipe(prompt=["ab", "ab"], condition_prompt=["depth", "depth"], negative_prompt_2=["x", "x"], guidance_scale=7.0, control_image=torch.zeros(2, 4, 8, 8),
         latents=torch.zeros(2, 4, 8, 8), num_inference_steps=1, max_sequence_length=9)
    assert tuple(seen["prompt_embeds"].shape) == (4, 77 + 9, 32) and not seen["prompt_embeds"][:, 77:].any()
    assert float(seen["prompt_embeds"][0, 0, 0]) == 1 + 2000.25 and float(seen["prompt_embeds"][2, 0, 0]) == 3 + 2000.25       # "" first, then "ab"
    assert float(seen["prompt_embeds"][0, 0, 8]) == 2 + 2000.5                                                                  # negative_prompt_2 = "x"
    assert float(seen["condition_pooled_prompt_embeds"][0, 0]) == 6.25 and tuple(seen["condition_pooled_prompt_embeds"].shape) == (4, 10)
