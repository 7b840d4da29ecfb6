"""unigen_amd/lora_io.py on the host: the three key forms (diffusers / PEFT, kohya, BFL-dotted) written by tests/lora_io_ref.py and read back through
`convert` - tensors and alphas exactly - every row of the BFL map, the live / merge-only partition, the refusals, and the reference's save hook
round trip (src/hook.py:29-70). No GPU."""
import importlib

import pytest
import torch

from tests import lora_io_ref as LR
from unigen_amd import lora_io

BF = torch.bfloat16
TINY = dict(num_layers=2, num_single_layers=4, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64)
SD3_TINY = dict(sample_size=16, num_layers=3, attention_head_dim=64, num_attention_heads=2, joint_attention_dim=64, caption_projection_dim=128,
                pooled_projection_dim=64, pos_embed_max_size=12, dual_attention_layers=(0, 1))
CONTROL = dict(use_rope=True, use_shared_expert=True, use_single_trans_blocks=True, single_control_dev=2, single_block_control_method="overall_add",
               top_num=1, expert_num_each_condition=3)


def _shapes(model):
    return {n[:-len(".weight")]: tuple(p.shape) for n, p in model.named_parameters() if n.endswith(".weight") and p.dim() == 2}


@pytest.fixture(scope="module")
def flux():
    T = importlib.import_module("src.UniGenTransformer")
    out = {}
    for cls in ("UniGenFlux", "MultiCondtionUniGenFlux"):
        m = getattr(T, cls).from_config(dict(TINY), device="cpu", dtype=BF)
        m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
        out[cls] = m
    m = out["UniGenFlux"]
    bfl, canon = LR.make_bfl_adapter(_shapes(m), LR.bfl_modules(TINY["num_layers"], TINY["num_single_layers"]), seed=3)
    return out, bfl, canon


@pytest.fixture(scope="module")
def sd3():
    m = importlib.import_module("src.UniGenTransformer").UniGenSD3.from_config(dict(SD3_TINY), device="cpu", dtype=BF)
    m.init_condition_block(condition_nums=1, condition_types=["depth"], control_params=dict(use_shared_expert=True, use_modulate=False))
    return m


def _same(got, canon):
    assert set(got) == set(canon), (sorted(set(got) ^ set(canon))[:6])
    for k, (A, B, alpha) in canon.items():
        a, b, al = got[k]
        assert torch.equal(a.float(), A) and torch.equal(b.float(), B), k
        assert al == alpha, (k, al, alpha)


def test_map_covers_every_row_and_kind_of_split(flux):
    _, bfl, canon = flux
    D = TINY["attention_head_dim"] * TINY["num_attention_heads"]
    down, up, _ = bfl["double_blocks.1.img_attn.qkv"]
    for j, leaf in enumerate(("to_q", "to_k", "to_v")):                                     # thirds, one shared lora_down
        A, B, _ = canon[f"transformer_blocks.1.attn.{leaf}"]
        assert A is down and torch.equal(B, up[j * D:(j + 1) * D])
    down, up, _ = bfl["double_blocks.0.txt_attn.qkv"]
    assert torch.equal(canon["transformer_blocks.0.attn.add_k_proj"][1], up[D:2 * D])
    down, up, _ = bfl["single_blocks.2.linear1"]                                            # [D, D, D, 4 D]
    assert up.shape[0] == 7 * D
    assert torch.equal(canon["single_transformer_blocks.2.attn.to_v"][1], up[2 * D:3 * D])
    assert torch.equal(canon["single_transformer_blocks.2.proj_mlp"][1], up[3 * D:])
    down, up, _ = bfl["final_layer.adaLN_modulation.1"]                                     # (shift, scale) -> (scale, shift)
    assert torch.equal(canon["norm_out.linear"][1], torch.cat([up[D:], up[:D]], 0))
    rows = {leaf for t in (LR.BFL_DOUBLE, LR.BFL_SINGLE) for v in t.values() for leaf in v} | set(LR.BFL_TOP.values())
    hit = {leaf for leaf in rows if any(m == leaf or m.endswith("." + leaf) for m in canon)}
    assert rows - hit == {x for x in rows if "guidance_embedder" in x}                      # schnell geometry: no guidance embedder


@pytest.mark.parametrize("cls", ["UniGenFlux", "MultiCondtionUniGenFlux"])
@pytest.mark.parametrize("naming", ["kohya_f16", "kohya_bf16", "bfl", "bfl_bare", "diffusers", "peft", "down_up", "legacy"])
def test_each_naming_converts_exactly(flux, cls, naming):
    models, bfl, canon = flux
    model = models[cls]
    sd = {"kohya_f16": lambda: LR.write_kohya(bfl, torch.float16), "kohya_bf16": lambda: LR.write_kohya(bfl, BF),
          "bfl": lambda: LR.write_bfl(bfl), "bfl_bare": lambda: LR.write_bfl(bfl, prefix=""),
          "diffusers": lambda: LR.write_diffusers(canon), "peft": lambda: LR.write_diffusers(canon, prefix="base_model.model.", adapter="default"),
          "down_up": lambda: LR.write_diffusers(canon, prefix="", sides=("lora_down", "lora_up")),
          "legacy": lambda: LR.write_diffusers(canon, sides=("lora.down", "lora.up"))}[naming]()
    if naming.startswith("kohya"):
        assert all(v.dim() == 0 for k, v in sd.items() if k.endswith(".alpha")) and any(k.endswith(".alpha") for k in sd)
    assert any(v[2] is None for v in canon.values()) and any(v[2] is not None for v in canon.values())      # alpha present and absent
    got, rep = lora_io.convert(sd, model)
    _same(got, canon)
    assert set(rep.live) == {m for m in canon if model.lora_capable(m)} and set(rep.merge_only) == set(canon) - set(rep.live)
    assert rep.live and rep.merge_only and not rep.ignored
    assert {"transformer_blocks.0.norm1.linear", "single_transformer_blocks.3.norm.linear", "x_embedder", "proj_out", "norm_out.linear",
            "time_text_embed.timestep_embedder.linear_1", "single_transformer_blocks.0.proj_out"} - set(rep.merge_only) == {"single_transformer_blocks.0.proj_out"}
    flat = lora_io.lora_state_dict(sd)                                                     # the diffusers form, whatever the file used
    assert set(flat) == {f"transformer.{m}.lora_{s}.weight" for m in canon for s in "AB"} | {f"transformer.{m}.alpha" for m, v in canon.items() if v[2] is not None}
    for m, (A, B, alpha) in canon.items():
        assert torch.equal(flat[f"transformer.{m}.lora_A.weight"].float(), A) and torch.equal(flat[f"transformer.{m}.lora_B.weight"].float(), B)
        if alpha is not None:
            assert float(flat[f"transformer.{m}.alpha"]) == alpha


def test_sd3_diffusers_names_and_refusal_of_bfl_names(sd3, flux):
    _, bfl, _ = flux
    shapes = _shapes(sd3)
    mods = ["transformer_blocks.0.attn.to_q", "transformer_blocks.1.attn2.to_out.0", "transformer_blocks.2.ff.net.2", "transformer_blocks.0.norm1.linear",
            "context_embedder", "time_text_embed.timestep_embedder.linear_1", "proj_out", "norm_out.linear", "control_transformer_blocks.0.attn.to_k"]
    g = torch.Generator().manual_seed(1)
    canon = {m: (torch.randn(4, shapes[m][1], generator=g).to(BF).float(), torch.randn(shapes[m][0], 4, generator=g).to(BF).float(), 8.0 if i % 2 else None)
             for i, m in enumerate(mods)}
    got, rep = lora_io.convert(LR.write_diffusers(canon), sd3)
    _same(got, canon)
    assert set(rep.live) == {m for m in mods if sd3.lora_capable(m)} == {mods[0], mods[1], mods[2], mods[8]}
    with pytest.raises(KeyError, match="lora_unet_double_blocks_0_img_attn_qkv"):
        lora_io.convert(LR.write_kohya({"double_blocks.0.img_attn.qkv": bfl["double_blocks.0.img_attn.qkv"]}), sd3)
    with pytest.raises(KeyError, match="pos_embed.proj"):                                   # a convolution is not a linear projection
        lora_io.convert({"transformer.pos_embed.proj.lora_A.weight": torch.zeros(4, 16), "transformer.pos_embed.proj.lora_B.weight": torch.zeros(128, 4)}, sd3)


def test_text_encoder_keys_are_reported_not_dropped(flux):
    models, bfl, canon = flux
    sd = LR.write_kohya(bfl)
    te = {"lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8), "lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_up.weight": torch.zeros(8, 4),
          "lora_te1_text_model_encoder_layers_0_mlp_fc1.alpha": torch.tensor(4.0), "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight": torch.zeros(4, 8),
          "text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_B.weight": torch.zeros(8, 4)}
    sd.update(te)
    got, rep = lora_io.convert(sd, models["UniGenFlux"])
    _same(got, canon)
    assert sorted(rep.ignored) == sorted(te)
    assert set(te) <= set(lora_io.lora_state_dict(sd))


@pytest.mark.parametrize("key,exc", [
    ("transformer.transformer_blocks.0.attn.to_q.dora_scale", KeyError), ("transformer.transformer_blocks.0.attn.to_q.lora_magnitude_vector.weight", KeyError),
    ("lora_unet_double_blocks_0_img_attn_qkv.dora_scale", KeyError), ("lora_unet_double_blocks_0_img_attn_qkv.hada_w1_a", KeyError),
    ("lora_unet_double_blocks_0_img_attn_qkv.lokr_w1", KeyError), ("diffusion_model.double_blocks.0.img_attn.qkv.diff", KeyError),
    ("diffusion_model.double_blocks.0.img_attn.qkv.diff_b", KeyError), ("transformer.transformer_blocks.0.attn.norm_q.weight", KeyError),
    ("transformer.transformer_blocks.0.attn.to_q.lora_B.bias", KeyError), ("lora_unet_double_blocks_0_img_attn_norm_query_norm.lora_down.weight", KeyError),
    ("lora_unet_double_blocks_0_img_attnqkv.alpha", KeyError), ("diffusion_model.double_blocks.0.img_attn.norm.query_norm.lora_A.weight", KeyError),
    ("transformer.processor.qkv_lora1.down.weight", KeyError),
])
def test_unrecognised_keys_are_refused_by_name(flux, key, exc):
    models, _, canon = flux
    sd = LR.write_diffusers({k: canon[k] for k in ["transformer_blocks.1.attn.to_k"]})
    sd[key] = torch.zeros(4, 256)
    if key.endswith("lora_A.weight") or key.endswith("lora_down.weight"):
        sd[key.replace("lora_A", "lora_B").replace("lora_down", "lora_up")] = torch.zeros(256, 4)
    with pytest.raises(exc) as ei:
        lora_io.convert(sd, models["UniGenFlux"])
    assert key in str(ei.value) or key.replace("lora_A", "lora_B") in str(ei.value)


def test_shape_rank_and_model_mismatches_name_the_key(flux):
    models, _, canon = flux
    model = models["UniGenFlux"]
    m = "transformer_blocks.1.attn.to_k"
    A, B, _ = canon[m]
    bad = {f"transformer.{m}.lora_A.weight": A, f"transformer.{m}.lora_B.weight": B[:, :-1]}
    with pytest.raises(ValueError, match=r"transformer\.transformer_blocks\.1\.attn\.to_k\.lora_B\.weight"):
        lora_io.convert(bad, model)
    with pytest.raises(ValueError, match=r"transformer_blocks\.1\.attn\.to_k"):
        lora_io.convert({f"transformer.{m}.lora_A.weight": A[:, :-8], f"transformer.{m}.lora_B.weight": B}, model)
    with pytest.raises(KeyError, match="lora_A / lora_down"):
        lora_io.convert({f"transformer.{m}.lora_B.weight": B}, model)
    gone = {"transformer.transformer_blocks.7.attn.to_k.lora_A.weight": A, "transformer.transformer_blocks.7.attn.to_k.lora_B.weight": B}
    with pytest.raises(KeyError, match=r"transformer_blocks\.7\.attn\.to_k"):
        lora_io.convert(gone, model)
    got, rep = lora_io.convert(gone, model, strict=False)
    assert not got and rep.ignored == ["transformer_blocks.7.attn.to_k"]
    with pytest.raises(ValueError, match="alpha"):
        lora_io.convert({f"transformer.{m}.lora_A.weight": A, f"transformer.{m}.lora_B.weight": B, f"transformer.{m}.alpha": torch.ones(2)}, model)


def test_read_lora_file_forms(tmp_path, flux):
    from safetensors.torch import save_file
    _, _, canon = flux
    sd = LR.write_diffusers({k: canon[k] for k in list(canon)[:3]})
    save_file(sd, str(tmp_path / "a.safetensors"))
    (tmp_path / "d").mkdir()
    save_file(sd, str(tmp_path / "d" / lora_io.LORA_FILE))
    torch.save(sd, str(tmp_path / "a.bin"))
    torch.save({"state_dict": sd}, str(tmp_path / "a.pt"))
    for p in ("a.safetensors", "d", "a.bin", "a.pt"):
        got = lora_io.read_lora_file(tmp_path / p)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd), p
    with pytest.raises(OSError):
        lora_io.read_lora_file(tmp_path / "missing.safetensors")
    (tmp_path / "e").mkdir()
    with pytest.raises(OSError, match=lora_io.LORA_FILE):
        lora_io.read_lora_file(tmp_path / "e")
    (tmp_path / "a.txt").write_text("x")
    with pytest.raises(ValueError):
        lora_io.read_lora_file(tmp_path / "a.txt")


def test_load_save_round_trip_is_the_reference_hook_format(tmp_path, flux):
    """load_lora_weights (host part: attach live sites, keep merge-only entries) -> save_lora_weights -> read_lora_file -> lora_state_dict gives exactly
    the keys the reference's load hook filters for (src/hook.py:63-67: `transformer.` prefix, "lora" in k) and the same tensors; unload leaves no trace."""
    from unigen_amd import lib as L
    from unigen_amd.pipeline import UniGenFLUXPipeline
    T = importlib.import_module("src.UniGenTransformer")
    model = T.UniGenFlux.from_config(dict(TINY), device="cpu", dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
    _, bfl, canon = flux
    names0 = [n for n, _ in model.named_parameters()]
    pipe = UniGenFLUXPipeline(transformer=model)
    rep = pipe.load_lora_weights(LR.write_kohya(bfl), adapter_name="style")
    assert set(rep.live) == set(model._lora_sites) and set(rep.merge_only) == set(model._lora_merge_only["style"])
    for m in rep.live:
        lay = model._lora_sites[m]
        A, B, alpha = canon[m]
        assert lay.r["style"] == A.shape[0] and lay.lora_alpha["style"] == (alpha if alpha is not None else A.shape[0]) and lay.scaling["style"] == LR.scaling(canon[m])
        assert torch.equal(lay.lora_A["style"].weight.float(), A) and torch.equal(lay.lora_B["style"].weight.float(), B)
    with pytest.raises(L.UniGenHipError, match="fuse_lora"):                                # the guard sits before any device work
        model(torch.zeros(1, 4, 64))
    path = lora_io.save_lora_weights(tmp_path / "style", model, "style")
    assert path.endswith(lora_io.LORA_FILE)
    flat = UniGenFLUXPipeline.lora_state_dict(str(tmp_path / "style"))
    hook = {k.replace("transformer.", ""): v for k, v in flat.items() if k.startswith("transformer.") and "lora" in k}
    assert set(hook) == {f"{m}.lora_{s}.weight" for m in canon for s in "AB"}
    for m, (A, B, alpha) in canon.items():
        assert torch.equal(hook[f"{m}.lora_A.weight"].float(), A) and torch.equal(hook[f"{m}.lora_B.weight"].float(), B)
        assert float(flat[f"transformer.{m}.alpha"]) == (alpha if alpha is not None else A.shape[0])
    with pytest.raises(L.UniGenHipError, match="already covers"):
        model.load_lora_weights(LR.write_kohya(bfl), adapter_name="style")
    pipe.unload_lora_weights()
    assert not model._lora_sites and not model._lora_merge_only and [n for n, _ in model.named_parameters()] == names0
    assert not any(hasattr(m, "lora_A") for m in model.modules())


def test_a_failed_load_leaves_nothing_attached(flux, monkeypatch):
    """A failure part-way through the rank groups (here: the second add_lora call) rolls back the sites the first ones attached; a module name that
    is also the tail of a deeper module's name is refused before anything is attached."""
    from unigen_amd import lib as L
    T = importlib.import_module("src.UniGenTransformer")
    model = T.UniGenFlux.from_config(dict(TINY), device="cpu", dtype=BF)
    model.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
    _, bfl, canon = flux
    names0 = [n for n, _ in model.named_parameters()]
    real, calls = model.add_lora, []

    def flaky(*a, **k):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("boom")
        return real(*a, **k)

    monkeypatch.setattr(model, "add_lora", flaky)
    with pytest.raises(RuntimeError, match="boom"):
        model.load_lora_weights(LR.write_kohya(bfl), adapter_name="style")
    assert len(calls) == 2 and not model._lora_sites and not model._lora_merge_only and [n for n, _ in model.named_parameters()] == names0
    monkeypatch.setattr(model, "add_lora", real)
    from unigen_amd.engine import _register
    _register(model, "x.transformer_blocks.1.attn.to_k.weight", (256, 256), "cpu", BF)     # a deeper module with the same tail as a file entry
    m = "transformer_blocks.1.attn.to_k"
    with pytest.raises(L.UniGenHipError, match="suffix"):
        model.load_lora_weights(LR.write_diffusers({m: canon[m]}), adapter_name="style")
    assert not model._lora_sites
