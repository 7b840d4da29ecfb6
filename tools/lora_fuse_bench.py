"""What a LoRA file costs to load, merge and take out again, and what the forward costs with the adapter live, merged and absent: UniGenFlux at
FLUX-schnell geometry (1024^2, random weights) with a rank-R "all linear" adapter in the kohya naming - attention, MLPs, img_mod / txt_mod / modulation,
the embedders and the final layer of every base block - written to a safetensors file first, so that load_lora_weights is timed from disk.
  load_lora_weights | fuse_lora (backup on the device) | unfuse_lora | forward: adapter absent / live (LORA_CAPABLE sites only) / merged, interleaved.
The merged and the absent forward run the same launches; after unfuse_lora the forward must give the adapter-free bits again.
    python tools/lora_fuse_bench.py [--batch 1] [--rank 16]"""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safetensors.torch import save_file
from unigen_amd.flux import UniGenFlux
from unigen_amd.pipeline import prepare_latent_image_ids
import bench

ap = argparse.ArgumentParser(); ap.add_argument("--batch", type=int, default=1); ap.add_argument("--rank", type=int, default=16); a = ap.parse_args()
dev, BF = torch.device("cuda:0"), torch.bfloat16
B, grid, T, r = a.batch, 64, 512, a.rank
m = UniGenFlux.from_config({}, device=dev, dtype=BF)
m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(bench.CONTROL_PARAMS))
m.init_synthetic_(seed=0, std=0.02)
cfg, D = m.config, m.inner_dim
g = torch.Generator(device=dev).manual_seed(12443)
rn = lambda *s: torch.randn(*s, generator=g, device=dev)
N = grid * grid
ids, txt = prepare_latent_image_ids(grid, grid, dev, BF), torch.zeros(T, 3, device=dev, dtype=BF)
kw = dict(hidden_states=rn(B, N, 64).to(BF), condition_hidden_states=rn(B, N, 64).to(BF), encoder_hidden_states=(0.1 * rn(B, T, cfg.joint_attention_dim)).to(BF),
          pooled_projections=rn(B, cfg.pooled_projection_dim).to(BF), condition_pooled_projections=rn(B, cfg.pooled_projection_dim).to(BF),
          timestep=torch.full((B,), 0.75, device=dev, dtype=BF), img_ids=ids, txt_ids=txt, condition_ids=ids, gate_uniform=torch.rand(B * N, m._ctl.expert_nums, generator=g, device=dev))
if cfg.guidance_embeds:
    kw["guidance"] = torch.full((B,), 3.5, device=dev, dtype=BF)

# kohya names -> (rows, columns) of the BFL module
shapes = {}
for i in range(cfg.num_layers):
    for s in ("img", "txt"):
        p = f"lora_unet_double_blocks_{i}_{s}_"
        shapes.update({p + "attn_qkv": (3 * D, D), p + "attn_proj": (D, D), p + "mlp_0": (4 * D, D), p + "mlp_2": (D, 4 * D), p + "mod_lin": (6 * D, D)})
for i in range(cfg.num_single_layers):
    p = f"lora_unet_single_blocks_{i}_"
    shapes.update({p + "linear1": (7 * D, D), p + "linear2": (D, 5 * D), p + "modulation_lin": (3 * D, D)})
shapes.update({"lora_unet_img_in": (D, cfg.in_channels), "lora_unet_txt_in": (D, cfg.joint_attention_dim), "lora_unet_time_in_in_layer": (D, 256),
               "lora_unet_time_in_out_layer": (D, D), "lora_unet_vector_in_in_layer": (D, cfg.pooled_projection_dim), "lora_unet_vector_in_out_layer": (D, D),
               "lora_unet_final_layer_linear": (m.out_channels, D), "lora_unet_final_layer_adaLN_modulation_1": (2 * D, D)})
sd = {}
for k, (n_out, k_in) in shapes.items():
    sd[k + ".lora_down.weight"] = (rn(r, k_in) / k_in ** 0.5).to(BF).cpu()
    sd[k + ".lora_up.weight"] = (rn(n_out, r) * 0.02).to(BF).cpu()
    sd[k + ".alpha"] = torch.tensor(float(r), dtype=torch.float16)
tmp = tempfile.mkdtemp(prefix="lora_fuse_bench_")
path = os.path.join(tmp, "all_linear.safetensors")
save_file(sd, path)
file_mb = os.path.getsize(path) / 2 ** 20
live_only = {k: v for k, v in sd.items() if not any(x in k for x in ("mod_lin", "modulation_lin", "_in.", "_in_", "final_layer"))}
del sd


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fwd(n=3):
    out = m(**kw)[0]; torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t, out = wall(lambda: m(**kw)[0]); ts.append(t)
    return min(ts), out.clone()


res, fw = {}, {"absent": [], "live": [], "merged": []}
t, out0 = fwd(); fw["absent"].append(t)
for rep in range(2):
    res["load_lora_weights_s"], report = wall(lambda: m.load_lora_weights(path, adapter_name="style"))
    res["fuse_lora_s"], touched = wall(lambda: m.fuse_lora())
    backup_gb = sum(v.numel() * v.element_size() for v in m._lora_backup.values()) / 1e9
    t, out_m = fwd(); fw["merged"].append(t)
    res["unfuse_lora_s"], _ = wall(lambda: m.unfuse_lora())
    m.unload_lora_weights("style")
    t, out_a = fwd(); fw["absent"].append(t)
    assert torch.equal(out_a, out0), "after unfuse_lora + unload_lora_weights the forward must give the adapter-free bits"
    rep_live = m.load_lora_weights(live_only, adapter_name="style")
    assert not rep_live.merge_only
    t, out_l = fwd(); fw["live"].append(t)
    m.unload_lora_weights("style")
assert torch.isfinite(out_m.float()).all() and not torch.equal(out_m, out0) and not torch.equal(out_l, out0)
best = {k: min(v) for k, v in fw.items()}
print("LORA_FUSE_BENCH", json.dumps(dict(
    workload=f"UniGenFlux (schnell geometry, 1 condition), 1024^2, B={B}, one forward; rank-{r} all-linear kohya file, {file_mb:.0f} MiB: "
             f"{len(report.live)} live-capable + {len(report.merge_only)} merge-only modules, {len(touched)} weights merged",
    **res, backup_on_device_gb=backup_gb, forward_s=best, forward_all_s=fw,
    live_over_absent_pct=100.0 * (best["live"] / best["absent"] - 1.0), merged_over_absent_pct=100.0 * (best["merged"] / best["absent"] - 1.0))))
os.remove(path); os.rmdir(tmp)
