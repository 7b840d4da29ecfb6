"""Writes tests/golden/depth_tiny.safetensors: what the installed transformers library computes on the tiny Depth Anything model of
tests/depth_ref.py (DepthAnythingForDepthEstimation, DPTImageProcessorPil, the depth-estimation pipeline's post-processing), on the CPU with random
weights. Needs transformers and PIL; no download (HF_HUB_OFFLINE=1).

    python tests/golden/make_depth_golden.py

The weights (1.62 M parameters) are NOT stored: a committed file stays below 1 MiB, so tests regenerate them with depth_ref.random_state (seeded,
rounded to bf16 before the oracle runs) and check them against the stored fingerprint. Per case (B = 2; 28x28, 56x42, 70x98) the file holds the
float64 run's tensors as fp32 - all stages for 28x28, all but the largest fused map for 56x42, a subset for 70x98 - and, for EVERY stage of every case, the rel-L2 error of
transformers' own fp32 and bf16 runs against its float64 run: the yardsticks of tests/test_depth_gpu.py. Position interpolation runs in fp32 inside
every run (Dinov2Embeddings casts), everything else in the run's dtype. It also holds two images with the processor's pixel_values, PIL's BICUBIC
bytes and the pipeline's output for a stored depth map, and the measured constants `c` of the rounding kernels' bounds (torch in fp32 on the CPU
against float64 on the cases of the GPU test, docs/PARITY_TOLERANCES.md "Depth model").
"""
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import depth_ref as R  # noqa: E402

ALL = ["embeddings"] + [f"{g}.{i}" for g in ("feature_maps", "reassembled", "fused") for i in range(4)] + ["predicted_depth"]
STORED = {"g2x2": ALL, "g4x3": [k for k in ALL if k != "fused.3"],          # the largest maps stay out: the file is held below 1 MiB
          "g5x7": ["embeddings", "feature_maps.3", "reassembled.2", "reassembled.3", "fused.0", "predicted_depth"]}


def hf_model(cfg, sd):
    import transformers
    b = {k: v for k, v in cfg["backbone_config"].items() if k != "model_type"}
    bc = transformers.Dinov2Config(**b)
    top = {k: v for k, v in cfg.items() if k != "backbone_config"}
    m = transformers.DepthAnythingForDepthEstimation(transformers.DepthAnythingConfig(backbone_config=bc, **top)).eval()
    have = m.state_dict()
    assert set(have) == set(sd), (set(have) ^ set(sd))
    assert all(tuple(have[k].shape) == tuple(sd[k].shape) for k in sd)
    m.load_state_dict({k: v.float() for k, v in sd.items()})
    return m


def hf_stages(m, pv):
    """One run of transformers' model -> the dict layout of depth_ref.forward."""
    got = {}
    hooks = [m.backbone.embeddings.register_forward_hook(lambda mod, i, o: got.__setitem__("embeddings", o)),
             m.backbone.register_forward_hook(lambda mod, i, o: got.__setitem__("feature_maps", list(o.feature_maps))),
             m.neck.reassemble_stage.register_forward_hook(lambda mod, i, o: got.__setitem__("reassembled", list(o))),
             m.neck.fusion_stage.register_forward_hook(lambda mod, i, o: got.__setitem__("fused", list(o)))]
    with torch.no_grad():
        got["predicted_depth"] = m(pixel_values=pv.to(next(m.parameters()).dtype)).predicted_depth
    for h in hooks:
        h.remove()
    return got


def kernel_constants():
    """c = max |torch fp32 - float64| / (2^-24 * scale) over the GPU test's cases, per rounding kernel."""
    out = {}
    for name, cases in R.kernel_cases().items():
        worst = 0.0
        for case in cases:
            t64, scale = R.kernel_truth(name, case, torch.float64)
            t32, _ = R.kernel_truth(name, case, torch.float32)
            worst = max(worst, float(((t32.double() - t64).abs() / (2.0 ** -24 * scale)).max()))
        out[name] = worst
    return out


def image_cases(seed, proc, m64, m32, Image, get_resize_output_image_size):
    """The two images (60x100, 45x33) with the processor's and the pipeline's outputs on them."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for tag, (H, W) in (("img0", (60, 100)), ("img1", (45, 33))):
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        img = torch.stack([128 + 90 * torch.sin(0.13 * yy + 0.09 * xx + c) for c in range(3)], -1) + 30 * torch.randn(H, W, 3, generator=g)
        img = img.clamp(0, 255).to(torch.uint8)
        pil = Image.fromarray(img.numpy())
        pv = torch.from_numpy(np.asarray(proc(images=pil, return_tensors="np")["pixel_values"]))
        h, w = pv.shape[-2:]
        want = get_resize_output_image_size(np.zeros((3, H, W)), (56, 56), True, 14)
        assert (h, w) == (want.height, want.width)
        out[f"{tag}.u8"], out[f"{tag}.pixel_values"] = img, pv.float().contiguous()
        out[f"{tag}.bicubic"] = torch.from_numpy(np.array(pil.resize((w, h), Image.BICUBIC)))
        # the pipeline on transformers' own predicted depth in float64 (cast to fp32: the stored map), fp32 and bf16
        d64, d32 = (hf_stages(m, pv)["predicted_depth"][0] for m in (m64, m32))
        stored = d64.float()
        res = proc.post_process_depth_estimation(type("O", (), {"predicted_depth": stored[None]})(), [(H, W)])[0]["predicted_depth"]
        a = res.numpy()
        a = (a - a.min()) / (a.max() - a.min())
        depth_u8 = torch.from_numpy((a * 255).astype("uint8"))
        out[f"{tag}.depth_in"], out[f"{tag}.depth_up"], out[f"{tag}.depth_u8"] = stored.contiguous(), res.contiguous(), depth_u8
        # the share of pixels by which transformers' fp32 run differs from its float64 run after the same post-processing
        _, u32 = R.postprocess(d32.float(), H, W)
        out[f"{tag}.share_fp32"] = torch.tensor([float((u32 != depth_u8).double().mean()), float((u32.int() - depth_u8.int()).abs().max())], dtype=torch.float64)
    return out


def main():
    from PIL import Image
    from safetensors.torch import save_file
    from transformers.models.dpt.image_processing_pil_dpt import DPTImageProcessorPil, get_resize_output_image_size
    sd = R.random_state(R.TINY)
    out = {"w.fingerprint": R.fingerprint(sd)}
    m64, m32, m16 = hf_model(R.TINY, sd).double(), hf_model(R.TINY, sd), hf_model(R.TINY, sd).to(torch.bfloat16)
    for name in R.CASES:
        u8 = R.case_images(name)
        pv = R.pixel_values(u8)
        s64, s32, s16 = (R.stage_list(hf_stages(m, pv)) for m in (m64, m32, m16))
        d = s64[-1][1]
        pos, spread = float((d > 0).double().mean()), float(d.max() - d.min())
        assert 0.3 <= pos <= 0.98 and spread > 1, (name, pos, spread)               # a dead head must not pass
        errs = []
        for (k, a), (_, b), (_, c) in zip(s64, s32, s16):
            if k in STORED[name]:
                out[f"{name}.{k}"] = a.float().contiguous()
            errs.append([R.rel_l2(b, a), R.rel_l2(c, a)])
        out[f"{name}.err"] = torch.tensor(errs, dtype=torch.float64)                  # [stage, (fp32, bf16)] in stage_list order
        print(name, f"positive {pos:.2f} max {float(d.max()):.1f}  predicted_depth rel-L2 fp32 {errs[-1][0]:.2e} bf16 {errs[-1][1]:.2e}")
    # the image processor and the pipeline's post-processing on two images
    proc = DPTImageProcessorPil(size={"height": 56, "width": 56}, keep_aspect_ratio=True, ensure_multiple_of=14, do_resize=True, do_rescale=True,
                                do_normalize=True, image_mean=list(R.IMAGENET_MEAN), image_std=list(R.IMAGENET_STD))
    # A yardstick of zero differing pixels would admit no rounding at all, which no fp32 run can promise (transformers' own differs in 0 or 1 pixel
    # per image, depending on the noise): take the first noise seed at which its fp32 run differs from its float64 run on BOTH images.
    for seed in range(77, 400):
        img_out = image_cases(seed, proc, m64, m32, Image, get_resize_output_image_size)
        if all(float(img_out[f"{tag}.share_fp32"][0]) > 0 for tag in ("img0", "img1")):
            break
    else:
        raise AssertionError("no seed gives an informative yardstick")
    print("image noise seed", seed)
    out.update(img_out)
    out["img.seed"] = torch.tensor([seed], dtype=torch.int32)
    c = kernel_constants()
    out["c.names"] = torch.tensor([ord(ch) for ch in ",".join(sorted(c))], dtype=torch.uint8)
    out["c.values"] = torch.tensor([c[k] for k in sorted(c)], dtype=torch.float64)
    print("kernel constants", c)
    path = os.path.join(HERE, "depth_tiny.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= (1 << 20)


if __name__ == "__main__":
    main()
