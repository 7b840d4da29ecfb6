"""One `estimate_depth` of a 1024 x 1024 image with depth-anything-small's geometry (synthetic weights): the processor (PIL BICUBIC to 518 x 518 and
the patch rows), the DINOv2 backbone, the DPT neck and head, the bicubic resize back to 1024 x 1024 and the uint8 map, each stage timed with HIP
events after warm-up, and the whole call. The yardstick printed beside it is one `vae.encode` of the same image on the same visit, the stage the
condition image feeds (as tools/image_bench.py does).

    python tools/depth_bench.py [--size 1024] [--iters 10] [--out profiles/depth_bench.log]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from unigen_amd import ops
    from unigen_amd.depth import DepthAnythingForDepthEstimation, DepthImageProcessor, estimate_depth
    from unigen_amd.image import VaeImageProcessor
    from unigen_amd.vae import AutoencoderKL
    dev, BF = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(float(a.size)), torch.arange(float(a.size)), indexing="ij")
    img = torch.stack([128 + 100 * torch.sin(0.02 * yy + 0.013 * xx + c) for c in range(3)], -1) + 30 * torch.randn(a.size, a.size, 3, generator=g)
    img = img.clamp(0, 255).to(torch.uint8).to(dev)
    model = DepthAnythingForDepthEstimation(device=dev, dtype=BF).init_synthetic_(0)
    proc = DepthImageProcessor(device=dev)
    rec = dict(size=a.size, model_side=proc.output_size(a.size, a.size)[0], dtype="bf16")
    patches, grid, (H, W) = proc.preprocess(img, dtype=BF)
    B, (ph, pw) = 1, grid
    feats = model.backbone(patches, B, ph, pw)
    depth = model.neck_and_head(feats, B, ph, pw)
    up = ops.bicubic_f32(depth, H, W)
    rec["preprocess_ms"] = timed(lambda: proc.preprocess(img, dtype=BF), a.iters)
    rec["backbone_ms"] = timed(lambda: model.backbone(patches, B, ph, pw), a.iters)
    rec["neck_head_ms"] = timed(lambda: model.neck_and_head(feats, B, ph, pw), a.iters)
    rec["bicubic_ms"] = timed(lambda: ops.bicubic_f32(depth, H, W), a.iters)
    rec["minmax_u8_ms"] = timed(lambda: ops.minmax_to_u8(up, 3), a.iters)
    rec["estimate_depth_ms"] = timed(lambda: estimate_depth(model, img, proc), a.iters)
    rec["positive_share"] = round(float((depth > 0).float().mean()), 3)
    vae = AutoencoderKL(device=dev, dtype=BF)
    vae.init_synthetic_(seed=0)
    x = VaeImageProcessor(vae_scale_factor=16).preprocess(img).to(BF)
    rec["vae_encode_ms"] = timed(lambda: vae.encode(x), max(a.iters // 2, 2))
    line = "DEPTH_BENCH " + json.dumps(rec)
    print(line)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
