"""Image front end at 1024 x 1024 x 3, B = 1 and B = 8: time (HIP events after warm-up) and bytes moved per second of ug_canny_u8 (with its sweep count
and the three stages apart), ug_img_resize_u8 from 1536^2 to 1024^2, the two converters and ug_img_box_blur_u8 as PIL's GaussianBlur(10) (the "deblurring" condition), fused
(all three passes of an axis in one launch) against fuse=0 (one launch per pass), the two interleaved in one process.

    python tools/image_bench.py [--size 1024] [--batches 1 8] [--steps blur] [--out profiles/NAME.log]

Each step runs in a fresh child process under its own time limit (`--step NAME` is what a child runs); a step that fails or runs out of time ends the
run - nothing more is started on the GPU after it. The yardstick to read the numbers against is one `vae.encode` of the same image
(tools/vae_bench.py, same visit): the stage this front end feeds. Bytes are the algorithm's: every input read once, every output written once.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ["canny", "canny_stages", "resize", "u8_to_chw", "chw_to_u8", "blur"]
STEP_SECONDS = 120


def timed(fn, iters=20, warmup=3):
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
    return e0.elapsed_time(e1) / iters


def run_step(step, size, B):
    import numpy as np
    import torch
    from tests.image_ref import synth
    from unigen_amd import ops
    from unigen_amd.image import resize_u8
    dev = torch.device("cuda:0")
    rec = dict(step=step, size=size, batch=B)
    tile = synth(1, 256, 256, 3, seed=1)                              # blobs, edges, stripes and noise, tiled to the size (the recipe is slow on the host)
    reps = -(-size // 256)
    img = torch.from_numpy(np.tile(tile, (B, reps, reps, 1))[:, :size, :size].copy()).to(dev)
    n = B * size * size
    if step == "canny":
        out, sweeps = ops.canny_u8(img)
        ms = timed(lambda: ops.canny_u8(img), iters=10)
        rec.update(ms=ms, sweeps=sweeps, edge_share=float((out == 255).float().mean()), bytes=n * 3 + n)
    elif step == "canny_stages":
        dx, dy, mag = ops.canny_grad(img)
        emap = ops.canny_nms(dx, dy, mag, 100, 200)
        _, sweeps = ops.canny_hysteresis(emap)
        rec.update(grad_ms=timed(lambda: ops.canny_grad(img)), nms_ms=timed(lambda: ops.canny_nms(dx, dy, mag, 100, 200)),
                   hysteresis_ms=timed(lambda: ops.canny_hysteresis(emap), iters=10), sweeps=sweeps,
                   grad_bytes=n * 3 + n * 8, nms_bytes=n * 8 + n, note="hysteresis_ms includes a copy of the map per call")
    elif step == "resize":
        big = size * 3 // 2
        src = torch.from_numpy(np.tile(tile, (B, -(-big // 256), -(-big // 256), 1))[:, :big, :big].copy()).to(dev)
        resize_u8(src, size, size)
        # horizontal pass reads big x big, writes big x size; vertical pass reads that, writes size x size
        rec.update(ms=timed(lambda: resize_u8(src, size, size)), src=big, bytes=B * 3 * (big * big + 2 * big * size + size * size))
    elif step == "u8_to_chw":
        rec.update(ms=timed(lambda: ops.img_u8_to_chw(img)), bytes=n * 3 + n * 3 * 4)
    elif step == "chw_to_u8":
        x = ops.img_u8_to_chw(img)
        xb = x.to(torch.bfloat16)
        rec.update(fp32_ms=timed(lambda: ops.img_chw_to_u8(x)), fp32_bytes=n * 3 * 4 + n * 3, bf16_ms=timed(lambda: ops.img_chw_to_u8(xb)),
                   bf16_bytes=n * 3 * 2 + n * 3)
    elif step == "blur":
        from unigen_amd.image import box_blur_constants, gaussian_box_radius
        c = box_blur_constants(gaussian_box_radius(10))
        fused, generic = lambda: ops.img_box_blur_u8(img, c, c, 3, fuse=True), lambda: ops.img_box_blur_u8(img, c, c, 3, fuse=False)
        same = bool(torch.equal(fused(), generic()))
        rounds = [(timed(fused), timed(generic)) for _ in range(7)]                 # interleaved: a drift of the machine hits both alike
        med = lambda v: sorted(v)[len(v) // 2]
        rec.update(fused_ms=med([r[0] for r in rounds]), generic_ms=med([r[1] for r in rounds]), fused_min_ms=min(r[0] for r in rounds),
                   generic_min_ms=min(r[1] for r in rounds), fused_max_ms=max(r[0] for r in rounds), generic_max_ms=max(r[1] for r in rounds), same_bytes=same,
                   constants=list(c), fused_bytes=n * 3 * 4, generic_bytes=n * 3 * 12, note="medians of 7 interleaved rounds of 20 calls; a launch reads and "
                   "writes the image once: 2 launches fused, 6 with fuse=0; each call also allocates its output and workspace")
    for k in [k for k in rec if k.endswith("bytes") and k != "same_bytes"]:
        ms = rec[k[:-5] + "ms"]
        rec[k[:-5] + "GBps"] = round(rec[k] / ms / 1e6, 1)
    print("IMAGE_BENCH", json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", nargs="+", choices=STEPS, default=STEPS)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.size, a.batch)
    lines = []
    for B in a.batches:
        for step in a.steps:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--size", str(a.size), "--batch", str(B)], cwd=ROOT,
                                   capture_output=True, text=True, timeout=STEP_SECONDS)
            except subprocess.TimeoutExpired:
                print(f"IMAGE_BENCH step {step} B={B}: no result within {STEP_SECONDS} s; stopping", flush=True)
                return 1
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("IMAGE_BENCH")]
            if r.returncode != 0 or not got:
                print(f"IMAGE_BENCH step {step} B={B} failed (exit {r.returncode}); stopping\n{r.stderr[-2000:]}", flush=True)
                return 1
            print(got[-1], flush=True)
            lines.append(got[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
