"""AutoencoderDC (dc-ae-f32c32-sana geometry, synthetic weights) at 1024^2: the record behind profiles/dcae_bench.log.

    python tools/dcae_bench.py [--cells 1024x1,1024x4] [--rounds 5]
        decode and encode of ONE process per cell (size x batch), interleaved round by round (decode, encode, again ...), every timing a host clock
        around a call that ends in a device synchronise; median / min / max ms. One line of JSON per cell (DCAE_BENCH).
    python tools/dcae_bench.py --kernels
        each new kernel of csrc/dcae.hip at a shape of the 1024^2 pass, device events around 5 launches after 2 warm ones: counted bytes (operands read
        once + output written once) per second, beside ug_add_bf16 (two reads, one write) on a tensor of the output's size. One line each (DCAE_KERNEL).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dcae_bench.py --one-pass
    python tools/dcae_bench.py --classify DIR/*/*kernel_stats.csv
        one decode and one encode at 1024^2, B = 1, without a warm-up, and the split of its kernel time by class (DCAE_SPLIT).
AutoencoderKL (FLUX geometry, 8x, 16 channels) decodes / encodes 1024^2 in 13.6 / 7.7 ms on the same chip (README.md): the context printed
beside the cells."""
import argparse, csv, json, os, re, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser(); ap.add_argument("--cells", default="1024x1,1024x4"); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kernels", action="store_true"); ap.add_argument("--one-pass", action="store_true"); ap.add_argument("--classify", default=None)
a = ap.parse_args()

CLASSES = (("rmsnorm_bias_rows", ("rmsnorm_bias_rows_kernel",)), ("msconv_proj", ("msconv_proj_kernel",)), ("dc_shortcut", ("dc_shortcut_kernel",)),
           ("silu", ("Silu<",)), ("linear attention", ("linattn_",)), ("GLU dwconv", ("glu_dwconv3x3_kernel",)), ("layout", ("nchw_to_nhwc", "nhwc_to_nchw")))


def classify(path):
    rows = list(csv.DictReader(open(path)))
    t = lambda r: float(r["TotalDurationNs"]) / 1e6
    out = {}
    for r in rows:
        n = r["Name"]
        cls = next((c for c, keys in CLASSES if any(k in n for k in keys)), None)
        if cls is None:
            if "conv2d_nhwc_kernel" in n or re.search(r"gemm256_kernel<[^>]*, true>", n):          # <EPI, LORA, QKDH, CONV>
                cls = "convolutions"
            elif "gemm256_kernel" in n or "gemm128_kernel" in n or "gemm_f32" in n:
                cls = "GEMMs"
            else:
                cls = "other (torch: weight init, copies, fills)"
        e = out.setdefault(cls, dict(ms=0.0, calls=0))
        e["ms"] += t(r); e["calls"] += int(r["Calls"])
    own = sum(v["ms"] for c, v in out.items() if not c.startswith("other"))
    for v in out.values():
        v["ms"], v["share_of_own"] = round(v["ms"], 3), round(v["ms"] / own, 4)
    print("DCAE_SPLIT", json.dumps(dict(size=1024, batch=1, passes="one decode + one encode", own_kernel_ms=round(own, 2), classes=out)))


if a.classify:
    classify(a.classify); sys.exit(0)

import torch
from unigen_amd import lib as L, ops
from unigen_amd.dcae import DCAE_F32C32_SANA, AutoencoderDC

dev, BF = torch.device("cuda:0"), torch.bfloat16
g = torch.Generator(device=dev).manual_seed(0)


def kernels_report():
    cdll, st = L.load(), torch.cuda.current_stream().cuda_stream
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(BF)

    def timed(run):
        for _ in range(2): run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
        for s_, e_ in ev:
            s_.record(); run(); e_.record()
        torch.cuda.synchronize()
        return statistics.median(x.elapsed_time(y) for x, y in ev)

    def report(name, shape, nbytes, run, out):
        ms = timed(run)
        n = out.numel()
        u, v, w = rnd(n), rnd(n), torch.empty(n, device=dev, dtype=BF)
        add_ms = timed(lambda: L.check(cdll.ug_add_bf16(u.data_ptr(), n, v.data_ptr(), n, w.data_ptr(), n, 1, n, st), "add"))
        gbps, add_gbps = nbytes / ms / 1e6, 6.0 * n / add_ms / 1e6
        print("DCAE_KERNEL", json.dumps(dict(kernel=name, shape=shape, ms=round(ms, 4), counted_mb=round(nbytes / 1e6, 1), gbps=round(gbps, 1),
              add_same_size_ms=round(add_ms, 4), add_gbps=round(add_gbps, 1), ratio_to_add=round(gbps / add_gbps, 3))), flush=True)

    M = 1024 * 1024
    x, w, b = rnd(M, 128), rnd(128), rnd(128)
    report("ug_rmsnorm_bias_rows + ReLU", "rows 1024^2, C 128 (decoder norm_out)", 2 * 2 * x.numel(), lambda: ops.rmsnorm_bias_rows(x, w, b, 1e-5, relu=True, out=x), x)
    x, r, w, b = rnd(128 * 128, 512), rnd(128 * 128, 512), rnd(512), rnd(512)
    o = torch.empty_like(x)
    report("ug_rmsnorm_bias_rows + residual", "rows 128^2, C 512 (EfficientViTBlock)", 3 * 2 * x.numel(), lambda: ops.rmsnorm_bias_rows(x, w, b, 1e-5, residual=r, out=o), o)
    x, r, w, b = rnd(256 * 256, 512), rnd(256 * 256, 512), rnd(512), rnd(512)
    o = torch.empty_like(x)
    report("ug_rmsnorm_bias_rows + residual", "rows 256^2, C 512 (ResBlock)", 3 * 2 * x.numel(), lambda: ops.rmsnorm_bias_rows(x, w, b, 1e-5, residual=r, out=o), o)
    x = rnd(M, 128)
    report("ug_silu", "1024^2 x 128 (ResBlock, stage 0)", 2 * 2 * x.numel(), lambda: ops.silu(x, x), x)
    for H, C in ((128, 512), (64, 1024), (32, 1024)):
        G = 3 * C // 32
        x, wd, wp = rnd(H * H, 3 * C), rnd(25, 3 * C), rnd(G, 32, 32)
        o = torch.empty_like(x)
        report("ug_msconv_proj k 5", f"{H}^2, G {G} (width {C})", 2 * 2 * x.numel(), lambda: ops.msconv_proj(x, wd, wp, o, B=1, H=H, W=H, G=G), o)
    h, x = rnd(M, 128), rnd(M, 64)
    o = torch.empty(M // 4, 256, device=dev, dtype=BF)
    report("ug_dc_shortcut_down f 2, x_shuffle", "1024^2 x 128 -> 512^2 x 256", 2 * (h.numel() + x.numel() + o.numel()),
           lambda: ops.dc_shortcut(h, o, up=False, B=1, H=1024, W=1024, Cin=128, Cout=256, factor=2, x=x, x_shuffle=True), o)
    report("ug_dc_shortcut_down f 2, no x", "1024^2 x 128 -> 512^2 x 256", 2 * (h.numel() + o.numel()),
           lambda: ops.dc_shortcut(h, o, up=False, B=1, H=1024, W=1024, Cin=128, Cout=256, factor=2), o)
    h, x = rnd(M // 4, 256), rnd(M // 4, 512)
    o = torch.empty(M, 128, device=dev, dtype=BF)
    report("ug_dc_shortcut_up f 2, x_shuffle", "512^2 x 256 -> 1024^2 x 128", 2 * (h.numel() + x.numel() + o.numel()),
           lambda: ops.dc_shortcut(h, o, up=True, B=1, H=512, W=512, Cin=256, Cout=128, factor=2, x=x, x_shuffle=True), o)
    h = rnd(32 * 32, 1024)
    o = torch.empty(32 * 32, 32, device=dev, dtype=BF)
    report("ug_dc_shortcut_down f 1 (encoder out)", "32^2 x 1024 -> 32", 2 * (h.numel() + o.numel()),
           lambda: ops.dc_shortcut(h, o, up=False, B=1, H=32, W=32, Cin=1024, Cout=32, factor=1), o)


if a.kernels:
    kernels_report(); sys.exit(0)

m = AutoencoderDC(DCAE_F32C32_SANA, device=dev).init_synthetic_(0)
if a.one_pass:
    img = torch.randn(1, 3, 1024, 1024, generator=g, device=dev).to(BF)
    lat = torch.randn(1, 32, 32, 32, generator=g, device=dev).to(BF)
    m.decode(lat); m.encode(img); torch.cuda.synchronize(); sys.exit(0)
for cell in a.cells.split(","):
    size, B = (int(v) for v in cell.split("x"))
    img = torch.randn(B, 3, size, size, generator=g, device=dev).to(BF)
    lat = torch.randn(B, 32, size // 32, size // 32, generator=g, device=dev).to(BF)
    runs = (("decode", lambda: m.decode(lat).sample), ("encode", lambda: m.encode(img).latent))
    torch.cuda.reset_peak_memory_stats()
    for _, f in runs:
        f(); f()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in runs}
    for _ in range(a.rounds):
        for n, f in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(); ms[n].append((time.perf_counter() - t0) * 1e3)
    res = dict(size=size, batch=B, rounds=a.rounds, peak_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2),
               context="AutoencoderKL (8x, 16 channels) at 1024^2, B = 1: decode 13.6 ms, encode 7.7 ms")
    for n, v in ms.items():
        res[n + "_ms"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    print("DCAE_BENCH", json.dumps(res), flush=True)
    m._buf.clear(); del img, lat; torch.cuda.empty_cache()
