"""AutoencoderKL (FLUX geometry) at 1024^2: decode and encode latency, per-call conv shapes. usage: python tools/vae_bench.py [--size 1024] [--batch 1]
--tiled [--size 2048] [--rounds 5]: untiled against tiled (enable_tiling(), default tile sizes 1024 / 128 / 0.25) decode and encode of ONE process,
interleaved round by round (untiled decode, tiled decode, untiled encode, tiled encode, again ...), every timing a host clock around calls that end in a
device synchronise; then one instrumented pass with a device-event pair around every ug_vae_tile_blend launch for the blend's share of the tiled time.
--flash [--rounds 5] [--cells 1024x1,1024x4,2048x1,4096x1]: the default attention route against enable_flash_attention() in ONE process, per cell (size x
batch) decode and encode interleaved round by round (default decode, flash decode, default encode, flash encode, again ...), median ms of host clocks around
calls that end in a device synchronise, and torch.cuda.max_memory_allocated of one call of each route on an empty workspace; 4096 runs the flash route only
(the default route's [HW, HW] scratch, about 275 GB, cannot be allocated). Then ug_flash_attn_fwd_wide alone at each cell's token count: device events
around 3 launches after 2 warm ones, TFLOP/s of 4 B N^2 512. One line of JSON per cell (profiles/vae_flash_bench.log)."""
import argparse, os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unigen_amd.vae import AutoencoderKL

ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=None); ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--tiled", action="store_true"); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--flash", action="store_true"); ap.add_argument("--cells", default="1024x1,1024x4,2048x1,4096x1"); a = ap.parse_args()
a.size = a.size or (2048 if a.tiled else 1024)
dev = torch.device("cuda:0")
def flash_report():
    import statistics
    from unigen_amd import ops
    vae = AutoencoderKL(device=dev, dtype=torch.bfloat16).init_synthetic_(seed=0)
    g = torch.Generator(device=dev).manual_seed(0)
    rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
    for cell in a.cells.split(","):
        size, B = (int(x) for x in cell.split("x"))
        routes = ("flash",) if size >= 4096 else ("default", "flash")
        img = torch.randn(B, 3, size, size, generator=g, device=dev).to(torch.bfloat16)
        lat = torch.randn(B, 16, size // 8, size // 8, generator=g, device=dev).to(torch.bfloat16)
        def call(route, op):
            vae.use_flash_attention = route == "flash"
            return vae.decode(lat).sample if op == "decode" else vae.encode(img).latent_dist._m
        res, outs = dict(size=size, batch=B, tokens=(size // 8) ** 2, rounds=a.rounds), {}
        for op in ("decode", "encode"):
            for route in routes:                           # peak memory of ONE call on an empty workspace (inputs and weights included); also the warm-up
                vae._ws.clear(); torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                outs[route, op] = call(route, op).clone(); torch.cuda.synchronize()
                res[f"{op}_{route}_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
                res[f"{op}_{route}_peak_over_resident_gb"] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 2)
        for op in ("decode", "encode"):
            for route in routes:
                call(route, op)
        torch.cuda.synchronize()
        ms = {(r_, op): [] for r_ in routes for op in ("decode", "encode")}
        for _ in range(a.rounds):
            for op in ("decode", "encode"):
                for route in routes:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    call(route, op)
                    torch.cuda.synchronize(); ms[route, op].append((time.perf_counter() - t0) * 1e3)
        for (route, op), v in ms.items():
            res[f"{op}_{route}_ms"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
        if "default" in routes:
            res["decode_flash_vs_default_relL2"] = round(rel(outs["flash", "decode"], outs["default", "decode"]), 5)
            res["encode_flash_vs_default_relL2"] = round(rel(outs["flash", "encode"], outs["default", "encode"]), 5)
        # the kernel alone, on N(0, 1) operands at the mid-block's shape: [B*N, 512] q, k, v, one launch over the batch
        vae._ws.clear(); outs.clear(); torch.cuda.empty_cache()
        N = (size // 8) ** 2
        q, k, v = (torch.randn(B * N, 512, generator=g, device=dev).to(torch.bfloat16) for _ in range(3))
        o, st = torch.empty_like(q), (512, N * 512)
        run = lambda: ops.flash_attn(q, k, v, o, batches=B, heads=1, dh=512, Lq=N, Lkv=N, q_strides=st, k_strides=st, v_strides=st, o_strides=st)
        for _ in range(2): run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
        for s_, e_ in ev:
            s_.record(); run(); e_.record()
        torch.cuda.synchronize()
        t = statistics.median(x.elapsed_time(y) for x, y in ev)
        res["attn_kernel_ms"] = round(t, 3); res["attn_kernel_tflops"] = round(4.0 * B * N * N * 512 / (t * 1e-3) / 1e12, 1)
        del q, k, v, o
        print("VAE_FLASH_BENCH", json.dumps(res), flush=True)
if a.flash:
    flash_report(); sys.exit(0)
vae = AutoencoderKL(device=dev, dtype=torch.bfloat16)
vae.init_synthetic_(seed=0)
g = torch.Generator(device=dev).manual_seed(0)
img = torch.randn(a.batch, 3, a.size, a.size, generator=g, device=dev).to(torch.bfloat16)
lat = torch.randn(a.batch, 16, a.size // 8, a.size // 8, generator=g, device=dev).to(torch.bfloat16)
from unigen_amd import ops
_flops = [0.0]
_conv = ops.conv2d_nhwc
def _counting_conv(x, w, bias, out, *, B, H, W, Ho, Wo, KH, KW, **kw):
    _flops[0] += 2.0 * B * Ho * Wo * w.shape[0] * KH * KW * w.shape[-1]
    return _conv(x, w, bias, out, B=B, H=H, W=W, Ho=Ho, Wo=Wo, KH=KH, KW=KW, **kw)
import unigen_amd.vae as _v
_v.ops.conv2d_nhwc = _counting_conv
def count(f):
    _flops[0] = 0.0; f(); return _flops[0]
def timeit(f, n=5):
    f(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e3
def tiled_report():
    import statistics
    def mode(on, f):
        def run():
            vae.enable_tiling(on); return f()
        return run
    runs = [("decode_untiled", mode(False, lambda: vae.decode(lat).sample)), ("decode_tiled", mode(True, lambda: vae.decode(lat).sample)),
            ("encode_untiled", mode(False, lambda: vae.encode(img).latent_dist._m)), ("encode_tiled", mode(True, lambda: vae.encode(img).latent_dist._m))]
    outs = {}
    for name, f in runs:                                   # warm-up of every shape the timed window uses; the outputs serve the difference below
        outs[name] = f().float(); torch.cuda.synchronize()
    rel = lambda x, y: float((x - y).norm() / y.norm())
    ms = {name: [] for name, _ in runs}
    for _ in range(a.rounds):
        for name, f in runs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(2): f()
            torch.cuda.synchronize(); ms[name].append((time.perf_counter() - t0) / 2 * 1e3)
    res = dict(size=a.size, batch=a.batch, rounds=a.rounds, tile_sample_min_size=vae.tile_sample_min_size, tile_latent_min_size=vae.tile_latent_min_size,
               tile_overlap_factor=vae.tile_overlap_factor)
    for name, v in ms.items():
        res[name + "_ms"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    res["decode_tiled_vs_untiled_relL2"] = round(rel(outs["decode_tiled"], outs["decode_untiled"]), 4)          # different by design: per-tile GroupNorm / attention
    res["encode_tiled_vs_untiled_relL2"] = round(rel(outs["encode_tiled"], outs["encode_untiled"]), 4)
    # the blend launches' share: device events around each launch, in a pass of its own (the events cost host time, so it is not one of the timings above)
    blend = ops.vae_tile_blend
    for name, f in runs[1::2]:
        ev, nbytes = [], [0]
        def timed(tile, up, left, ul, out, extent):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); r = blend(tile, up, left, ul, out, extent); e.record(); ev.append((s, e))
            nbytes[0] += out.element_size() * out.shape[0] * out.shape[2] * out.shape[3] * (out.shape[1] + tile.stride(3))      # crop written + the tile's crop read (whole pixels)
            return r
        _v.ops.vae_tile_blend = timed
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); f(); e.record(); torch.cuda.synchronize()
        _v.ops.vae_tile_blend = blend
        total, b = s.elapsed_time(e), sum(x.elapsed_time(y) for x, y in ev)
        res[name + "_blend"] = dict(launches=len(ev), blend_ms=round(b, 3), pass_ms=round(total, 2), share=round(b / total, 4), crop_bytes=nbytes[0],
                                    crop_gbps=round(nbytes[0] / (b * 1e-3) / 1e9, 1))
    print("VAE_TILED_BENCH", json.dumps(res))
if a.tiled:
    tiled_report(); sys.exit(0)
dec = timeit(lambda: vae.decode(lat))
enc = timeit(lambda: vae.encode(img))
fd, fe = count(lambda: vae.decode(lat)), count(lambda: vae.encode(img))
print("VAE_BENCH", json.dumps(dict(size=a.size, batch=a.batch, decode_ms=round(dec, 2), encode_ms=round(enc, 2), decode_conv_tflop=round(fd / 1e12, 2),
      encode_conv_tflop=round(fe / 1e12, 2), decode_tflops_effective=round(fd / dec / 1e9, 1), encode_tflops_effective=round(fe / enc / 1e9, 1))))
