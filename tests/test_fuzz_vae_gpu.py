"""Seeded sweeps of the AutoencoderKL kernels (csrc/vae.hip, the CONV mode of gemm256_kernel) against the float64 references of
tests/vae_kernel_ref.py (themselves checked against torch and the oracle by tests/test_vae_kernel_ref_cpu.py): the implicit-GEMM convolution
on the 128^2 kernel, on the 256^2 route and its fp32 twin, GroupNorm (+ SiLU) in its generic, fast and fp32 forms, the row softmax in its
generic, fast and fp32 forms, the layout kernels and the latent sampling.

Tolerances (docs/PARITY_TOLERANCES.md, "AutoencoderKL kernel sweep"):
  - fp32 twins: rel-L2 <= 1e-5 against the fp64 truth, every row metric <= 1e-4.
  - bf16: every metric <= max(1.5 x the rounding-point variant's own value of that metric against the same truth, 2^-9). Convolution: rel-L2,
    worst pixel row, worst BORDER pixel row (a pixel with at least one padding tap), worst row of the last partial 128-row tile. GroupNorm:
    rel-L2, worst pixel row, worst row of a sample's last partial slab, worst (sample, group) block.
  - softmax bf16 per element: one bf16 ulp of the fp64 value plus 2^-20 (1 + |scale s - max|) relative.
  - layouts: copies exact; the latent un-scaling and the sampling within one bf16 ulp of the variant per element, their twins 1e-6 relative.
Every element around an output (guard rows above and below it, the leading-dimension padding of the softmax) is compared bit for bit with the
sentinel written before the call: out-of-bounds writes are looked for with in-bounds sentinels, never by provoking a fault. Kernel variants
that an environment switch selects (the 256^2 convolution route against the 128^2 kernel, the generic GroupNorm and softmax at the shapes the
fast kernels take) run in ONE child process, which prints a JSON line per case; its non-zero exit is the failure."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    os.environ["UG_ENV_DYNAMIC"] = "1"            # the child: switches are read per call
    os.environ["UG_CONV256_MIN_TILES"] = "1"
    sys.path.insert(0, ROOT)

from tests import vae_kernel_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -7.625                                     # exact in bf16
GUARD = 4
GEO = ("Ho", "Wo", "stride", "pad_t", "pad_l", "up")


def _guarded(rows, cols, dt, dev):
    """a [GUARD + rows + GUARD, cols] buffer of sentinels and its contiguous middle"""
    buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=dt, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    b = buf.cpu()
    return bool((b[:GUARD] == SENT).all() and (b[GUARD + rows:] == SENT).all())


def _refused(code, fn):
    from unigen_amd import lib as L
    with pytest.raises(L.UniGenHipError, match=rf"\(code {code}\)"):
        fn()


# ----------------------------------------------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------------------------------------------
def _conv_once(c, dt, dev, cin, cout):
    """-> dict(got, m, b, guard, mismatch, ...): one call of ug_conv2d_nhwc[_f32] on case c with its metrics and their bounds"""
    from unigen_amd import ops
    g = torch.Generator().manual_seed(5000 + c["seed"])
    x, w, b, R = VR.conv_data(c, g, cin, cout)
    truth, var, border = VR.conv2d(x, w, b, R, **{k: c[k] for k in GEO})
    M = c["B"] * c["Ho"] * c["Wo"]
    buf, out = _guarded(M, cout, dt, dev)
    Rd = None
    if R is not None:
        Rd = R.reshape(M, cout).to(dt).to(dev)
        if c["res"] == "alias":                    # the residual is read from `out` itself; the guard rows sit around the shared buffer
            out.copy_(Rd)
            Rd = out
    ops.conv2d_nhwc(x.reshape(-1, cin).to(dt).to(dev), w.to(dt).to(dev), None if b is None else b.to(dt).to(dev), out, B=c["B"], H=c["H"], W=c["W"], Ho=c["Ho"],
                    Wo=c["Wo"], KH=c["KH"], KW=c["KW"], stride=c["stride"], pad_t=c["pad_t"], pad_l=c["pad_l"], up=c["up"], residual=Rd)
    torch.cuda.synchronize()
    got = out.cpu().to(F64).reshape(truth.shape)
    is_bf = dt == BF
    m = VR.conv_metrics(got, truth, border)
    bd = VR.bounds(VR.conv_metrics(VR.bf16(var), truth, border), is_bf)
    mis = VR.mismatch(got, var) if is_bf and R is not None and got.numel() >= VR.MISMATCH_MIN else None
    return dict(got=got, m=m, b=bd, guard=_guards_intact(buf, M), mismatch=mis, finite=bool(torch.isfinite(got).all()))


def _conv_judge(name, r, c):
    assert r["guard"], ("written outside its [B Ho Wo, Cout] rows", name, c)
    assert r["finite"], (name, c)
    VR.judge(name, r["m"], r["b"], c)
    if r["mismatch"] is not None:
        print(f"{name}: share of elements that differ from the rounded variant {r['mismatch']:.4f} (bound {VR.MISMATCH_MAX})")
        assert r["mismatch"] <= VR.MISMATCH_MAX, ("bf16(acc + bias) + R is not what was rounded", name, r["mismatch"], c)


def _conv_refusal(c, dt, dev, cin, cout):
    from unigen_amd import ops
    M = c["B"] * c["Ho"] * c["Wo"]
    buf, out = _guarded(M, cout, dt, dev)
    x = torch.zeros(c["B"] * c["H"] * c["W"], cin, dtype=dt, device=dev)
    w = torch.zeros(cout, c["KH"], c["KW"], cin, dtype=dt, device=dev)
    code = VR.conv_check(dict(c, Cin=cin, Cout=cout), dt == BF)
    assert code != VR.OK, c
    _refused(code, lambda: ops.conv2d_nhwc(x, w, None, out, B=c["B"], H=c["H"], W=c["W"], Ho=c["Ho"], Wo=c["Wo"], KH=c["KH"], KW=c["KW"], stride=c["stride"],
                                           pad_t=c["pad_t"], pad_l=c["pad_l"], up=c["up"]))
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENT).all()), ("a refused call wrote its output", c)


@pytest.mark.parametrize("seed", range(VR.CONV_SEEDS))
def test_conv2d_random_geometries(gpu, seed):
    """the 128^2 convolution kernel and the fp32 twin on one drawn geometry (kernel 1..7 x 1..7, stride 1..4, any top / left padding inside the
    kernel, with and without the folded nearest-2x upsampling, the largest output conv_check admits or a smaller one); every eighth seed is a
    geometry conv_check refuses: the documented code, the output untouched"""
    c = VR.conv_case(seed)
    for dt, cin, cout in ((BF, c["Cin"], c["Cout"]), (F32, c["Cin32"], c["Cout32"])):
        if c["refuse"]:
            _conv_refusal(c, dt, gpu, cin, cout)
            continue
        _conv_judge(f"conv2d {str(dt)[6:]} seed {seed} (M {c['B'] * c['Ho'] * c['Wo']}, {cin} -> {cout}, {c['KH']}x{c['KW']} s{c['stride']} up{c['up']})",
                    _conv_once(c, dt, gpu, cin, cout), c)


@pytest.mark.parametrize("mode", list(VR.VAE_GEOMETRIES))
@pytest.mark.parametrize("cin,cout", VR.VAE_CHANNELS)
def test_conv2d_vae_call_shapes(gpu, cin, cout, mode):
    """the (Cin, Cout) pairs unigen_amd/vae.py calls with - conv_in (3 padded to 64), the resnets, conv_out (3 padded to 8), the encoder's
    conv_out (2 x 16) - in its three geometries, at a small spatial size"""
    c = VR.vae_conv_case(cin, cout, mode)
    for dt in (BF, F32):
        _conv_judge(f"conv2d {str(dt)[6:]} {mode} {cin} -> {cout}", _conv_once(c, dt, gpu, cin, cout), c)


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ----------------------------------------------------------------------------------------------------------------------------------
def _gn_once(c, dt, dev, slab):
    from unigen_amd import ops
    x, ga, be = VR.gn_data(c, torch.Generator().manual_seed(6000 + c["seed"]))
    if dt == BF:
        x = x.to(BF).to(F32)                       # the truth is taken from the inputs as the kernel sees them
    truth, var = VR.groupnorm(x, ga, be, c["G"], c["eps"], c["silu"])
    B, HW, C = x.shape
    buf, out = _guarded(B * HW, C, dt, dev)
    ops.groupnorm_nhwc(x.reshape(B * HW, C).to(dt).to(dev), ga.to(dt).to(dev), be.to(dt).to(dev), out, B=B, HW=HW, groups=c["G"], eps=c["eps"], silu=c["silu"])
    torch.cuda.synchronize()
    got = out.cpu().to(F64).reshape(B, HW, C)
    return dict(m=VR.gn_metrics(got, truth, c["G"], slab), b=VR.bounds(VR.gn_metrics(var, truth, c["G"], slab), dt == BF), guard=_guards_intact(buf, B * HW),
                finite=bool(torch.isfinite(got).all()))


def _gn_judge(name, r, c):
    assert r["guard"], ("written outside its [B HW, C] rows", name, c)
    assert r["finite"], (name, c)
    VR.judge(name, r["m"], r["b"], c)


@pytest.mark.parametrize("seed", range(VR.GN_SEEDS))
def test_groupnorm_random_shapes(gpu, seed):
    """the bf16 kernels (the fast pair where groupnorm_impl dispatches to it, the generic pair elsewhere) and the fp32 twin; group means of
    0 ... 64 standard deviations, channels 100 x apart inside a group, constant samples (variance 0: beta, finite), samples 1000 x apart"""
    c = VR.gn_case(seed)
    tag = f"seed {seed} (B {c['B']}, HW {c['HW']}, C {c['C']}, G {c['G']}, {c['data']}" + (f" {c['ratio']}" if c["data"] == "offset" else "") + ")"
    _gn_judge(f"groupnorm bf16 {'fast' if VR.gn_fast(c) else 'generic'} {tag}", _gn_once(c, BF, gpu, 256 if VR.gn_fast(c) else 64), c)
    _gn_judge(f"groupnorm f32 {tag}", _gn_once(c, F32, gpu, 64), c)


@pytest.mark.parametrize("c", VR.GN_REFUSALS, ids=lambda c: f"C{c['C']}G{c['G']}")
@pytest.mark.parametrize("dt", [BF, F32])
def test_groupnorm_refuses_what_it_documents(gpu, c, dt):
    from unigen_amd import ops
    buf, out = _guarded(c["B"] * c["HW"], c["C"], dt, gpu)
    x, v = torch.ones(c["B"] * c["HW"], c["C"], dtype=dt, device=gpu), torch.ones(c["C"], dtype=dt, device=gpu)
    _refused(c["code"], lambda: ops.groupnorm_nhwc(x, v, v, out, B=c["B"], HW=c["HW"], groups=c["G"]))
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENT).all()), ("a refused call wrote its output", c)


# ----------------------------------------------------------------------------------------------------------------------------------
# softmax
# ----------------------------------------------------------------------------------------------------------------------------------
def _softmax_once(c, dt, dev):
    from unigen_amd import ops
    S, s0 = VR.softmax_data(c, torch.Generator().manual_seed(7000 + c["seed"]))
    rows, cols = c["rows"], c["cols"]
    truth, var, arg = VR.softmax_rows(s0, cols, c["scale"])          # data "offset": the truth of the un-offset scores
    buf = torch.full((rows + 2 * GUARD, c["ld_p"]), SENT, dtype=dt, device=dev)
    ops.softmax_rows(S.to(dev)[:, :cols], buf[GUARD:GUARD + rows, :cols], c["scale"])
    torch.cuda.synchronize()
    b = buf.cpu()
    got = b[GUARD:GUARD + rows, :cols].to(F64)
    guard = _guards_intact(buf, rows) and bool((b[GUARD:GUARD + rows, cols:] == SENT).all())
    m = dict(zip(("rel_l2", "worst_row"), VR.err(got, truth)[:2]))
    bd = VR.bounds(dict(zip(("rel_l2", "worst_row"), VR.err(var, truth)[:2])), dt == BF)
    over = float(((got - truth).abs() / VR.softmax_elem_bound(truth, arg)).max()) if dt == BF else 0.0
    return dict(m=m, b=bd, guard=guard, elem=over, rowsum=float((got.sum(1) - 1).abs().max()), finite=bool(torch.isfinite(got).all()))


def _softmax_judge(name, r, c):
    assert r["guard"], ("written outside its rows x cols", name, c)
    assert r["finite"], (name, c)
    VR.judge(name, r["m"], r["b"], c)
    print(f"{name}: worst element error / (one bf16 ulp + 2^-20 (1 + |arg|) relative) {r['elem']:.3f}, |row sum - 1| {r['rowsum']:.2e}")
    assert r["elem"] <= 1.0, (name, r["elem"], c)


@pytest.mark.parametrize("c", VR.softmax_cases(), ids=lambda c: f"{c['rows']}x{c['cols']}-{c['data']}-{c['seed']}")
def test_softmax_rows_cases(gpu, c):
    """bf16 (the single-read kernel where softmax_impl dispatches to it - whole multiples of 1024 columns, positive scale - and the generic kernel
    elsewhere, a negative scale included) and the fp32 twin, on views into wider buffers; scores with a common offset of 1e4 must give the
    un-offset result"""
    tag = f"{c['rows']} x {c['cols']} (ld {c['ld_s']} / {c['ld_p']}), scale {c['scale']:.4f}, {c['data']}"
    fast = VR.softmax_fast(c["cols"], c["scale"], c["ld_s"], c["ld_p"])
    _softmax_judge(f"softmax bf16 {'fast' if fast else 'generic'} {tag}", _softmax_once(c, BF, gpu), c)
    _softmax_judge(f"softmax f32 {tag}", _softmax_once(c, F32, gpu), c)


# ----------------------------------------------------------------------------------------------------------------------------------
# layouts and sampling (through the C ABI: the ops layer allocates these outputs itself, which leaves no room for guard rows)
# ----------------------------------------------------------------------------------------------------------------------------------
def _call(base, dt, *args):
    from unigen_amd import lib as L, ops
    L.check(ops._fn(base, dt)(*args, ops._stream()), base)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", VR.LAYOUT_CASES, ids=str)
@pytest.mark.parametrize("dt", [BF, F32])
def test_layout_kernels(gpu, case, dt):
    B, C, H, W, Cp = case
    HW = H * W
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(8000 + B * C + Cp)).to(BF).to(dt)
    xd = x.to(gpu)
    for div, add in ((0.0, 0.0), (0.3611, 0.1159)):
        truth, var = VR.nchw_to_nhwc(x, Cp, div, add)
        buf, out = _guarded(B * HW, Cp, dt, gpu)
        _call("ug_nchw_to_nhwc", dt, xd.data_ptr(), out.data_ptr(), B, C, HW, Cp, div, add)
        got = out.cpu().to(F64).reshape(B, HW, Cp)
        assert _guards_intact(buf, B * HW), ("ug_nchw_to_nhwc wrote outside its rows", case)
        assert not got[..., C:].any(), ("padding channels are not zero", case)
        if div == 0.0:
            assert torch.equal(got, truth), case
            nhwc = out
        elif dt == BF:
            far = (got - var).abs() / VR.bf16_ulp(var).clamp_min(1e-300)
            print(f"nchw_to_nhwc bf16 {case}: {int((got != var).sum())} of {got.numel()} elements differ from the variant, at most {float(far.max()):.2f} ulp")
            assert float(far.max()) <= 1.0, case
        else:
            e = VR.err(got[..., :C], truth[..., :C])[0]
            print(f"nchw_to_nhwc f32 {case}: rel-L2 {e:.3e} (bound 1e-6)")
            assert e <= 1e-6, case
    # the round trip of the plain copy
    buf, back = _guarded(B * C, HW, dt, gpu)
    _call("ug_nhwc_to_nchw", dt, nhwc.data_ptr(), back.data_ptr(), B, C, HW, Cp)
    assert _guards_intact(buf, B * C), ("ug_nhwc_to_nchw wrote outside its rows", case)
    assert torch.equal(back.cpu().reshape(B, C, H, W), x), case
    assert torch.equal(back.cpu().to(F64).reshape(B, C, H, W), VR.nhwc_to_nchw(nhwc.cpu(), B, C, H, W)), case


@pytest.mark.parametrize("c", VR.SAMPLE_CASES, ids=lambda c: f"B{c['B']}L{c['L']}Cp{c['Cp']}")
@pytest.mark.parametrize("dt", [BF, F32])
def test_vae_sample(gpu, c, dt):
    """log-variances over [-40, 30]: both clamps are reached; Cp = 2 L and wider; with and without the latent shift / scale"""
    B, L, HW, Cp = c["B"], c["L"], c["H"] * c["W"], c["Cp"]
    mom, noise = VR.sample_data(c, torch.Generator().manual_seed(9000 + Cp + L))
    sh, sc = (0.1159, 0.3611) if c["affine"] else (0.0, 1.0)
    truth, var = VR.vae_sample(mom, noise, L, sh, sc)
    buf, z = _guarded(B * L, HW, dt, gpu)
    md, nd = mom.reshape(B * HW, Cp).to(dt).to(gpu), noise.to(dt).to(gpu)
    _call("ug_vae_sample", dt, md.data_ptr(), Cp, nd.data_ptr(), z.data_ptr(), B, L, HW, sh, sc)
    got = z.cpu().to(F64).reshape(B, L, HW)
    assert _guards_intact(buf, B * L), ("ug_vae_sample wrote outside its rows", c)
    assert torch.isfinite(got).all(), c
    if dt == BF:
        far = (got - var).abs() / VR.bf16_ulp(var).clamp_min(1e-300)
        print(f"vae_sample bf16 {c}: {int((got != var).sum())} of {got.numel()} elements differ from the variant, at most {float(far.max()):.2f} ulp")
        assert float(far.max()) <= 1.0, c
    else:
        e = VR.err(got, truth)[0]
        print(f"vae_sample f32 {c}: rel-L2 {e:.3e} (bound 1e-6)")
        assert e <= 1e-6, c


# ----------------------------------------------------------------------------------------------------------------------------------
# the variants an environment switch selects: one child process
# ----------------------------------------------------------------------------------------------------------------------------------
def _child_main():
    dev = torch.device("cuda:0")
    strip = lambda r: {k: v for k, v in r.items() if k != "got"}
    for i, c in enumerate(VR.CONV256_CASES):
        os.environ["UG_CONV256"] = "0"
        small = _conv_once(c, BF, dev, c["Cin"], c["Cout"])
        os.environ["UG_CONV256"] = "1"
        big = _conv_once(c, BF, dev, c["Cin"], c["Cout"])
        print(json.dumps(dict(kind="conv256", i=i, identical=bool(torch.equal(small["got"], big["got"])), small=strip(small), big=strip(big))), flush=True)
    os.environ["UG_GN_FAST"] = "0"
    for seed in range(VR.GN_SEEDS):
        c = VR.gn_case(seed)
        if VR.gn_fast(c):
            print(json.dumps(dict(kind="gn_generic", i=seed, r=_gn_once(c, BF, dev, 64))), flush=True)
    os.environ["UG_SOFTMAX_FAST"] = "0"
    for i, c in enumerate(VR.softmax_cases()):
        if VR.softmax_fast(c["cols"], c["scale"], c["ld_s"], c["ld_p"]):
            print(json.dumps(dict(kind="softmax_generic", i=i, r=_softmax_once(c, BF, dev))), flush=True)


@pytest.fixture(scope="module")
def child(gpu):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]            # not restarted: the exit code is the failure
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            out[(d["kind"], d["i"])] = d
    return out


@pytest.mark.parametrize("i", range(len(VR.CONV256_CASES)))
def test_conv2d_on_the_256_route(child, i):
    """1x1 ... 5x5 kernels, strides 1 ... 4, the folded upsampling with stride 2, Cin / 64 in {2, 4, 8}, tiles that straddle sample boundaries, a
    separate and an aliased residual, no bias: the 256^2 GEMM kernel's per-tap gather gives the 128^2 kernel's bits, and both lie inside the
    float64 bounds, border rows included"""
    c = VR.CONV256_CASES[i]
    assert VR.conv_takes_256(c), ("the case would silently run on the 128^2 kernel", c)
    d = child[("conv256", i)]
    _conv_judge(f"conv2d 128^2 kernel, 256-route case {i}", d["small"], c)
    _conv_judge(f"conv2d 256^2 route case {i}", d["big"], c)
    assert d["identical"], ("the 256^2 route differs from the 128^2 kernel", c)


@pytest.mark.parametrize("seed", [s for s in range(VR.GN_SEEDS) if VR.gn_fast(VR.gn_case(s))])
def test_groupnorm_generic_kernels_at_the_fast_shapes(child, seed):
    c = VR.gn_case(seed)
    _gn_judge(f"groupnorm bf16 generic (UG_GN_FAST=0) seed {seed} (B {c['B']}, HW {c['HW']}, C {c['C']}, G {c['G']}, {c['data']})", child[("gn_generic", seed)]["r"], c)


@pytest.mark.parametrize("i", [i for i, c in enumerate(VR.softmax_cases()) if VR.softmax_fast(c["cols"], c["scale"], c["ld_s"], c["ld_p"])])
def test_softmax_generic_kernel_at_the_fast_shapes(child, i):
    c = VR.softmax_cases()[i]
    _softmax_judge(f"softmax bf16 generic (UG_SOFTMAX_FAST=0) {c['rows']} x {c['cols']}, {c['data']}", child[("softmax_generic", i)]["r"], c)


if __name__ == "__main__":
    _child_main()
