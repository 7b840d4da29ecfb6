"""The depth condition on the device (unigen_amd/depth.py, csrc/depth.hip): every new kernel against a float64 restatement (tests/depth_ref.py), the
tiny Depth Anything model of tests/golden/depth_tiny.safetensors against the float64 run of transformers with transformers' own fp32 / bf16 error
as the yardstick, the pipeline (`estimate_depth`, `depth_image`, `Condition`) and one run at depth-anything-small's real geometry.

Bounds (docs/PARITY_TOLERANCES.md, "Depth model"): an fp32 twin may miss the float64 result by 4 c 2^-24 scale per element, c the constant torch's
own fp32 run on the CPU needs on the same cases (stored by the generator), scale the magnitude of the inputs; a bf16 entry by that plus half a bf16
ulp of the truth per rounding the entry makes. The kernels with exactly specified arithmetic (patches, ReLU, min-max) have one right answer."""
import os

import numpy as np
import pytest
import torch

from tests import depth_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
RECORD = {}                     # figures printed at the end of the module (pytest -s) and quoted in docs/PARITY_TOLERANCES.md


@pytest.fixture(scope="module")
def gold():
    from safetensors.torch import load_file
    g = load_file(os.path.join(ROOT, "tests", "golden", "depth_tiny.safetensors"))
    names = bytes(g["c.names"].tolist()).decode().split(",")
    g["c"] = dict(zip(names, g["c.values"].tolist()))
    return g


@pytest.fixture(scope="module")
def sd(gold):
    s = R.random_state(R.TINY)
    assert torch.equal(R.fingerprint(s), gold["w.fingerprint"])
    return s


@pytest.fixture(scope="module")
def truth(sd):
    """float64 stages of every case, computed once (tests/test_depth_ref_cpu.py pins depth_ref to transformers and to the stored tensors)."""
    return {name: dict(R.stage_list(R.forward(sd, R.TINY, R.pixel_values(R.case_images(name))))) for name in R.CASES}


@pytest.fixture(scope="module")
def models(gpu, sd):
    from unigen_amd.depth import DepthAnythingForDepthEstimation
    out = {}
    for dt in (F32, BF):
        m = DepthAnythingForDepthEstimation(R.TINY, device=gpu, dtype=dt)
        m.load_state_dict(sd)
        out[dt] = m
    return out


def half_ulp_bf16(t):
    """half a bf16 ulp (8 significant bits) of |t|, elementwise, float64"""
    t = t.double().abs().clamp_min(2.0 ** -126)
    return 0.5 * 2.0 ** (torch.floor(torch.log2(t)) - 7)


def check(name, got, want, scale, c, bf16_roundings=0, extra=None):
    """|got - want| <= 4 c 2^-24 scale (+ bf16_roundings half ulps of the truth, taken a binade generously at the fp32 bound's distance)."""
    bound = 4 * c * 2.0 ** -24 * (scale if isinstance(scale, torch.Tensor) else torch.tensor(float(scale), dtype=torch.float64))
    bound = bound + torch.zeros_like(want)
    if bf16_roundings:
        bound = bound + bf16_roundings * half_ulp_bf16(want.abs() + bound)
    if extra is not None:
        bound = bound + extra
    err = (got.double().cpu() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    key = name + (".bf16" if bf16_roundings else ".f32")
    RECORD[key] = max(RECORD.get(key, 0.0), ratio)
    assert ratio <= 1.0, (name, ratio)


def teardown_module(module):
    for k in sorted(RECORD):
        print(f"[depth] {k}: {RECORD[k]:.4g}")


# ---- kernels -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF])
def test_img_u8_to_patches(gpu, dt):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(5)
    big = torch.randint(0, 256, (2, 30, 50, 3), generator=g, dtype=torch.uint8)
    for view in (big[:, :28, :42].contiguous(), big[:, 1:29, 3:45]):                    # the second: byte strides that are no multiple of 4
        x = view.to(gpu) if view.is_contiguous() else big.to(gpu)[:, 1:29, 3:45]
        assert x.is_contiguous() == view.is_contiguous()
        want = R.patch_rows(R.pixel_values(view), 14)                                     # fp32, the processor's rounding points
        got = ops.img_u8_to_patches(x, 14, R.IMAGENET_MEAN, R.IMAGENET_STD, dtype=dt).cpu()
        assert got.shape == (2 * 2 * 3, 640) and (got[:, 588:] == 0).all()
        assert torch.equal(got, want.to(dt)), float((got.float() - want).abs().max())    # one right answer; bf16 rounds once, at the store
    gray = big[:1, :14, :28, :1].contiguous()
    got = ops.img_u8_to_patches(gray.to(gpu), 14, R.IMAGENET_MEAN, R.IMAGENET_STD, dtype=dt).cpu()
    assert torch.equal(got, R.patch_rows(R.pixel_values(gray.expand(-1, -1, -1, 3)), 14).to(dt))


@pytest.mark.parametrize("dt", [F32, BF])
@pytest.mark.parametrize("n", [8, 4104])
def test_relu(gpu, dt, n):
    from unigen_amd import ops
    x = (3 * torch.randn(n, generator=torch.Generator().manual_seed(n))).to(dt)
    xg = x.to(gpu)
    assert torch.equal(ops.relu(xg).cpu(), torch.relu(x))
    assert torch.equal(xg.cpu(), x)
    ops.relu(xg, xg)                                                                  # in place
    assert torch.equal(xg.cpu(), torch.relu(x))
    odd = torch.zeros(n + 8, dtype=dt, device=gpu)
    odd[2:n + 2] = x.to(gpu)                                                          # a base that is not 16-byte aligned
    assert torch.equal(ops.relu(odd[2:n + 2]).cpu(), torch.relu(x))


@pytest.mark.parametrize("dt", [F32, BF])
def test_deconv_scatter(gpu, gold, dt):
    from unigen_amd import ops
    for case in R.kernel_cases()["deconv_scatter"]:
        i = R.kernel_inputs("deconv_scatter", case)
        want, scale = R.kernel_truth("deconv_scatter", case)
        got = ops.deconv_scatter_nhwc(i["prod"].to(gpu), i["bias"].to(gpu, dt), B=2, h=case["h"], w=case["w"], f=case["f"], Cout=case["Cout"], Cp=case["Cp"])
        assert got.shape == want.shape and got.dtype == dt and (got[..., case["Cout"]:] == 0).all()
        check("deconv_scatter", got, want, scale, gold["c"]["deconv_scatter"], bf16_roundings=int(dt == BF))


@pytest.mark.parametrize("dt", [F32, BF])
def test_bilinear(gpu, gold, dt):
    from unigen_amd import ops
    for case in R.kernel_cases()["bilinear"]:
        x = R.kernel_inputs("bilinear", case)["x"]
        want, scale = R.kernel_truth("bilinear", case)
        got = ops.bilinear_nhwc(x.to(gpu, dt), *case["dst"], align_corners=case["align"])
        assert got.shape == want.shape
        check("bilinear", got, want, scale, gold["c"]["bilinear"], bf16_roundings=int(dt == BF))
        if case["src"] == case["dst"]:
            assert torch.equal(got.cpu(), x.to(dt))                                    # equal sizes: a copy


@pytest.mark.parametrize("dt", [F32, BF])
def test_depth_head_out(gpu, gold, dt):
    from unigen_amd import ops
    for case in R.kernel_cases()["head_out"]:
        i = R.kernel_inputs("head_out", case)
        want, scale = R.kernel_truth("head_out", case)
        got = ops.depth_head_out(i["x"].to(gpu, dt), i["w"].to(gpu, dt), i["bias"].to(gpu, dt), C_=32, max_depth=i["max_depth"], metric=case["metric"])
        assert got.dtype == F32 and got.shape == want.shape
        extra, roundings = None, int(dt == BF)
        if dt == BF and case["metric"]:
            # three roundings: conv3's output v (passed on by the sigmoid's slope <= 1/4 and max_depth), the sigmoid, the product
            v = (torch.relu(i["x"][..., :32].double()) * i["w"].double()).sum(-1) + i["bias"].double()
            extra = i["max_depth"] * (0.25 * half_ulp_bf16(v.abs() + 1e-3) + half_ulp_bf16(torch.sigmoid(v)))
        check("head_out", got, want, scale, gold["c"]["head_out"], bf16_roundings=roundings, extra=extra)


def test_bicubic_f32(gpu, gold):
    from unigen_amd import ops
    for case in R.kernel_cases()["bicubic"]:
        x = R.kernel_inputs("bicubic", case)["x"]
        want, scale = R.kernel_truth("bicubic", case)
        got = ops.bicubic_f32(x.to(gpu), *case["dst"])
        assert got.shape == want.shape
        check("bicubic", got, want, scale, gold["c"]["bicubic"])


def test_minmax_to_u8_is_numpys(gpu, gold):
    from unigen_amd import ops
    g = torch.Generator().manual_seed(9)
    imgs = {"stored": gold["img0.depth_up"][None], "negative": -5 - 3 * torch.rand(2, 33, 45, generator=g), "one pixel": torch.tensor([[[2.5]]]),
            "constant": torch.full((2, 7, 9), -1.25), "mixed": torch.stack([10 * torch.randn(31, 37, generator=g), torch.full((31, 37), 3.0)]),
            "quads": 4 * torch.randn(3, 64, 100, generator=g), "large": torch.randn(1, 300, 500, generator=g)}
    for name, d in imgs.items():
        want = np.stack([R.minmax_u8(a) for a in d.numpy()])
        dg = d.to(gpu)
        for ch in (1, 3):
            ws = torch.empty(ops.minmax_workspace_bytes(d.shape[0], d.shape[1] * d.shape[2]), dtype=torch.uint8, device=gpu)
            ws.fill_(0xFF)                                                            # NaN bit patterns: the workspace needs no initialisation
            got = ops.minmax_to_u8(dg, ch, ws)
            assert got.shape == (*d.shape, ch) and all(np.array_equal(got[..., c].cpu().numpy(), want) for c in range(ch)), (name, ch)
            other = ops.minmax_to_u8((100 - 7 * dg).contiguous(), ch, ws)             # dirties the workspace with another image's extremes
            again = ops.minmax_to_u8(dg, ch, ws)
            assert torch.equal(again, got) and other.shape == got.shape, (name, ch)
    assert np.array_equal(ops.minmax_to_u8(imgs["stored"].to(gpu))[0, :, :, 0].cpu().numpy(), gold["img0.depth_u8"].numpy())
    assert (ops.minmax_to_u8(imgs["constant"].to(gpu), 3) == 0).all()


def test_bicubic_resize_u8_is_pils(gpu, gold):
    from unigen_amd.image import resize_u8
    for tag in ("img0", "img1"):
        want = gold[tag + ".bicubic"]
        got = resize_u8(gold[tag + ".u8"][None].to(gpu), want.shape[0], want.shape[1], filter="bicubic")
        assert torch.equal(got[0].cpu(), want), tag
    lanczos = resize_u8(gold["img0.u8"][None].to(gpu), 56, 98)
    assert not torch.equal(lanczos[0].cpu(), gold["img0.bicubic"])                     # the default filter is still Lanczos


def test_refusals(gpu):
    from unigen_amd import lib, ops
    with pytest.raises(lib.UniGenHipError):
        ops.relu(torch.zeros(12, dtype=BF, device=gpu))                                 # n % 8
    with pytest.raises(lib.UniGenHipError):
        ops.bilinear_nhwc(torch.zeros(1, 2, 2, 12, dtype=BF, device=gpu), 4, 4, True)   # C % 8
    with pytest.raises(lib.UniGenHipError):
        ops.minmax_to_u8(torch.zeros(1, 4, 4, device=gpu), 2)
    with pytest.raises(lib.UniGenHipError):
        ops.minmax_to_u8(torch.zeros(1, 4, 4, device=gpu), 1, torch.empty(8, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError):
        ops.img_u8_to_patches(torch.zeros(1, 15, 28, 3, dtype=torch.uint8, device=gpu), 14, R.IMAGENET_MEAN, R.IMAGENET_STD)


# ---- the model on the fixture --------------------------------------------------------------------------------------------------------------------
def _run(model, name):
    depth, st = model(pixel_u8=R.case_images(name).to(model.device), return_stages=True)
    got = {"embeddings": st["embeddings"], "predicted_depth": depth}
    for grp in ("feature_maps", "reassembled", "fused"):
        got.update({f"{grp}.{i}": t for i, t in enumerate(st[grp])})
    return got


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_fp32_path(gold, truth, models, name):
    """rel-L2 to the float64 tensors within 4x the error of transformers' own fp32 run on that case, stage by stage."""
    got = _run(models[F32], name)
    for j, (k, want) in enumerate(truth[name].items()):
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        e, yard = R.rel_l2(got[k].cpu(), want), float(gold[name + ".err"][j, 0])
        print(f"[depth] {name} fp32 {k}: {e:.3e} (transformers fp32 {yard:.3e}, ratio {e / yard:.2f})")
        RECORD[f"model.f32.{k.split('.')[0]}"] = max(RECORD.get(f"model.f32.{k.split('.')[0]}", 0.0), e / yard)
        assert e <= 4 * yard, (name, k, e, yard)
    d = got["predicted_depth"]
    assert d.dtype == F32 and 0.3 <= float((d > 0).double().mean()) <= 0.98


@pytest.mark.parametrize("name", list(R.CASES))
def test_model_bf16_path(gold, truth, models, name):
    """rel-L2 at most 1.25x the error of transformers' own bf16 run on that case, stage by stage."""
    got = _run(models[BF], name)
    for j, (k, want) in enumerate(truth[name].items()):
        e, yard = R.rel_l2(got[k].float().cpu(), want), float(gold[name + ".err"][j, 1])
        print(f"[depth] {name} bf16 {k}: {e:.3e} (transformers bf16 {yard:.3e}, ratio {e / yard:.2f})")
        RECORD[f"model.bf16.{k.split('.')[0]}"] = max(RECORD.get(f"model.bf16.{k.split('.')[0]}", 0.0), e / yard)
        assert e <= 1.25 * yard, (name, k, e, yard)


def test_pad_channels_stay_zero_and_patches_equal_pixels(models):
    from unigen_amd.depth import DepthImageProcessor
    m = models[BF]
    u8 = R.case_images("g4x3").to(m.device)
    a = m(pixel_u8=u8)
    patches, grid, size = DepthImageProcessor(size=(56, 42)).preprocess(u8, dtype=BF)
    assert grid == (4, 3) and size == (56, 42)
    assert torch.equal(m(patches=patches, grid=grid), a)                              # 56x42 in: no resize, the same patches


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["img0", "img1"])
def test_estimate_depth_against_the_pipeline(gpu, gold, models, tag):
    from unigen_amd.depth import DepthImageProcessor, estimate_depth
    proc = DepthImageProcessor(size=56)
    img = gold[tag + ".u8"]
    out = estimate_depth(models[F32], img.to(gpu), proc)
    assert out["predicted_depth"].shape == img.shape[:2] and out["predicted_depth"].dtype == F32 and out["depth"].dtype == torch.uint8
    assert out["depth"].is_cuda and out["predicted_depth"].is_cuda
    diff = (out["depth"].cpu().int() - gold[tag + ".depth_u8"].int()).abs()
    share, yard = float((diff > 0).double().mean()), float(gold[tag + ".share_fp32"][0])
    print(f"[depth] {tag}: {int((diff > 0).sum())} of {diff.numel()} levels differ (share {share:.2e}; transformers fp32 against float64 {yard:.2e})")
    assert int(diff.max()) <= 1
    assert share <= 2 * yard, (share, yard)
    both = estimate_depth(models[F32], img[None].to(gpu), proc)
    assert isinstance(both, list) and len(both) == 1 and torch.equal(both[0]["depth"], out["depth"])


def test_depth_image_kinds_and_condition(gpu, gold, models):
    from PIL import Image
    from unigen_amd.condition import Condition, depth_image
    from unigen_amd.depth import DepthImageProcessor
    from tests.test_image_gpu import tiny_pipe
    proc, m = DepthImageProcessor(size=56), models[F32]
    img = gold["img1.u8"]
    t = depth_image(img.to(gpu), m, proc)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == (45, 33, 3) and t.dtype == torch.uint8
    assert torch.equal(t[..., 0], t[..., 1]) and torch.equal(t[..., 0], t[..., 2])
    a = depth_image(img.numpy(), m, proc)
    assert isinstance(a, np.ndarray) and np.array_equal(a, t.cpu().numpy())
    p = depth_image(Image.fromarray(img.numpy()), m, proc)
    assert isinstance(p, Image.Image) and p.mode == "RGB" and np.array_equal(np.array(p), a)
    c = depth_image(img.cpu(), m, proc)
    assert isinstance(c, torch.Tensor) and not c.is_cuda and torch.equal(c, t.cpu())
    gray = depth_image(img[..., 0].to(gpu), m, proc)
    assert gray.shape == (45, 33, 3)
    # the reference's condition: tokens and ids of the canny case's shapes, type_id 0
    pipe = tiny_pipe()
    big = torch.randint(0, 256, (35, 34, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)      # preprocess rounds to 32 x 32
    tok, ids, tid = Condition("depth", raw_img=depth_image(big.to(gpu), m, proc), no_process=True).encode(pipe)
    tok_c, ids_c, _ = Condition("canny", raw_img=big.to(gpu)).encode(pipe)
    assert tok.shape == tok_c.shape == (1, 64, 4 * pipe.vae.config.latent_channels) and ids.shape == ids_c.shape == (64, 3) and torch.equal(ids, ids_c)
    assert tid.shape == (64, 1) and bool((tid == 0).all())


# ---- real geometry -------------------------------------------------------------------------------------------------------------------------------
def test_real_geometry_bf16_against_fp32_twins(gpu, gold):
    """depth-anything-small's own config at 518x518: a 37x37 grid, 1370 tokens (a ragged attention length), K = 588 -> 640, neck widths 48 / 96 / 192
    padded to 64 / 128 / 192. No fixture: weights drawn on the device. The bf16 path against the fp32-twin path within the bound the tiny cases
    established: 1.25x the largest error transformers' own bf16 run shows against float64 on them."""
    from unigen_amd.depth import DepthAnythingForDepthEstimation
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(518.0), torch.arange(518.0), indexing="ij")
    img = torch.stack([128 + 100 * torch.sin(0.02 * yy + 0.013 * xx + c) for c in range(3)], -1) + 30 * torch.randn(518, 518, 3, generator=g)
    u8 = img.clamp(0, 255).to(torch.uint8)[None].to(gpu)
    m32 = DepthAnythingForDepthEstimation(device=gpu, dtype=F32).init_synthetic_(0)
    m16 = DepthAnythingForDepthEstimation(device=gpu, dtype=BF)
    m16.load_state_dict(m32.state_dict())
    assert m32._p["patch_w"].shape == (384, 640) and m32._p["n0.proj_w"].shape == (64, 384) and m32._p["n2.proj_w"].shape == (192, 384)
    d32, d16 = m32(pixel_u8=u8), m16(pixel_u8=u8)
    assert d32.shape == (1, 518, 518) and torch.isfinite(d32).all() and torch.isfinite(d16).all()
    pos = float((d32 > 0).double().mean())
    e = R.rel_l2(d16.cpu(), d32.cpu())
    bound = 1.25 * max(float(gold[n + ".err"][-1, 1]) for n in R.CASES)
    print(f"[depth] real geometry: positive share {pos:.2f}, spread {float(d32.max() - d32.min()):.1f}, bf16 against fp32 twins {e:.3e} (bound {bound:.3e})")
    assert 0.3 <= pos <= 0.98 and float(d32.max() - d32.min()) > 1
    assert e <= bound, (e, bound)
