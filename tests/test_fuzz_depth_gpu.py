"""The depth-condition kernels (csrc/depth.hip) through the C ABI over the case table of tests/depth_kernel_cases.py, the BICUBIC route of resize_u8
against PIL's tables, and the tiny Depth Anything model at B = 3 with more than one GEMM tile per sample (tests/test_depth_kernel_cases_cpu.py
checks on the host what the table promises and that its judgement catches every slip).

Bounds (docs/PARITY_TOLERANCES.md, "Depth model", "Depth kernel sweep"), all in depth_kernel_cases.bound:
  bilinear, bicubic   |got - variant| <= k 2^-24 sum |w_i| |x_i| per element, the variant (depth_ref.*_variant) sharing the kernel's fp32 coordinates
                      and weights bit for bit, k the counted fp32 roundings of a tap's longest path (4 and 8); and the outer check against float64,
                      4 c 2^-24 scale with c computed here from torch's own fp32 CPU run on the case. bf16 adds half a bf16 ulp.
  deconv, head_out    the outer form alone, c live per case
  patches, relu, minmax   one right answer
Arenas. Every operand lies in a buffer of its own with guard rows before and behind; float guards, product-row gaps and the pad channels of the
head's input hold NaN, the surround of a uint8 image holds a byte no pixel has. Outputs are pre-filled with a sentinel that must survive everywhere
outside the window (guards, the gap behind a row of ld_out, the spare row); pad channels must be +0; a second launch gives the same bits. The bases
are 16-byte aligned and the cases' element offsets decide the path. Nothing outside the repository is read."""
import ctypes

import numpy as np
import pytest
import torch

from tests import depth_kernel_cases as K
from tests import depth_ref as R
from tests import image_ref
from tests.test_depth_kernel_cases_cpu import BICUBIC_PAIRS

pytestmark = pytest.mark.gpu

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
SENT, SENT_U8, NAN = -768.0, 0xA5, float("nan")          # -768 is exact in bf16
RECORD = {}                                              # (kernel, dtype name) -> worst error / bound; printed at the end of the module (pytest -s)


def teardown_module(module):
    for k, dt in sorted(RECORD):
        print(f"[depth-sweep] {k} {dt}: worst error / bound {RECORD[k, dt]:.4g}")


class Arena:
    """guard | off | window of n elements | guard, all `fill`; the base is 16-byte aligned and the guards are whole multiples of 16 bytes"""

    def __init__(self, dev, dtype, n, off=0, fill=NAN, guard=64):
        self.guard = (max(int(guard), 64) + 63) // 64 * 64
        self.lo, self.n, self.fill = self.guard + off, n, fill
        self.flat = torch.full((self.lo + n + self.guard,), fill, dtype=dtype, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.win = self.flat[self.lo:self.lo + n]

    @property
    def ptr(self):
        return self.win.data_ptr()

    def put(self, t):
        self.win.copy_(t.reshape(-1).to(self.flat.dtype))
        return self

    def bits(self):
        return self.flat.view(U8).clone()

    def read(self, keep=None):
        """-> (the window on the host, whether `fill` is intact outside it; keep: bool mask [n] of the window's elements the entry may write)"""
        flat = self.flat.cpu()
        win = flat[self.lo:self.lo + self.n]
        got = win.clone()
        if keep is None:
            win.fill_(self.fill)
        else:
            win[keep.reshape(-1)] = self.fill
        return got, bool(flat.isnan().all() if self.fill != self.fill else (flat == self.fill).all())


def entry(name, dt):
    from unigen_amd import lib as ULIB
    name = name + ("_f32" if dt == "f32" and name not in ("ug_bicubic_f32", "ug_minmax_to_u8") else "")
    fn = getattr(ULIB.load(), name)

    def run(*args):
        ULIB.check(fn(*args, torch.cuda.current_stream().cuda_stream), name)
        torch.cuda.synchronize()
    return run


def settle(kernel, cid, dt, got, intact, launch, out):
    """the checks every case shares: the sentinel, the judgement, the record, a second launch's bits"""
    assert intact, ("the sentinel outside the output window was overwritten", kernel, cid, dt)
    ratio, line = K.judge(kernel, cid, dt, got)
    print(f"[depth-sweep] {line}")
    RECORD[kernel, dt] = max(RECORD.get((kernel, dt), 0.0), ratio)
    assert ratio <= 1.0, line
    first = out.bits()
    launch()
    assert torch.equal(out.bits(), first), ("a second launch on the same buffers differs", kernel, cid, dt)


def _float_in(gpu, dt, t, off=0, guard=64):
    a = Arena(gpu, K.DTYPES[dt], t.numel(), off, NAN, guard).put(t)
    assert torch.equal(a.win.cpu().double().reshape(t.shape), t) or bool(t.isnan().any())        # the operand fits the entry's type
    return a


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", K.case_ids("bilinear"))
def test_bilinear(gpu, cid):
    c, d = K.case("bilinear", cid), K.data("bilinear", cid)
    (H, W), (Ho, Wo), B, C = c["src"], c["dst"], c["B"], c["C"]
    for dt in K.dtypes("bilinear"):
        x = _float_in(gpu, dt, d["x"], c["x_off"], guard=W * C)
        out = Arena(gpu, K.DTYPES[dt], B * Ho * Wo * C, c["out_off"], SENT, guard=Wo * C)
        launch = lambda: entry("ug_bilinear_nhwc", dt)(x.ptr, B, H, W, C, out.ptr, Ho, Wo, int(c["align"]))
        launch()
        got, intact = out.read()
        settle("bilinear", cid, dt, got.view(B, Ho, Wo, C), intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("bicubic"))
def test_bicubic(gpu, cid):
    c, d = K.case("bicubic", cid), K.data("bicubic", cid)
    (H, W), (Ho, Wo), B = c["src"], c["dst"], c["B"]
    x = _float_in(gpu, "f32", d["x"], guard=W)
    out = Arena(gpu, F32, B * Ho * Wo, 0, SENT, guard=Wo)
    launch = lambda: entry("ug_bicubic_f32", "f32")(x.ptr, B, H, W, out.ptr, Ho, Wo)
    launch()
    got, intact = out.read()
    settle("bicubic", cid, "f32", got.view(B, Ho, Wo), intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("deconv"))
def test_deconv_scatter(gpu, cid):
    c, d = K.case("deconv", cid), K.data("deconv", cid)
    B, h, w, f, Cout, Cp, ld = (c[k] for k in ("B", "h", "w", "f", "Cout", "Cp", "ld"))
    rows = B * h * w
    prod = Arena(gpu, F32, rows * ld, c["prod_off"], NAN, guard=ld)
    prod.win.view(rows, ld)[:, :f * f * Cout].copy_(d["prod"])                         # the gap behind every product row stays NaN
    for dt in K.dtypes("deconv"):
        bias = _float_in(gpu, dt, d["bias"], c["bias_off"])
        out = Arena(gpu, K.DTYPES[dt], rows * f * f * Cp, c["out_off"], SENT, guard=w * f * Cp)
        launch = lambda: entry("ug_deconv_scatter_nhwc", dt)(prod.ptr, ld, bias.ptr, out.ptr, B, h, w, f, Cout, Cp)
        launch()
        got, intact = out.read()
        settle("deconv", cid, dt, got.view(B, h * f, w * f, Cp), intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("head"))
def test_depth_head_out(gpu, cid):
    c, d = K.case("head", cid), K.data("head", cid)
    npix, C, Cp = c["npix"], c["C"], c["Cp"]
    for dt in K.dtypes("head"):
        x = Arena(gpu, K.DTYPES[dt], npix * Cp, c["x_off"], NAN, guard=Cp)
        x.win.view(npix, Cp)[:, :C].copy_(d["x"])                                       # the pad channels [C, Cp) stay NaN: never read into the sum
        w, bias = _float_in(gpu, dt, d["w"], c["w_off"]), _float_in(gpu, dt, d["bias"])
        out = Arena(gpu, F32, npix, 0, SENT)
        launch = lambda: entry("ug_depth_head_out", dt)(x.ptr, npix, C, Cp, w.ptr, bias.ptr, d["max_depth"], int(c["metric"]), out.ptr)
        launch()
        got, intact = out.read()
        settle("head", cid, dt, got, intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("patches"))
def test_img_u8_to_patches(gpu, cid):
    c, d = K.case("patches", cid), K.data("patches", cid)
    B, H, W, C, P, Kp, ld = (c[k] for k in ("B", "H", "W", "C", "P", "Kp", "ld"))
    wide, y0, x0 = K.patch_window(c, d["img"])
    Hw, Ww = wide.shape[1:3]
    img = Arena(gpu, U8, wide.numel(), 0, 255, guard=Ww * C).put(wide)
    rows = B * (H // P) * (W // P)
    f3 = lambda v: (ctypes.c_float * 3)(*v)
    keep = torch.zeros(rows + 1, ld, dtype=torch.bool)                                   # a spare row behind the last; the gap behind every row's Kp columns
    keep[:rows, :Kp] = True
    for dt in K.dtypes("patches"):
        out = Arena(gpu, K.DTYPES[dt], (rows + 1) * ld, c["out_off"], SENT, guard=ld)
        launch = lambda: entry("ug_img_u8_to_patches", dt)(img.ptr + (y0 * Ww + x0) * C, Hw * Ww * C, Ww * C, B, H, W, C, P, 1 / 255, f3(R.IMAGENET_MEAN),
                                                           f3(R.IMAGENET_STD), out.ptr, ld, Kp)
        launch()
        got, intact = out.read(keep)
        settle("patches", cid, dt, got.view(rows + 1, ld)[:rows, :Kp], intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("minmax"))
def test_minmax_to_u8(gpu, cid):
    from unigen_amd import ops
    c, d = K.case("minmax", cid), K.data("minmax", cid)
    B, HW, ch = c["B"], c["HW"], c["ch"]
    x = Arena(gpu, F32, B * HW, c["d_off"], NAN, guard=c["W"]).put(d["d"])
    out = Arena(gpu, U8, B * HW * ch, c["out_off"], SENT_U8, guard=c["W"] * ch)
    ws = torch.full((ops.minmax_workspace_bytes(B, HW),), 0xFF, dtype=U8, device=gpu)   # NaN bit patterns: the workspace needs no initialisation
    launch = lambda: entry("ug_minmax_to_u8", "f32")(x.ptr, B, HW, out.ptr, ch, ws.data_ptr(), ws.numel())
    launch()
    got, intact = out.read()
    settle("minmax", cid, "f32", got.view(B, HW, ch), intact, launch, out)


@pytest.mark.parametrize("cid", K.case_ids("relu"))
def test_relu(gpu, cid):
    """NaN propagates and -0 stays -0, as torch.relu (include/unigen_hip.h states it); in place gives the same bits"""
    c, d = K.case("relu", cid), K.data("relu", cid)
    for dt in K.dtypes("relu"):
        x = _float_in(gpu, dt, d["x"], c["x_off"])
        out = Arena(gpu, K.DTYPES[dt], c["n"], c["out_off"], SENT)
        launch = lambda: entry("ug_relu", dt)(x.ptr, out.ptr, c["n"])
        launch()
        got, intact = out.read()
        settle("relu", cid, dt, got, intact, launch, out)
        entry("ug_relu", dt)(x.ptr, x.ptr, c["n"])                                      # in place; the guards around x stay NaN
        again, guards = x.read()
        assert guards and torch.equal(again.view(torch.int16 if dt == "bf16" else torch.int32), got.view(torch.int16 if dt == "bf16" else torch.int32)), (cid, dt)


# ---- BICUBIC resize_u8 against PIL's tables (tests/test_depth_kernel_cases_cpu.py: resize_pil_tables is PIL's BICUBIC on these pairs) --------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("pair", BICUBIC_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_bicubic_resize_u8(gpu, pair, C):
    from unigen_amd.image import resize_u8
    (H, W), (h, w) = pair
    img = image_ref.synth(3, H, W, 3, seed=47)[..., :C]
    want = np.stack([R.resize_pil_tables(a, h, w) for a in img])
    src = torch.from_numpy(np.ascontiguousarray(img)).to(gpu)
    assert np.array_equal(resize_u8(src[:1], h, w, filter="bicubic").cpu().numpy(), want[:1])
    assert np.array_equal(resize_u8(src, h, w, filter="bicubic").cpu().numpy(), want)                  # B = 3, image by image
    wide = torch.full((3, H + 2, W + 3, C), 255, dtype=U8, device=gpu)                                 # a strided view
    wide[:, 1:H + 1, 3:].copy_(src)
    assert np.array_equal(resize_u8(wide[:, 1:H + 1, 3:], h, w, filter="bicubic").cpu().numpy(), want)


def test_bicubic_resize_u8_large_ratio_takes_the_unstaged_path(gpu):
    """A workgroup's 256 outputs read more input bytes than the staged span holds: 16 x 20000 x 3 -> 16 x 300."""
    from unigen_amd.image import resize_u8
    img = image_ref.synth(1, 16, 20000, 3, seed=9)
    assert np.array_equal(resize_u8(torch.from_numpy(img).to(gpu), 16, 300, filter="bicubic").cpu().numpy()[0], R.resize_pil_tables(img[0], 16, 300))


# ---- the model at B = 3 with more than one tile per sample ------------------------------------------------------------------------------------------------
SIDE, BATCH = 238, 3                                    # a 17 x 17 grid: N = 289 patch rows and T = 290 tokens per sample, which no tile size divides


@pytest.fixture(scope="module")
def wide_refs():
    """float64 truth and the two yardsticks (depth_ref in fp32, and with bf16 rounding points: tests/test_depth_ref_cpu.py shows that both land on
    transformers' own errors), stage by stage, computed once"""
    sd = R.random_state(R.TINY)
    u8 = R.images(SIDE, SIDE, BATCH)
    pv = R.pixel_values(u8)
    run = lambda **kw: dict(R.stage_list(R.forward(sd, R.TINY, pv, **kw)))
    return dict(sd=sd, u8=u8, truth=run(), f32=run(dtype=F32), bf16=run(round_bf16=True))


def _stages(model, u8):
    depth, st = model(pixel_u8=u8.to(model.device), return_stages=True)
    got = {"embeddings": st["embeddings"], "predicted_depth": depth}
    for grp in ("feature_maps", "reassembled", "fused"):
        got.update({f"{grp}.{i}": t for i, t in enumerate(st[grp])})
    return got


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_model_with_several_tiles_per_sample(gpu, wide_refs, dt):
    """The patch-embedding GEMM with r_map = (N, 0) and c_map = (N, T) (a broadcast residual and a class-row gap) and the neck's a_map = (N, T), at
    N = 289 and B = 3. rel-L2 to float64 stage by stage within 4x (fp32 twins) / 1.25x (bf16) of the yardstick's; and every sample's depth in the
    batch within the same bound of the run of that sample alone, which a row map that sent a sample's rows to its neighbour would break."""
    from unigen_amd.depth import DepthAnythingForDepthEstimation
    margin = 4.0 if dt == "f32" else 1.25
    m = DepthAnythingForDepthEstimation(R.TINY, device=gpu, dtype=K.DTYPES[dt])
    m.load_state_dict(wide_refs["sd"])
    got = _stages(m, wide_refs["u8"])
    truth, yard = wide_refs["truth"], wide_refs[dt]
    assert got["embeddings"].shape == (BATCH, 290, 128)
    for k, want in truth.items():
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        e, y = R.rel_l2(got[k].float().cpu(), want), R.rel_l2(yard[k], want)
        print(f"[depth-sweep] model 238x238 B=3 {dt} {k}: {e:.3e} (yardstick {y:.3e}, ratio {e / y:.2f})")
        RECORD[f"model.{k.split('.')[0]}", dt] = max(RECORD.get((f"model.{k.split('.')[0]}", dt), 0.0), e / (margin * y))
        assert e <= margin * y, (k, e, y)
    depth = got["predicted_depth"].float().cpu()
    assert 0.3 <= float((depth > 0).double().mean()) <= 0.98
    for b in range(BATCH):
        alone = m(pixel_u8=wide_refs["u8"][b:b + 1].to(gpu)).float().cpu()[0]
        want, y = truth["predicted_depth"][b], R.rel_l2(yard["predicted_depth"][b], truth["predicted_depth"][b])
        e_alone, e_batch, apart = R.rel_l2(alone, want), R.rel_l2(depth[b], want), R.rel_l2(depth[b], alone.double())
        print(f"[depth-sweep] model 238x238 {dt} sample {b}: batch {e_batch:.3e}, alone {e_alone:.3e}, batch against alone {apart:.3e} (yardstick {y:.3e})")
        assert max(e_alone, e_batch, apart) <= margin * y, (b, e_alone, e_batch, apart, y)
