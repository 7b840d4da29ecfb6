"""The case table of the depth-condition kernel sweep (csrc/depth.hip behind ug_img_u8_to_patches, ug_relu, ug_deconv_scatter_nhwc, ug_bilinear_nhwc,
ug_depth_head_out, ug_bicubic_f32 and ug_minmax_to_u8): tests/test_fuzz_depth_gpu.py runs every case on the device through the C ABI inside guarded
arenas, tests/test_depth_kernel_cases_cpu.py checks on the host what each case promises (its vector / scalar path, the branch its name says), that
the rounding-point variants of depth_ref sit at torch's own fp32 distance from float64, that every slip (SLIPS: a reference with one deliberate
mistake) breaks the device-side judgement on some case, and that the correct reference, rounded as the entry rounds, passes it on all. Host only: no
GPU import. Operands are built on demand and seeded by the case's id.

Offsets (`*_off`) are in elements from a 16-byte aligned base; `path` is what the host's `vec` decision must come to for BOTH element types, by the
predicates VEC, restated from the entry points. Branches that only a named case enters:
  u8_to_patches  second trip of the `c0 += 1024` loop      P19-* (K = 1083, Kp = 1088: lanes 0..7 return), P64-* (K = 12288: twelve trips)
                 vec = 0                                   P14-c3-2x3-ld+3, P19-c3-1x2-ld+3 (ld_out fails the 16-byte rule), P14-c3-2x3-out+1 (the base does)
  deconv         ragged channels (Cout % 8 != 0, vec = 0)  f2-co1-cp8, f2-co20-cp24, f4-co20-cp24, f16-co1-cp8
                 vec = 0 with whole channels               f2-co96-cp128-3x5-ld+3, -bias+1, -out+1; pad groups (c0 >= Cout) under vec = 1: *-co24-cp64-*, *-co48-cp64-*
  head_out       ragged channels (C % 8 != 0)              C1, C7, C33, C100 (under vec = 1: C33-cp40, C100-cp104, C1-cp8)
                 vec = 0                                   C33-cp35 and C7-cp7 (a row that is no multiple of 16 bytes), C32-cp64-x+1, C32-cp64-w+1
  bilinear       vec = 0                                   4x3-9x7-x+1, 4x3-9x7-out+1
  relu           vec = 0                                   n4104-x+1, n4104-out+1
  minmax         second strided round (i += 64 * 1024)     every HW above 65536; extremes placed at 65536 (its first element) and 131071 (its last)
                 ragged tail (vec = 0, HW % 4 != 0)        257x523, 1x1023, 1x1025; extremes placed at HW - HW % 4 (the tail quad's first) and HW - 1
                 vec = 0 at HW % 4 == 0                    300x500-d+1, 300x500-out+1
"""
import functools
import zlib

import numpy as np
import torch

from tests import depth_ref as R

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
DTYPES = {"f32": F32, "bf16": BF}
ESIZE = {"f32": 4, "bf16": 2}
KERNELS = ("bilinear", "bicubic", "deconv", "head", "patches", "minmax", "relu")
TWINNED = ("bilinear", "deconv", "head", "patches", "relu")              # entries with an fp32 twin; bicubic and minmax are fp32 only
U = 2.0 ** -24
MARGIN = 4                                                               # the project's standing margin over torch's own fp32 error
MM_ROUND = 64 * 1024                                                     # elements a strided round of minmax_partial_kernel covers (MM_BLOCKS 1024)

_al = lambda off, es: (off * es) % 16 == 0
# the host code's `vec`, entry by entry (csrc/depth.hip, "host side"); es = sizeof(T)
VEC = {
    "bilinear": lambda c, es: _al(c["x_off"], es) and _al(c["out_off"], es),
    "relu": lambda c, es: _al(c["x_off"], es) and _al(c["out_off"], es),
    "deconv": lambda c, es: _al(c["prod_off"], 4) and c["ld"] % 4 == 0 and c["Cout"] % 8 == 0 and _al(c["bias_off"], es) and _al(c["out_off"], es),
    "head": lambda c, es: _al(c["x_off"], es) and _al(c["w_off"], es) and (c["Cp"] * es) % 16 == 0,
    "patches": lambda c, es: _al(c["out_off"], es) and (c["ld"] * es) % 16 == 0,
    "minmax": lambda c, es: c["HW"] % 4 == 0 and _al(c["d_off"], 4) and c["out_off"] % 4 == 0,
    "bicubic": lambda c, es: False,                                      # no vector path: one output per lane
}


def _bf(t):
    return t.to(BF).to(F64)


def half_ulp_bf16(t):
    """half a bf16 ulp (8 significant bits) of |t|, elementwise, float64"""
    t = t.double().abs().clamp_min(2.0 ** -126)
    return 0.5 * 2.0 ** (torch.floor(torch.log2(t)) - 7)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------
def _bilinear():
    out = []
    add = lambda tag, B, src, dst, C, aligns=(True, False), x_off=0, out_off=0: out.extend(
        dict(id=f"{tag}-{'ac' if a else 'hp'}", B=B, src=src, dst=dst, C=C, align=a, x_off=x_off, out_off=out_off, path="scalar" if x_off or out_off else "vec")
        for a in aligns)
    # the model's own call shapes (fusion stage 37 -> 74 -> 148 -> 296, the head 296 -> 518; B = 2 on a 74 x 37 grid)
    add("37-74-c8", 1, (37, 37), (74, 74), 8)
    add("37-74-c64", 1, (37, 37), (74, 74), 64, aligns=(False,))
    add("148-296-c8", 1, (148, 148), (296, 296), 8)
    add("296-518-c8", 1, (296, 296), (518, 518), 8)
    add("74x37-148x74-b2-c8", 2, (74, 37), (148, 74), 8)
    # shape edges
    add("1x9-4x20", 2, (1, 9), (4, 20), 8)
    add("7x1-15x3", 2, (7, 1), (15, 3), 8)
    add("5x6-1x11", 2, (5, 6), (1, 11), 8)                               # Ho = 1: with align_corners the row scale is 0
    add("6x5-9x1", 2, (6, 5), (9, 1), 8)
    add("100x60-37x23", 1, (100, 60), (37, 23), 8)                       # a non-integer downscale above 2
    add("5x7-identity", 2, (5, 7), (5, 7), 8)
    add("4x3-9x7-b3", 3, (4, 3), (9, 7), 8)
    # width edges: 48 pixels x C / 8 lanes = 144 and 1200, no multiple of 256; 1200 lanes are five workgroups
    add("3x4-6x8-c24", 1, (3, 4), (6, 8), 24)
    add("3x4-6x8-c200", 1, (3, 4), (6, 8), 200)
    add("4x3-9x7-x+1", 2, (4, 3), (9, 7), 8, x_off=1)
    add("4x3-9x7-out+1", 2, (4, 3), (9, 7), 8, out_off=1)
    return out


def _bicubic():
    rows = [("518-1080x1920", 1, (518, 518), (1080, 1920)), ("518-519x517", 1, (518, 518), (519, 517)), ("518-224", 1, (518, 518), (224, 224)),
            ("6x40-5x255", 2, (6, 40), (5, 255)), ("6x40-5x256", 2, (6, 40), (5, 256)), ("6x40-5x257", 2, (6, 40), (5, 257)),
            ("1x1-7x300", 2, (1, 1), (7, 300)), ("9x11-1x1", 2, (9, 11), (1, 1)),
            ("2x9-7x20", 2, (2, 9), (7, 20)), ("9x3-20x8", 2, (9, 3), (20, 8)), ("3x2-8x7", 2, (3, 2), (8, 7)), ("6x5-11x9-b3", 3, (6, 5), (11, 9))]
    return [dict(id=i, B=B, src=s, dst=d, path="scalar") for i, B, s, d in rows]


def _deconv():
    out = []

    def add(f, Cout, Cp, h=3, w=5, B=2, ld_extra=0, bias_off=0, out_off=0, path=None, tag=""):
        ld = f * f * Cout + ld_extra
        c = dict(id=f"f{f}-co{Cout}-cp{Cp}-{h}x{w}{tag}", B=B, h=h, w=w, f=f, Cout=Cout, Cp=Cp, ld=ld, prod_off=0, bias_off=bias_off, out_off=out_off)
        c["path"] = path or ("vec" if Cout % 8 == 0 and ld % 4 == 0 else "scalar")
        out.append(c)

    for Cout, Cp in ((1, 8), (20, 24), (24, 64), (48, 64), (96, 128), (384, 384)):
        add(2, Cout, Cp)
    for f in (1, 4, 16):
        add(f, 24, 64)
    add(16, 1, 8), add(4, 20, 24), add(1, 384, 384), add(16, 96, 128, B=1)
    add(2, 96, 128, h=1, w=1), add(2, 96, 128, h=37, w=37, B=1)                        # the model's shape; 3 x 5 is in the first loop
    add(2, 96, 128, ld_extra=8, tag="-ld+8")                                           # a gap behind every product row, NaN
    add(2, 96, 128, ld_extra=3, path="scalar", tag="-ld+3")
    add(2, 96, 128, bias_off=1, path="scalar", tag="-bias+1")
    add(2, 96, 128, out_off=1, path="scalar", tag="-out+1")
    return out


def _head():
    out = []

    def add(npix, C, Cp, metric, amp=2.0, x_off=0, w_off=0, path="vec", tag=""):
        out.append(dict(id=f"n{npix}-C{C}-cp{Cp}-{'sigmoid' if metric else 'relu'}{tag}", npix=npix, C=C, Cp=Cp, metric=metric, amp=amp, x_off=x_off, w_off=w_off,
                        path=path))

    widths = ((1, 8, "vec"), (7, 8, "vec"), (32, 64, "vec"), (33, 40, "vec"), (100, 104, "vec"), (33, 35, "scalar"), (7, 7, "scalar"))
    for i, npix in enumerate((1, 63, 65, 257)):
        for j, (C, Cp, path) in enumerate(widths):
            if (i + j) % 2 == 0 or npix == 257:                                        # every width at 257 pixels, every pixel count at four or three widths
                for metric in (False, True):
                    add(npix, C, Cp, metric, path=path)
    for metric in (False, True):
        add(518 * 518, 32, 32, metric)
        add(257, 32, 64, metric, amp=120.0, tag="-pm100")                              # conv3's output spans +-100: the sigmoid saturates both ways
        add(65, 32, 64, metric, x_off=1, path="scalar", tag="-x+1")
        add(65, 32, 64, metric, w_off=1, path="scalar", tag="-w+1")
    return out


def _patches():
    out = []

    def add(P, C, ph, pw, B=2, kp_extra=0, ld_extra=8, out_off=0, margin=(2, 3), path="vec", tag=""):
        Kp = (3 * P * P + 63) // 64 * 64 + kp_extra
        out.append(dict(id=f"P{P}-c{C}-{ph}x{pw}{tag}", B=B, P=P, C=C, H=ph * P, W=pw * P, Kp=Kp, ld=Kp + ld_extra, out_off=out_off, margin=margin, path=path))

    # 8 spare columns behind every row's Kp (the sentinel stays there) unless the tag says otherwise
    add(1, 3, 3, 5), add(1, 1, 3, 5), add(14, 3, 2, 3), add(14, 1, 2, 3), add(16, 3, 2, 1), add(16, 1, 1, 2)
    add(19, 3, 2, 1), add(19, 1, 1, 2), add(64, 3, 1, 2, B=1), add(64, 1, 1, 1)
    add(14, 3, 2, 3, kp_extra=64, tag="-kp+64")
    add(19, 3, 1, 1, kp_extra=64, tag="-kp+64")
    add(14, 3, 2, 3, ld_extra=0, tag="-ld=kp")                                         # rows back to back, as the model's call has them
    add(19, 3, 1, 2, ld_extra=0, tag="-ld=kp")
    add(14, 3, 2, 3, ld_extra=3, path="scalar", tag="-ld+3")
    add(19, 3, 1, 2, ld_extra=3, path="scalar", tag="-ld+3")
    add(14, 3, 2, 3, out_off=1, path="scalar", tag="-out+1")
    add(14, 3, 2, 3, margin=(0, 0), tag="-contiguous")                                 # as the model calls it; every other case is a window of a wider image
    return out


def mm_indices(HW):
    """where an extreme matters to minmax_partial_kernel: the ends, both sides of the first round's end, the last element of the second round, the
    first element of the tail quad (HW - HW % 4; the last quad when there is no ragged one)"""
    tail = HW - (HW % 4 or 4)
    return [i for i in (0, HW - 1, MM_ROUND - 1, MM_ROUND, tail, 2 * MM_ROUND - 1) if 0 <= i < HW]


def _minmax():
    out = []

    def add(H, W, ch, kind, lo=None, hi=None, d_off=0, out_off=0, tag=""):
        HW = H * W
        c = dict(id=f"{H}x{W}-ch{ch}-{kind}{'' if lo is None else f'-lo{lo}-hi{hi}'}{tag}", B=2, H=H, W=W, HW=HW, ch=ch, kind=kind, lo=lo, hi=hi, d_off=d_off, out_off=out_off)
        c["path"] = "vec" if HW % 4 == 0 and not d_off and not out_off else "scalar"
        out.append(c)

    n = 0
    for H, W in ((300, 500), (257, 523), (1, 1023), (1, 1025)):
        idx = list(dict.fromkeys(mm_indices(H * W)))
        for k, lo in enumerate(idx):                                                   # cyclic pairs: every index holds the minimum once and the maximum once
            add(H, W, (1, 3)[n % 2], "placed", lo, idx[(k + 1) % len(idx)])
            n += 1
    add(300, 500, 1, "placed", 65536, 149999, d_off=1, tag="-d+1")
    add(300, 500, 3, "placed", 149996, 0, out_off=1, tag="-out+1")
    add(300, 500, 3, "placed", 0, 131071, d_off=1, out_off=2, tag="-d+1-out+2")
    for kind in ("subnormal", "offset", "random"):
        add(33, 45, 1, kind), add(257, 523, 3, kind)
    return out


def _relu():
    rows = [("n8", 8, 0, 0), ("n4104", 4104, 0, 0), ("n4104-x+1", 4104, 1, 0), ("n4104-out+1", 4104, 0, 1), ("n4104-x+3-out+3", 4104, 3, 3)]
    return [dict(id=i, n=n, x_off=xo, out_off=oo, path="scalar" if xo or oo else "vec") for i, n, xo, oo in rows]


@functools.lru_cache(maxsize=None)
def cases(kernel):
    out = {"bilinear": _bilinear, "bicubic": _bicubic, "deconv": _deconv, "head": _head, "patches": _patches, "minmax": _minmax, "relu": _relu}[kernel]()
    assert len({c["id"] for c in out}) == len(out), kernel
    return tuple(out)


def case_ids(kernel):
    return [c["id"] for c in cases(kernel)]


def case(kernel, cid):
    return next(c for c in cases(kernel) if c["id"] == cid)


def dtypes(kernel):
    return ("f32", "bf16") if kernel in TWINNED else ("f32",)


# ---- operands (host tensors; the device test copies them into its arenas) ----------------------------------------------------------------------------
RELU_SPECIALS = (0.0, -0.0, float("nan"), float("inf"), float("-inf"), -1.5, 2.0 ** -126, -(2.0 ** -126))


@functools.lru_cache(maxsize=3)
def data(kernel, cid):
    """-> dict of host tensors. Float operands are float64 holding values the bf16 entry can hold wherever it stores bf16, so that both entries share
    one truth; uint8 and fp32-only operands have their own type."""
    c = case(kernel, cid)
    g = torch.Generator().manual_seed(zlib.crc32(f"{kernel}/{cid}".encode()))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    if kernel == "bilinear":
        return dict(x=_bf(2 * rn(c["B"], *c["src"], c["C"])))
    if kernel == "bicubic":
        return dict(x=(5 * rn(c["B"], *c["src"])).float().double())
    if kernel == "deconv":
        return dict(prod=(3 * rn(c["B"] * c["h"] * c["w"], c["f"] ** 2 * c["Cout"])).float().double(), bias=_bf(rn(c["Cout"])))
    if kernel == "head":
        return dict(x=_bf(c["amp"] * rn(c["npix"], c["C"])), w=_bf(0.3 * rn(c["C"])), bias=_bf(torch.tensor([0.5], dtype=F64)), max_depth=20.0 if c["metric"] else 1.0)
    if kernel == "patches":
        return dict(img=torch.randint(0, 255, (c["B"], c["H"], c["W"], c["C"]), generator=g, dtype=torch.uint8))        # 255 is the surround's byte
    if kernel == "relu":
        x = _bf(3 * rn(c["n"]))
        x[:len(RELU_SPECIALS)] = torch.tensor(RELU_SPECIALS, dtype=F64)
        return dict(x=x)
    assert kernel == "minmax"
    B, HW = c["B"], c["HW"]
    if c["kind"] == "placed":                                           # three values; the minimum and the maximum at exactly one index each, swapped in image 1
        d = torch.full((B, HW), 0.5, dtype=F32)
        d[0, c["lo"]], d[0, c["hi"]], d[1, c["hi"]], d[1, c["lo"]] = -2.0, 3.0, -2.0, 3.0
    elif c["kind"] == "subnormal":                                      # max - min = 6e-39, a subnormal float
        d = torch.tensor([0.0, 3e-39, 6e-39], dtype=F32)[torch.randint(0, 3, (B, HW), generator=g)]
    elif c["kind"] == "offset":                                         # a large offset with a small spread: 1e30 +- 1e24
        d = (torch.tensor(1e30, dtype=F64) + 1e24 * torch.randint(-1, 2, (B, HW), generator=g).double()).float()
    else:
        d = (10 * rn(B, HW)).float()
    return dict(d=d)


def patch_window(c, img):
    """the wider uint8 image a patches case reads a window of: the surround (margin rows above and below, margin columns left and right) holds 255, a
    byte no image pixel has -> (wide [B, H + 2 my, W + 2 mx, C], y0, x0)"""
    my, mx = c["margin"]
    wide = torch.full((c["B"], c["H"] + 2 * my, c["W"] + 2 * mx, c["C"]), 255, dtype=torch.uint8)
    wide[:, my:my + c["H"], mx:mx + c["W"]] = img
    return wide, my, mx


# ---- references and bounds ---------------------------------------------------------------------------------------------------------------------------
def _live_c(t32, truth, scale):
    """the constant torch's own fp32 CPU run needs on this case: max |fp32 - float64| / (2^-24 scale), at least 1"""
    return max(1.0, float(((t32.double() - truth).abs() / (U * scale)).max()))


@functools.lru_cache(maxsize=2)
def refs(kernel, cid):
    """-> dict. Bounded kernels: truth (float64), c (live, floor 1), scale, and for the interpolations variant / mag / t32 (torch's fp32 run). Exact
    kernels: want (the one right answer, per dtype name where it depends on it)."""
    c, d = case(kernel, cid), data(kernel, cid)
    if kernel == "bilinear":
        x = d["x"]
        truth, t32 = R.bilinear_nhwc(x, *c["dst"], c["align"]), R.bilinear_nhwc(x.float(), *c["dst"], c["align"])
        variant, mag = R.bilinear_variant(x, *c["dst"], c["align"])
        scale = float(x.abs().max())
        return dict(truth=truth, t32=t32, variant=variant, mag=mag, scale=scale, c=_live_c(t32, truth, scale), k=R.BILINEAR_K)
    if kernel == "bicubic":
        x = d["x"]
        truth, t32 = R.bicubic(x, *c["dst"]), R.bicubic(x.float(), *c["dst"])
        variant, mag = R.bicubic_variant(x, *c["dst"])
        scale = float(x.abs().max())
        return dict(truth=truth, t32=t32, variant=variant, mag=mag, scale=scale, c=_live_c(t32, truth, scale), k=R.BICUBIC_K)
    if kernel == "deconv":
        args = (c["B"], c["h"], c["w"], c["f"], c["Cout"], c["Cp"])
        truth, t32 = R.deconv_scatter(d["prod"], d["bias"], *args), R.deconv_scatter(d["prod"].float(), d["bias"].float(), *args)
        scale = float(max(d["prod"].abs().max(), d["bias"].abs().max()))
        return dict(truth=truth, scale=scale, c=_live_c(t32, truth, scale))
    if kernel == "head":
        args = (c["C"], d["w"], d["bias"], d["max_depth"], c["metric"])
        truth = R.head_out(d["x"], *args)
        t32 = R.head_out(d["x"].float(), c["C"], d["w"].float(), d["bias"].float(), d["max_depth"], c["metric"])
        scale = ((torch.relu(d["x"]) * d["w"].abs()).sum(-1) + d["bias"].abs()) * d["max_depth"]
        v = (torch.relu(d["x"]) * d["w"]).sum(-1) + d["bias"]                             # conv3's output
        return dict(truth=truth, scale=scale, c=_live_c(t32, truth, scale), v=v)
    if kernel == "patches":
        img = d["img"].expand(-1, -1, -1, 3)                                             # C = 1: the one byte under each channel's mean and std
        want = R.patch_rows(R.pixel_values(img), c["P"], c["Kp"])
        return dict(want={"f32": want, "bf16": want.to(BF)})
    if kernel == "relu":
        want = torch.relu(d["x"])
        return dict(want={n: want.to(t) for n, t in DTYPES.items()})
    assert kernel == "minmax"
    return dict(want=torch.from_numpy(np.stack([R.minmax_u8(a) for a in d["d"].numpy()])))


def bound(kernel, c, rf, dt):
    """-> [(reference, per-element bound)] the device result is judged against, float64. The interpolations on two levels: the variant with the
    counted k 2^-24 sum |w| |x| (derived: nothing measured), and float64 with 4 c 2^-24 scale, c live; deconv and head_out keep the second form.
    bf16 adds half a bf16 ulp per rounding the entry makes, taken at |reference| + the fp32 bound: the fp32 value that is rounded may lie that far
    out, in the next binade."""
    bf = dt == "bf16"
    outer = MARGIN * rf["c"] * U * (rf["scale"] + torch.zeros_like(rf["truth"]))
    if kernel in ("bilinear", "bicubic"):
        inner = rf["k"] * U * rf["mag"]
        if bf:
            inner, outer = inner + half_ulp_bf16(rf["variant"].abs() + inner), outer + half_ulp_bf16(rf["truth"].abs() + outer)
        return [(rf["variant"], inner), (rf["truth"], outer)]
    if bf:
        outer = outer + half_ulp_bf16(rf["truth"].abs() + outer)
        if kernel == "head" and c["metric"]:
            # three roundings: conv3's output v (passed on by the sigmoid's slope <= 1/4 and max_depth), the sigmoid, the product
            md = data("head", c["id"])["max_depth"]
            outer = outer + md * (0.25 * half_ulp_bf16(rf["v"].abs() + 1e-3) + half_ulp_bf16(torch.sigmoid(rf["v"])))
    if kernel == "deconv":
        outer = outer[..., :c["Cout"]]
        return [(rf["truth"][..., :c["Cout"]], outer)]
    return [(rf["truth"], outer)]


def judge(kernel, cid, dt, got):
    """-> (worst error / bound, or inf where an exact kernel differs or a pad channel is not +0, a line for the record). got: the entry's output window
    on the host in the entry's type - bilinear [B, Ho, Wo, C], bicubic [B, Ho, Wo], deconv [B, h f, w f, Cp], head [npix], patches [rows, Kp],
    minmax [B, HW, ch], relu [n]."""
    c, rf = case(kernel, cid), refs(kernel, cid)
    if kernel in ("patches", "relu"):
        want = rf["want"][dt]
        same = got.dtype == want.dtype and got.shape == want.shape and bool(((got == want) | (got.isnan() & want.isnan())).all())
        if kernel == "relu":
            num = ~want.isnan()                                                              # -0 stays -0; a NaN's sign and payload are free
            same = same and torch.equal(torch.signbit(got)[num], torch.signbit(want)[num])
        else:
            same = same and not bool(torch.signbit(got[:, 3 * c["P"] ** 2:]).any())          # the pad columns are +0
        return (0.0 if same else float("inf")), f"{kernel} {cid} {dt}: {'equal' if same else 'DIFFERS'}"
    if kernel == "minmax":
        same = got.shape == (c["B"], c["HW"], c["ch"]) and all(torch.equal(got[..., k], rf["want"]) for k in range(c["ch"]))
        return (0.0 if same else float("inf")), f"minmax {cid}: {'equal' if same else 'DIFFERS'}"
    g = got.double()
    worst = 0.0
    if kernel == "deconv":
        pad = g[..., c["Cout"]:]
        if not bool(((pad == 0) & ~torch.signbit(pad)).all()):
            worst = float("inf")
        g = g[..., :c["Cout"]]
    ratios = []
    for want, b in bound(kernel, c, rf, dt):
        err, live = (g - want).abs(), b > 0
        r = float((err[live] / b[live]).max()) if bool(live.any()) else 0.0
        if not bool(torch.isfinite(g).all()) or bool((err[~live] != 0).any()):              # a zero bound (every tap zero) asks for equality
            r = float("inf")
        ratios.append(r)
    worst = max([worst] + ratios)
    if kernel == "bilinear" and c["src"] == c["dst"] and not torch.equal(g, data(kernel, cid)["x"]):
        worst = float("inf")                                                                # equal sizes: a bit-exact copy
    return worst, f"{kernel} {cid} {dt}: " + " ".join(f"{r:.3f}" for r in ratios) + (f" (c {rf['c']:.1f})" if "c" in rf else "")


def as_entry(dt, val):
    """a float64 reference rounded as the entry rounds: fp32 arithmetic, then the store's type"""
    return val.float().to(DTYPES[dt])


# ---- slips: a reference with one deliberate mistake each; some case's judgement must fail on every one ---------------------------------------------------
def _minmax_slipped(c, d, keep):
    """the kernel's conversion with the extremes taken over the elements `keep` selects only"""
    out = []
    for a in d.numpy():
        lo, hi = a[keep].min(), a[keep].max()
        q = ((a - lo) / (hi - lo)) * np.float32(255) if hi > lo else np.zeros_like(a)
        out.append((q.astype(np.int64) & 255).astype(np.uint8))
    return torch.from_numpy(np.stack(out))[..., None].expand(-1, -1, c["ch"])


def _slip_interp(kernel, name):
    def run(c, d, dt):
        if kernel == "bilinear":
            return as_entry(dt, R.bilinear_variant(d["x"], *c["dst"], c["align"], slip=name)[0])
        return as_entry(dt, R.bicubic_variant(d["x"], *c["dst"], slip=name)[0])
    return run


def _slip_bias_in_pad(c, d, dt):
    y = R.deconv_scatter(d["prod"], d["bias"], c["B"], c["h"], c["w"], c["f"], c["Cout"], c["Cp"])
    y[..., c["Cout"]:] = d["bias"][torch.arange(c["Cp"] - c["Cout"]) % c["Cout"]]
    return as_entry(dt, y)


def _slip_kykx(c, d, dt):
    f, Cout = c["f"], c["Cout"]
    prod = d["prod"].reshape(-1, f, f, Cout).transpose(1, 2).reshape(-1, f * f * Cout)
    return as_entry(dt, R.deconv_scatter(prod, d["bias"], c["B"], c["h"], c["w"], f, Cout, c["Cp"]))


def _slip_head_no_relu(c, d, dt):
    v = (d["x"] * d["w"]).sum(-1) + d["bias"]
    return ((torch.sigmoid(v) if c["metric"] else torch.relu(v)) * d["max_depth"]).float()


def _slip_tail(c, d, dt):
    keep = np.arange(c["HW"]) < c["HW"] - c["HW"] % 4                                      # the ragged tail quad never read
    return _minmax_slipped(c, d["d"], keep)


def _slip_round2(c, d, dt):
    i = np.arange(c["HW"])
    return _minmax_slipped(c, d["d"], (i < MM_ROUND) | (i >= 2 * MM_ROUND))                # the loop's second trip never made


def _slip_patch_trip(c, d, dt):
    want = refs("patches", c["id"])["want"][dt].clone()
    want[:, 1024:] = 0                                                                     # only the first 128 x 8 columns written
    return want


# name -> (kernel, what a wrong kernel would return for (case, data, dtype name))
SLIPS = {
    "bilinear: half-pixel offset dropped": ("bilinear", _slip_interp("bilinear", "no_half_pixel")),
    "bilinear: negative coordinate not clamped": ("bilinear", _slip_interp("bilinear", "negative_not_clamped")),
    "bilinear: align_corners swapped": ("bilinear", _slip_interp("bilinear", "align_swapped")),
    "bicubic: A = -0.5": ("bicubic", _slip_interp("bicubic", "cubic_a_half")),
    "bicubic: taps clamped to [0, n - 2]": ("bicubic", _slip_interp("bicubic", "taps_clamped_short")),
    "deconv: bias added into the pad channels": ("deconv", _slip_bias_in_pad),
    "deconv: ky and kx swapped": ("deconv", _slip_kykx),
    "head: ReLU missing ahead of the dot product": ("head", _slip_head_no_relu),
    "minmax: tail quad dropped": ("minmax", _slip_tail),
    "minmax: second round dropped": ("minmax", _slip_round2),
    "patches: second column trip dropped": ("patches", _slip_patch_trip),
}


def correct(kernel, cid, dt):
    """the correct reference rounded as the entry rounds (the interpolations: their variant)"""
    rf = refs(kernel, cid)
    if "want" in rf:
        w = rf["want"]
        return w[dt] if isinstance(w, dict) else w[..., None].expand(-1, -1, case(kernel, cid)["ch"])
    if kernel != "head":
        return as_entry(dt, rf.get("variant", rf["truth"]))
    c, d = case(kernel, cid), data(kernel, cid)
    rnd = (lambda t: t.float().to(BF).double()) if dt == "bf16" else (lambda t: t.float().double())      # conv3's output, the activation, the product
    v = rnd(rf["v"])
    return rnd(rnd(torch.sigmoid(v) if c["metric"] else torch.relu(v)) * d["max_depth"]).float()
